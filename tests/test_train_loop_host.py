"""The pieces of ContrastiveEstimationTrainer.train that need no GPU, on CPU tensors: the per-step readback (_StepReadback: row
layout, delivery in order, the NaN step), the BatchNorm / step-count rollback (_NanRollback) and the diagonal scatter of the generic
route's loss gradient (_step_block_grads)."""
import math
from types import SimpleNamespace

import pytest
import torch

from cpc_audio_amd.contrastive_estimation_training import _NanRollback, _StepReadback, _ring_depth, _step_block_grads


class _Meter:
    def __init__(self):
        self.seen = []

    def update(self, v):
        self.seen.append(v)


class _Logger:
    def __init__(self, *extra):
        self.loss_meter, self.score_meter, self.steps = _Meter(), _Meter(), []
        for name in extra:
            setattr(self, name, _Meter())

    def log(self, step):
        self.steps.append(step)


def _trainer(logger, host_temperature=None):
    return SimpleNamespace(logger=logger, verbose=False, host_sync_interval=1, host_sync_lag=1, last_lr=None, last_grad_norm=None,
                           last_temperature=None, score_function=SimpleNamespace(temperature=host_temperature))


def _row(step, width):
    """Column c of step s holds s + c / 16 (exact in float32); no NaN indicator."""
    row = torch.tensor([step + c / 16 for c in range(width)], dtype=torch.float32)
    row[_StepReadback.NAN] = 0.0
    return row


def _readback(logger, clip=False, device_temp=None, temp_route=None, host_temperature=None):
    tr = _trainer(logger, host_temperature)
    return tr, _StepReadback(tr, optimizer=None, clip=clip, fused=False, on_gpu=False, device_temp=device_temp, temp_route=temp_route)


def _push_five(tr, rb, width):
    for s in range(5):
        tr.last_lr = 1e-3 * (s + 1)          # the step's rate rides along with its row
        if rb.temp_route == "host":
            tr.score_function.temperature = 0.5 - s / 16
        rb.push(s, _row(s, width))


def test_rows_are_delivered_in_order_and_keep_leaves_the_latest_pending():
    logger = _Logger("lr_meter")
    tr, rb = _readback(logger)
    assert rb.width == 6
    _push_five(tr, rb, 8)          # (a wider result cell: only the row's columns are kept)
    assert rb.flush(keep=1) is None
    assert logger.steps == [0, 1, 2, 3] and len(rb.pending) == 1
    assert rb.flush() is None
    assert logger.steps == [0, 1, 2, 3, 4] and rb.pending == []
    assert logger.loss_meter.seen == [float(s) for s in range(5)]                     # column 0
    assert logger.score_meter.seen == [s + 1 / 16 for s in range(5)]                  # column 1
    assert logger.lr_meter.seen == [1e-3 * (s + 1) for s in range(5)]
    assert tr.last_grad_norm is None and tr.last_temperature is None
    assert rb.flush() is None and logger.steps == [0, 1, 2, 3, 4]                     # nothing pending: nothing delivered twice


def test_logger_without_the_optional_meters_and_no_logger():
    logger = _Logger()
    tr, rb = _readback(logger, clip=True, temp_route="host", host_temperature=0.5)
    _push_five(tr, rb, 8)
    assert rb.flush() is None and logger.steps == [0, 1, 2, 3, 4]
    assert tr.last_grad_norm == 4 + 6 / 16 and tr.last_temperature == 0.5 - 4 / 16
    tr, rb = _readback(None)
    _push_five(tr, rb, 6)
    assert rb.flush(keep=2) is None and len(rb.pending) == 2


def test_clipping_widens_the_row_and_the_norm_follows_column_6():
    logger = _Logger("grad_norm_meter")
    tr, rb = _readback(logger, clip=True)
    assert rb.width == 8 and (rb.GRAD_NORM, rb.CLIP_COEF) == (6, 7)
    _push_five(tr, rb, 8)
    assert rb.flush(keep=1) is None
    assert logger.steps == [0, 1, 2, 3] and tr.last_grad_norm == 3 + 6 / 16
    assert rb.flush() is None
    assert logger.grad_norm_meter.seen == [s + 6 / 16 for s in range(5)] and tr.last_grad_norm == 4 + 6 / 16
    assert logger.loss_meter.seen == [float(s) for s in range(5)]
    assert logger.score_meter.seen == [s + 1 / 16 for s in range(5)]


def test_host_route_temperature_is_the_one_of_the_step_pushed():
    logger = _Logger("temperature_meter")
    tr, rb = _readback(logger, temp_route="host", host_temperature=0.5)
    assert rb.width == 6
    _push_five(tr, rb, 6)
    tr.score_function.temperature = 9.0          # a later step's value: not what the pending rows carry
    assert rb.flush(keep=1) is None
    assert logger.temperature_meter.seen == [0.5 - s / 16 for s in range(4)] and tr.last_temperature == 0.5 - 3 / 16
    assert rb.flush() is None and tr.last_temperature == 0.5 - 4 / 16


@pytest.mark.parametrize("clip", [False, True])
def test_device_temperature_sits_behind_the_other_columns(clip):
    logger = _Logger("temperature_meter", "grad_norm_meter")
    device_temp = SimpleNamespace(tstate=torch.zeros(8))
    tr, rb = _readback(logger, clip=clip, device_temp=device_temp, temp_route="device")
    col = 8 if clip else 6
    assert rb.width == col + 1 and rb.TEMPERATURE == col
    _push_five(tr, rb, col + 1)
    assert rb.flush() is None
    assert logger.temperature_meter.seen == [s + col / 16 for s in range(5)] and tr.last_temperature == 4 + col / 16
    assert logger.grad_norm_meter.seen == ([s + 6 / 16 for s in range(5)] if clip else [])


@pytest.mark.parametrize("how", ["indicator", "nan loss"])
def test_nan_step_is_returned_unlogged_and_clears_pending(how):
    logger = _Logger()
    tr, rb = _readback(logger)
    for s in range(5):
        row = _row(s, 6)
        if s == 2 and how == "indicator":
            row[5] = 1.0
        elif s == 2:
            row[0] = math.nan
        rb.push(s, row)
    assert rb.flush(keep=1) == 2
    assert logger.steps == [0, 1] and logger.loss_meter.seen == [0.0, 1.0]
    assert rb.pending == [] and not rb.bad_grad_norm


def test_finite_loss_under_a_raised_indicator_blames_the_gradient_norm():
    for norm, loss, bad in ((math.inf, 1.0, True), (math.nan, 1.0, True), (2.0, 1.0, False), (math.inf, math.nan, False)):
        logger = _Logger("grad_norm_meter")
        tr, rb = _readback(logger, clip=True)
        row = _row(0, 8)
        row[0], row[5], row[6] = loss, 1.0, norm
        rb.push(0, row)
        assert rb.flush() == 0 and rb.bad_grad_norm is bad, (norm, loss)
        assert logger.steps == [] and logger.grad_norm_meter.seen == [] and rb.pending == []
    tr, rb = _readback(_Logger())          # without clipping the row has no norm to blame
    row = _row(0, 8)
    row[5], row[6] = 1.0, math.inf
    rb.push(0, row)
    assert rb.flush() == 0 and not rb.bad_grad_norm


class _Toy(torch.nn.Module):
    def __init__(self, batchnorm=True):
        super().__init__()
        self.lin = torch.nn.Linear(4, 4)
        if batchnorm:
            self.bn = torch.nn.BatchNorm1d(4)


def _bn_state(model):
    return {n: b.clone() for n, b in model.named_buffers()}


def _move_bn(model, by):
    with torch.no_grad():
        model.bn.running_mean += by
        model.bn.running_var *= 1.0 + by
        model.bn.num_batches_tracked += 1


def test_rollback_restores_the_next_steps_statistics_and_this_steps_count():
    model, opt = _Toy(), SimpleNamespace(t=7)
    tr = SimpleNamespace(model=model, host_sync_interval=1, host_sync_lag=1)
    rollback = _NanRollback(tr, opt, fused=True)
    assert [len(group) for group in rollback.bufs] == [2, 1]          # float32 statistics and the int64 counter
    assert len(rollback.ring) == _ring_depth(tr) == 4
    s = 10
    _move_bn(model, 0.25)
    rollback.snapshot(s)
    _move_bn(model, 0.5)
    opt.t = 8
    rollback.snapshot(s + 1)
    want = _bn_state(model)
    _move_bn(model, 1.0)
    opt.t = 9
    rollback.snapshot(s + 2)
    _move_bn(model, 2.0)
    opt.t = 10
    rollback.restore(s)
    got = _bn_state(model)
    assert set(got) == set(want) and all(torch.equal(got[n], want[n]) for n in want)
    assert int(model.bn.num_batches_tracked) == 2 and opt.t == 7


def test_rollback_drops_entries_older_than_the_ring_and_grows_with_the_lag():
    model, opt = _Toy(), SimpleNamespace(t=0)
    tr = SimpleNamespace(model=model, host_sync_interval=1, host_sync_lag=1)
    rollback = _NanRollback(tr, opt, fused=True)
    for step in range(9):
        rollback.snapshot(step)
    assert sorted(rollback.snaps) == [5, 6, 7, 8] and len(rollback.ring) == 4
    slots = [id(rollback.snaps[k][0]) for k in sorted(rollback.snaps)]
    assert len(set(slots)) == 4          # every entry kept has a ring slot of its own
    tr.host_sync_lag = 3                 # raised while training: the ring grows on the next snapshot
    rollback.snapshot(9)
    assert len(rollback.ring) == 6 and sorted(rollback.snaps) == [5, 6, 7, 8, 9]


def test_rollback_without_batchnorm_or_off_the_fused_route_allocates_nothing():
    tr = SimpleNamespace(model=_Toy(batchnorm=False), host_sync_interval=1, host_sync_lag=1)
    opt = SimpleNamespace(t=3)
    rollback = _NanRollback(tr, opt, fused=True)
    assert rollback.bufs == [] and rollback.ring == []
    rollback.snapshot(0)
    opt.t = 4
    rollback.snapshot(1)
    opt.t = 5
    assert rollback.ring == [] and rollback.snaps[0] == (None, 3)
    rollback.restore(0)
    assert opt.t == 3          # the step count is still put back
    tr = SimpleNamespace(model=_Toy(), host_sync_interval=1, host_sync_lag=1)
    generic = _NanRollback(tr, opt, fused=False)
    generic.snapshot(0)
    assert generic.ring == [] and generic.snaps == {}


def test_step_block_grads_fill_only_the_equal_step_diagonal():
    B, K, ld = 3, 2, 8
    dS = torch.randn(K, B, ld, generator=torch.Generator().manual_seed(0))          # the padding columns hold values too
    d_loss = torch.tensor(0.75)
    d = _step_block_grads(dS, B, K, d_loss)
    assert d.shape == (B, K, B, K) and d.dtype == torch.float32
    for b in range(B):
        for k in range(K):
            for b2 in range(B):
                for k2 in range(K):
                    want = float(dS[k, b, b2] * d_loss) if k == k2 else 0.0
                    assert float(d[b, k, b2, k2]) == want, (b, k, b2, k2)
