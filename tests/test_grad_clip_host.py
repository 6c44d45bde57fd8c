"""Gradient clipping by global norm, what needs no GPU: the argument checks of cpc_grad_norm / cpc_adam_clip (refused before any
launch), the workspace size, the refusals of FusedAdam and ContrastiveEstimationTrainer, and the data-parallel ordering — with
clipping on, GradAllReduce issues no update before every piece's reduction has been waited for (gloo, two ranks)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer
from cpc_audio_amd.engine import FusedAdam, check_max_grad_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, F = C.c_longlong, C.c_float


def test_grad_norm_arguments_are_checked_before_any_launch():
    """Every refusal include/cpc_hip.h states for cpc_grad_norm returns CPC_EINVAL (-22) from the argument check: no kernel is
    launched, so this runs without a GPU."""
    lib = _hip.lib()
    P = C.c_void_p(0x1000)        # 16-byte aligned, never dereferenced
    s = C.c_void_p(0)
    assert lib.cpc_grad_norm(P, L(0), F(1.0), F(1.0), P, P, None, s) == -22                     # n == 0
    assert lib.cpc_grad_norm(P, L(-8), F(1.0), F(1.0), P, P, None, s) == -22                    # n < 0
    assert lib.cpc_grad_norm(None, L(64), F(1.0), F(1.0), P, P, None, s) == -22                 # no gradient
    for misaligned in (0x1004, 0x1008, 0x100c):
        assert lib.cpc_grad_norm(C.c_void_p(misaligned), L(64), F(1.0), F(1.0), P, P, None, s) == -22
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert lib.cpc_grad_norm(P, L(64), F(1.0), F(bad), P, P, None, s) == -22, bad          # max_norm not finite or not > 0
    assert lib.cpc_grad_norm(P, L(64), F(1.0), F(1.0), None, P, None, s) == -22                 # no workspace
    assert lib.cpc_grad_norm(P, L(64), F(1.0), F(1.0), P, None, None, s) == -22                 # no state
    # cpc_adam_clip: cpc_adam's checks and a coefficient pointer
    adam = (L(64), F(1e-3), F(0.9), F(0.999), F(1e-8))
    assert lib.cpc_adam_clip(P, P, P, P, *adam, 1, F(1.0), None, None, s) == -22                # no coefficient
    assert lib.cpc_adam_clip(P, P, P, P, *adam, 0, F(1.0), P, None, s) == -22                   # steps count from 1
    assert lib.cpc_adam_clip(P, None, P, P, *adam, 1, F(1.0), P, None, s) == -22
    assert lib.cpc_adam_clip(P, P, P, P, L(0), *adam[1:], 1, F(1.0), P, None, s) == -22


def test_grad_norm_workspace_is_one_float_per_workgroup():
    """A workgroup takes 256 threads x 8 loads x 4 floats = 8 192 elements of the vector body (the geometry the error bound of
    tests/test_grad_clip_gpu.py is computed from)."""
    ws = _hip.lib().cpc_grad_norm_workspace_floats
    assert [ws(n) for n in (-1, 0)] == [0, 0]
    assert [ws(n) for n in (1, 3, 4, 8192, 8195)] == [1] * 5
    assert [ws(n) for n in (8196, 16384, 16388)] == [2, 2, 3]
    assert ws(7414784) == 906 and ws(3 * 2 ** 20 + 1) == 384
    assert ws(2 ** 33) == 2 ** 20


class _Model:
    def __init__(self, n=100):
        self._flat_param, self._flat_grad = torch.zeros(n), torch.zeros(n)


def test_max_grad_norm_values():
    assert check_max_grad_norm(None) is None and check_max_grad_norm(2) == 2.0
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError):
            check_max_grad_norm(bad)
        with pytest.raises(ValueError):
            FusedAdam(_Model(), lr=1e-3, max_grad_norm=bad)
    with pytest.raises(NotImplementedError):          # clipped steps are not captured into a hipGraph
        FusedAdam(_Model(), lr=1e-3, device_step=True, max_grad_norm=1.0)
    plain = FusedAdam(_Model(), lr=1e-3)
    assert plain.max_grad_norm is None and not hasattr(plain, "clip_state")          # no new buffer without the keyword
    clipped = FusedAdam(_Model(), lr=1e-3, max_grad_norm=0.5)
    assert clipped.clip_state.shape == (4,) and clipped.max_grad_norm == 0.5


def test_trainer_refuses_up_front():
    """Before any GPU work (there is no model, dataset or device here to get as far as one): ValueError for a max_grad_norm that is
    not a positive finite number, NotImplementedError together with use_graph."""
    tr = ContrastiveEstimationTrainer(model=None, dataset=None)
    assert tr.max_grad_norm is None and tr.last_grad_norm is None
    for bad in (0, -0.5, float("nan"), float("inf")):
        tr.max_grad_norm = bad
        with pytest.raises(ValueError):
            tr.train(batch_size=4, max_steps=1)
    tr.max_grad_norm, tr.use_graph = 1.0, True
    with pytest.raises(NotImplementedError):
        tr.train(batch_size=4, max_steps=1)


WORKER = r'''
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from cpc_audio_amd.engine import FusedAdam, GradAllReduce
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank, world = dist.get_rank(), dist.get_world_size()
N = 100

class Model:
    pass

def shard(step, r):
    return torch.randn(N, generator=torch.Generator().manual_seed(100 * step + r))

class Recorder(FusedAdam):
    """FusedAdam with its launches replaced by records: what the device would be asked to do, and on what."""
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.launches, self.aheads, self.sync, self.total = [], [], None, None
    def _grad_norm(self, grad_scale):
        g = self.model._flat_grad
        assert self.sync.pending == [] and self.sync.split is None          # finish() has waited for every piece
        assert torch.equal(g, self.total), "the norm would be taken of a gradient that is not reduced yet"
        self.norm = float((g.double() * grad_scale).norm())
        return "coef"
    def _update(self, lo, hi, t, grad_scale, coef=None):
        assert coef == "coef", f"a piecewise update [{lo}, {hi}) was launched although clipping is on"
        self.launches.append((lo, hi, grad_scale, self.norm))

m = Model()
m._flat_param = torch.zeros(N)
opt = Recorder(m, lr=1e-3, max_grad_norm=0.25)
opt.after_update = lambda lo, hi, final: opt.aheads.append((lo, hi, final))
for step in range(3):
    m._flat_grad = shard(step, rank)
    total = shard(step, 0)
    for r in range(1, world):
        total = total + shard(step, r)
    sync = GradAllReduce(m, optimizer=opt)
    opt.sync, opt.total = sync, total
    opt.launches, opt.aheads = [], []
    sync.reduce_flag(torch.zeros(8))
    time.sleep(0.03 * ((rank + step) % world))          # the ranks reach their hooks at different times
    sync.hook(60, 100)
    time.sleep(0.02 * ((rank * 3 + step) % world))
    sync.hook(20, 60)
    assert opt.launches == [] and opt.aheads == []          # recorded, nothing issued
    assert opt._done_lo == 60                               # (the piece of the first hook was handed over at the second)
    sync.finish()
    assert opt.launches == [] and opt.aheads == [] and opt._done_lo == 20
    opt.step(grad_scale=sync.grad_scale)
    want = float((total.double() / world).norm())
    assert len(opt.launches) == 1, opt.launches
    lo, hi, scale, norm = opt.launches[0]
    assert (lo, hi, scale) == (0, N, 1.0 / world)           # the one update covers the whole buffer once
    assert abs(norm - want) <= 1e-12 * want, (norm, want)
    assert opt.aheads == [(0, N, True)] and opt._done_lo is None and opt.t == step + 1
    norms = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(norms, torch.tensor([norm], dtype=torch.float64))
    assert all(float(x) == norm for x in norms)             # every rank computes the same norm
    assert sync.describe()["covers_once"]
# a step() whose scale differs from the one the pieces were recorded with is refused, as without clipping
opt.update_range(50, N, 0.5)
try:
    opt.step(grad_scale=1.0)
    raise SystemExit("a mismatching grad_scale was accepted")
except ValueError:
    pass
if rank == 0:
    print("CLIP-DP-OK")
dist.destroy_process_group()
'''


def test_clipped_update_waits_for_every_reduction_gloo_world2(tmp_path):
    """engine.GradAllReduce with FusedAdam(max_grad_norm=...) attached, two ranks that reach their hooks at different times: the
    pieces are recorded, no update is issued from the hooks or from finish(), and step() issues ONE update over the whole buffer
    whose norm is that of the summed gradient times 1 / world (float64), the same on both ranks."""
    script = tmp_path / "worker_clip.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29667", WORLD_SIZE="2", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "CLIP-DP-OK" in outs[0]
