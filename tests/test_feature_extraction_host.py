"""Whole-recording feature extraction, the parts that need no GPU: the host schedule against a scalar restatement, the window
arithmetic and the hand-off in the float64 reference itself, the argument checks of cpc_stream_gather / cpc_feature_emit /
cpc_stream_carry (refused before any launch), and the refusals of the constructor."""
import ctypes as C

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd import feature_extraction as FE
import feature_extraction_reference as R


def _lengths(rf, ds, Tc):
    """The issue's edge lengths: no frame, one frame, one frame with ds - 1 samples to spare, two frames, and frame counts around the
    chunk size."""
    out = [rf - 1, rf, rf + ds - 1, rf + ds]
    out += [R.samples_for(f, rf, ds, extra=k % ds) for k, f in enumerate((Tc - 1, Tc, Tc + 1, 2 * Tc)) if f >= 1]
    return out


@pytest.mark.parametrize("Tc", [1, 2, 7, 64])
@pytest.mark.parametrize("streams", [1, 2, 3, 11])
@pytest.mark.parametrize("geometry", [(R.RF, R.DS), (7, 3)], ids=["small-encoder", "rf7-ds3"])
def test_schedule_against_scalar_restatement(geometry, streams, Tc):
    rf, ds = geometry
    lengths = _lengths(rf, ds, Tc)
    assert streams != 11 or streams > len(lengths)
    for order in (lengths, lengths[::-1], lengths[3:] + lengths[:3]):
        first = [int(v) for v in np.concatenate([[0], np.cumsum(order)[:-1]])]
        sched = FE.plan_schedule(first, order, rf, ds, streams, Tc)
        steps, frames, offsets = R.scalar_schedule(first, order, rf, ds, streams, Tc)
        assert sched.table.dtype == np.int64 and sched.table.shape == (len(steps), streams, 6)
        assert sched.table.tolist() == steps
        assert sched.frame_counts.tolist() == frames and sched.frame_offsets.tolist() == offsets
        R.check_table(sched.table, first, order, rf, ds, streams, Tc)
        assert int(sched.table[:, :, 2].sum()) == sum(frames)


def test_schedule_of_nothing():
    """Recordings without frames are legal and contribute nothing: no step at all."""
    sched = FE.plan_schedule([0, 10], [10, R.RF - 1], R.RF, R.DS, 4, 8)
    assert sched.table.shape == (0, 4, 6) and sched.frame_offsets.tolist() == [0, 0, 0]
    assert FE.frame_count(R.RF, R.RF, R.DS) == 1 and FE.frame_count(R.RF + R.DS - 1, R.RF, R.DS) == 1
    assert FE.frame_count(R.RF + R.DS, R.RF, R.DS) == 2 and FE.frame_count(R.RF - 1, R.RF, R.DS) == 0


@pytest.mark.parametrize("kind,layers", [("gru", 1), ("gru", 2), ("lstm", 1)])
def test_chunked_reference_equals_whole_and_hand_off_matters(kind, layers):
    """On the CPU, in float64: the reference run chunk by chunk with the states handed on equals the whole run to 1e-12 (the window
    arithmetic: chunk k needs samples [k Tc ds, + (n - 1) ds + rf) and nothing else), and without the hand-off c at frames >= Tc is
    more than 1e-2 (relative l2) away -- so a device result within 1e-4 of the whole run has handed its states on."""
    model = R.model_for(kind, 32, layers)
    params = dict(model.state_dict())
    rec = R.recordings((37,), seed=11)[0].astype(np.float64) / 32768.0
    z, c = R.whole_reference(rec, params, kind, layers)
    assert z.shape == (37, R.E_S) and c.shape == (37, 32)
    for Tc in (1, 7, 16, 37, 64):
        zc, cc = R.chunked_reference(rec, params, kind, Tc, layers)
        assert R.rel_l2(zc, z) < 1e-12 and R.rel_l2(cc, c) < 1e-12, Tc
    for Tc in (7, 16):
        _, cn = R.chunked_reference(rec, params, kind, Tc, layers, hand_off=False)
        assert torch.equal(cn[:Tc], R.chunked_reference(rec, params, kind, Tc, layers)[1][:Tc])
        gap = R.rel_l2(cn[Tc:], c[Tc:])
        print(f"{kind} x{layers} Tc={Tc}: c without hand-off is {gap:.3f} away at frames >= Tc")
        assert gap > 1e-2


# ---------------------------------------------------------------------------------------------------------------- argument checks
P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
P4 = C.c_void_p(0x1004)         # 4-byte but not 8- / 16-byte aligned
P2 = C.c_void_p(0x1002)
S = C.c_void_p(0)
LL = C.c_longlong


def test_stream_gather_refuses_bad_arguments():
    lib = _hip.lib()

    def call(store=P, code=1, store_len=100, table=P, out=P, R_=2, L=10, ldo=10, scale=1.0, Tc=4, total=8, n_rec=2):
        return lib.cpc_stream_gather(store, code, LL(store_len), table, out, R_, L, LL(ldo), C.c_float(scale), Tc, LL(total), n_rec, S)

    bad = [dict(store=None), dict(table=None), dict(out=None), dict(R_=0), dict(R_=65536), dict(L=0), dict(L=(1 << 24) + 1), dict(ldo=9),
           dict(store_len=0), dict(Tc=0), dict(total=-1), dict(n_rec=0), dict(code=2), dict(code=-1), dict(scale=float("inf")),
           dict(scale=float("nan")), dict(store=C.c_void_p(0x1001)), dict(store=P2, code=0), dict(out=P2), dict(table=P4)]
    for kw in bad:
        assert call(**kw) == -22, kw


def test_feature_emit_refuses_bad_arguments():
    lib = _hip.lib()

    def call(table=P, top=P, top_item=4 * 16, hall=P, hall_item=5 * 16, src=_hip.F32, z=P, c=P, out=_hip.F32, R_=2, Tc=4, E=16, H=16,
             store_len=100, L=10, total=8, n_rec=2, partial=P, acc_z=P, acc_c=P):
        return lib.cpc_feature_emit(table, top, LL(top_item), hall, LL(hall_item), src, z, c, out, R_, Tc, E, H, LL(store_len), L,
                                    LL(total), n_rec, partial, acc_z, acc_c, S)

    bad = [dict(table=None), dict(z=None, c=None), dict(top=None), dict(hall=None), dict(src=2), dict(out=2), dict(src=-1), dict(R_=0),
           dict(R_=65536), dict(Tc=0), dict(Tc=(1 << 20) + 1), dict(E=0), dict(H=0), dict(E=18), dict(H=18), dict(E=-4), dict(H=-4),
           dict(E=65540), dict(src=_hip.BF16, E=20), dict(src=_hip.BF16, H=20), dict(top_item=4 * 16 - 4), dict(top_item=4 * 16 + 2),
           dict(hall_item=5 * 16 - 4), dict(hall_item=5 * 16 + 2), dict(L=0), dict(L=(1 << 24) + 1), dict(store_len=0), dict(total=-1),
           dict(n_rec=0), dict(top=P4), dict(hall=P4), dict(z=P4), dict(c=P4), dict(partial=P4), dict(acc_z=None), dict(acc_c=None),
           dict(acc_z=P2), dict(acc_c=P2), dict(table=P4)]
    for kw in bad:
        assert call(**kw) == -22, kw


def test_stream_carry_refuses_bad_arguments():
    lib = _hip.lib()
    arr = lambda *v: (C.c_void_p * len(v))(*v)
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000

    def call(table=P, src=arr(a, b), dst=arr(c, d), nstate=2, R_=2, H=16, store_len=100, L=10, Tc=4, total=8, n_rec=2):
        return lib.cpc_stream_carry(table, src, dst, nstate, R_, H, LL(store_len), L, Tc, LL(total), n_rec, S)

    nine = arr(*[0x10000 + 0x100 * i for i in range(9)])
    bad = [dict(table=None), dict(src=None), dict(dst=None), dict(nstate=0), dict(nstate=9, src=nine, dst=nine), dict(src=arr(a, 0)),
           dict(dst=arr(c, 0)), dict(src=arr(a, 0x2004)), dict(dst=arr(0x3008, d)), dict(dst=arr(a, d)), dict(dst=arr(c, a)),
           dict(R_=0), dict(R_=65536), dict(H=0), dict(H=18), dict(H=65540), dict(L=0), dict(store_len=0), dict(Tc=0), dict(total=-1),
           dict(n_rec=0), dict(table=P4)]
    for kw in bad:
        assert call(**kw) == -22, kw


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_from_the_constructor_without_a_device(golden_dir):
    from cpc_audio_amd.attention_model import AttentionModel
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel, ConvolutionalArModel
    enc = lambda: AudioEncoder(R.SMALL)
    conv = ConvolutionalArModel({'kernel_sizes': [3], 'channel_count': [R.E_S, 32], 'stride': [1], 'pooling': [1], 'batch_norm': False,
                                 'residual': False, 'bias': True})
    m_conv = AudioPredictiveCodingModel(enc(), conv, enc_size=R.E_S, ar_size=32, visible_steps=12, prediction_steps=4)
    attn = AttentionModel({'channels': R.E_S, 'num_layers': 1, 'num_heads': 2, 'feedforward_size': 64, 'sequence_length': 12,
                           'output_size': 32, 'dropout': 0.0, 'activation_register': None})
    m_attn = AudioPredictiveCodingModel(enc(), attn, enc_size=R.E_S, ar_size=32, visible_steps=12, prediction_steps=4)
    for m in (m_conv, m_attn):
        with pytest.raises(NotImplementedError, match="visible_steps"):
            FE.FeatureExtractor(m)
        with pytest.raises(NotImplementedError, match="visible_steps"):
            FE.FeatureExtractor(m, features=("c",))
        assert FE.FeatureExtractor(m, features=("z",)).kinds == ("z",)
    import copy
    import json
    import os
    from cpc_audio_amd.scalogram_model import ScalogramResidualEncoder
    blocks = copy.deepcopy(json.load(open(os.path.join(golden_dir, "scalogram_model.json")))["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    sc = ScalogramResidualEncoder(args_dict={'phase': True, 'blocks': blocks, 'activation_register': None})
    width = blocks[-1]['out_channels']
    m_sc = AudioPredictiveCodingModel(sc, AudioGRUModel(width, 32), enc_size=width, ar_size=32, visible_steps=12, prediction_steps=4)
    for feats in (("z", "c"), ("z",)):
        with pytest.raises(NotImplementedError, match="padded"):
            FE.FeatureExtractor(m_sc, features=feats)
    m = AudioPredictiveCodingModel(enc(), AudioGRUModel(R.E_S, 32, num_layers=4), enc_size=R.E_S, ar_size=32, visible_steps=12,
                                   prediction_steps=4)
    assert FE.FeatureExtractor(m).kinds == ("z", "c") and FE.FeatureExtractor(m, features=["c", "z"]).kinds == ("z", "c")
    for kw in (dict(features=()), dict(features=("y",)), dict(features=("z", "z")), dict(streams=0), dict(streams=65536),
               dict(streams=2.0), dict(chunk_frames=0), dict(chunk_frames=(1 << 20) + 1), dict(chunk_frames=True),
               dict(out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            FE.FeatureExtractor(m, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        FE.FeatureExtractor(m).extract([np.zeros(10, np.int16)])          # (the model is on the CPU: refused before any device work)
