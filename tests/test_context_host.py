"""The host contract of the context networks (contexts.ContextHost), on the CPU: the float32 host that stands between a bf16 engine and a
context computing in float32 (contexts.Float32Host) carries its own dtype, forwards exactly the contract's names from its engine, and
sizes split reductions for float32 through the helpers it inherits."""
import re
from types import SimpleNamespace

import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.contexts import Context, ContextHost, Float32Host


def _bare_host(dtype):
    """A ContextHost with nothing but its storage dtype: what _pick_split / _chunk of an engine of that dtype compute."""
    host = ContextHost.__new__(ContextHost)
    host.dt, host.code = dtype, _hip.dtype_code(dtype)
    return host


def _stub_engine():
    """An object with the attributes of a bf16 engine that matter here; nce_out and _pick_split stand for everything else it has."""
    return SimpleNamespace(dt=torch.bfloat16, code=_hip.dtype_code(torch.bfloat16), model="model", device=torch.device("cpu"),
                           B=4, E=64, H=32, K=3, V=10, T=13, geo=SimpleNamespace(alloc=[14]), colsum_blocks=1024, aux="aux", c="c",
                           slabs="slabs", use_aux=False, _gp_phase=3, gp_capable=True, _nbt_batch=None,
                           act=["bf16 top"], dact=["bf16 dtop"], nce_out="nce_out", pred="pred", ctx=None,
                           _pick_split=lambda *a: pytest.fail("the engine's helper ran"))


def test_float32_host_reads_the_contract_and_nothing_else():
    eng = _stub_engine()
    host = Float32Host(eng, "top32", "dtop32")
    assert host.dt == torch.float32 and host.code == _hip.dtype_code(torch.float32) != eng.code
    assert host.act == ["top32"] and host.dact == ["dtop32"]
    for name in Float32Host.ENGINE_NAMES:
        assert getattr(host, name) is getattr(eng, name), name
    # live reads: what the engine sets after the context was built, or between steps, is what the context sees
    eng.slabs, eng._gp_phase, eng.use_aux = "new slabs", 0, True
    assert host.slabs == "new slabs" and host._gp_phase == 0 and host.use_aux is True
    for name in ("nce_out", "pred", "ctx", "no_such_thing"):
        with pytest.raises(AttributeError):
            getattr(host, name)
    with pytest.raises(AttributeError):          # the forwarded names are read-only: a context never writes its host
        host.slabs = None


def test_float32_host_names_are_the_documented_contract():
    """Every forwarded name, and every name the host carries itself, is listed in ContextHost's docstring."""
    doc = ContextHost.__doc__
    for name in Float32Host.ENGINE_NAMES + ("dt", "code", "act", "dact"):
        if name == "_nbt_batch":          # count_batch()'s own state
            continue
        assert re.search(rf"(?<![\w.]){re.escape(name)}(?!\w)", doc), name
    for method in ("side", "_buf", "_pick_split", "_chunk", "_tn_to_grad", "_colsum_to_grad", "count_batch"):
        assert method + "()" in doc and callable(getattr(ContextHost, method))


def test_float32_host_sizes_split_reductions_for_float32():
    """The host over a bf16 engine answers _pick_split and _chunk as a float32 engine does, not as its bf16 engine does (row blocks of 32
    vs 64, 128- vs 256-wide tiles).  _pick_split(768, 256, 4096): 12 tiles of 128 -> min(512 // 12, 4096 / 256) = 16 in float32, 3 tiles of
    256 -> min(256 // 3, 4096 / 512) = 8 in bf16.  _chunk(1000, 4) cannot tell the two apart (250 rows round up to 256 under both block
    sizes), so it is only compared with float32's; _chunk(1000, 3) can: 334 rows round up to 352 vs 384."""
    host = Float32Host(_stub_engine(), "top32", "dtop32")
    f32, bf16 = _bare_host(torch.float32), _bare_host(torch.bfloat16)
    assert host._pick_split(768, 256, 4096) == f32._pick_split(768, 256, 4096) == 16
    assert bf16._pick_split(768, 256, 4096) == 8
    assert host._chunk(1000, 4) == f32._chunk(1000, 4) == 256
    assert host._chunk(1000, 3) == f32._chunk(1000, 3) == 352
    assert bf16._chunk(1000, 3) == 384


def test_engines_use_the_host_helpers_unchanged():
    from cpc_audio_amd.engine import CPCEngine
    from cpc_audio_amd.contexts import ContextOnlyEngine
    from cpc_audio_amd.scalogram_engine import ScalogramCPCEngine
    for cls in (CPCEngine, ScalogramCPCEngine, ContextOnlyEngine, Float32Host):
        assert issubclass(cls, ContextHost)
        for method in ("side", "_buf", "_pick_split", "_chunk", "_tn_to_grad", "_colsum_to_grad", "count_batch"):
            assert getattr(cls, method) is getattr(ContextHost, method), (cls.__name__, method)
    assert not issubclass(ContextOnlyEngine, CPCEngine)


def test_context_protocol_defaults():
    from cpc_audio_amd.contexts import AttentionContext, ConvArContext, Float32Context, GRUContext
    from cpc_audio_amd.scalogram_engine import ConvArGridContext, GridContext, ResNetArContext
    assert Context.ahead_ok is False and Context.z_scale == 1.0
    for cls in (GRUContext, ConvArContext, AttentionContext, Float32Context, GridContext, ConvArGridContext, ResNetArContext):
        assert issubclass(cls, Context), cls.__name__
    bare = Context()
    with pytest.raises(NotImplementedError):
        bare.tangent(None)
    with pytest.raises(NotImplementedError):
        bare.gp_grads({})
