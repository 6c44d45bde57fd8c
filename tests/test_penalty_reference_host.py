"""The references, emulations, measures and bounds of test_penalty_kernels_gpu.py (tests/penalty_reference.py) judged on the host:
  * the references against each other: the GRU probe construction against autograd's double backward of the plain GRU and, with
    W_hh = 0, against a closed form per unit; the closed formulas of the attention and LayerNorm kernels against jvp + grad on the
    definitions (this file is now the judge of that algebra at kernel level; tools/gp_attention_algebra.py checks the whole context
    network once, by hand); a dropout mask read at a wrong index changes the result;
  * every float32 emulation stays below its cap (a quarter of 10 x the older tests' tolerance, so that no bound exceeds 10 x), figures
    printed per case;
  * the mutation table: each deliberate mistake, applied to the emulation, is rejected by the new measures on every case that can
    express it; whether the older measures (whole-tensor maxima at 1e-4 / 1e-5 / 1e-6, L2 of the assembled GRU gradients at 2e-4)
    reject it as well is recorded and printed;
  * the case table covers every route; the launchers' argument checks return -22 before any launch (the library loads on a CPU host;
    the pointers are never dereferenced).

What the older GRU measure cannot see (measured here with the reference, test_gru_old_measure_is_blind_to_the_early_steps): with a
whole block of dA replaced by zeros at one step (an error of 100 % there), the L2 of every assembled gradient stays below 2e-4 for
41 % of the (block, step) pairs of the decay case (2, 40, 64) and for 2 % at (3, 13, 48).  Old-measure record of the mutation table
(printed in full by the three table tests): a non-zero initial tangent state h~_{-1} passes the older measures on 8 of the 15 GRU
cases (every one with V >= 13) and is rejected by the new ones on all 15 (the tangent slot at t = 0 must be exactly 0); every other
listed mutation is also rejected by the older whole-tensor measures when they are applied against these references (the older
tests' own weakness there was their judge, a restated formula, not their tolerance).
No device is touched.
"""
import ctypes as C

import pytest
import torch

import context_reference as R
import penalty_reference as G
from cpc_audio_amd import _hip

GRU_CASES, ATTN_CASES, LN_CASES = G.gru_gp_cases(), G.attn_gp_cases(), G.ln_gp_cases()


# ====================================================================================================================== GRU
@pytest.mark.parametrize("B,V,H", [(2, 1, 16), (3, 13, 48), (2, 40, 64), (2, 100, 96), (2, 3, 512)])
def test_gru_probe_reference_against_double_backward(B, V, H):
    """On unrounded projections the gradients assembled from the probe reference as GRUContext.gp_grads assembles them equal
    autograd's double backward of the plain GRU, per row of every gradient, to 1e-9 (they agree to about 1e-13); the kernels' formulas
    evaluated in float64 agree with the probe reference per step to 1e-11."""
    d = G.gru_gp_data(B, V, H)
    Gi, GiT = d["Gi64"].reshape(B, V, 3 * H), d["GiT64"].reshape(B, V, 3 * H)
    tape, ct, dA = G.gru_gp_probe_reference(Gi, GiT, d["Whh"], d["bhh"], d["wc"])
    ref = dict(tape=tape, ct=ct, dA=dA, grads=G.gru_gp_double_backward(d))
    et, ec, ea = G.gru_gp_emulate(Gi, GiT, d["Whh"], d["bhh"], d["wc"], dtype=torch.float64, seq=False)
    errs = G.gru_gp_errors(et, ec, ea, G.gru_gp_assemble(tape, dA, d["x"], d["xt"], d["Wih"]), ref)
    worst = {k: float(v.max()) for k, v in errs.items()}
    print(f"B={B} V={V} H={H}: assembled vs double backward {max(worst[k] for k in G.GRU_GRADS):.1e}, "
          f"kernel formulas in float64 vs probes {max(v for k, v in worst.items() if k not in G.GRU_GRADS):.1e}")
    assert all(worst[k] < 1e-9 for k in G.GRU_GRADS), worst
    assert all(v < 1e-11 for k, v in worst.items() if k not in G.GRU_GRADS), worst


@pytest.mark.parametrize("B,V,H", [(1, 2, 16), (3, 13, 48), (2, 40, 64)])
def test_gru_probe_reference_against_the_closed_form_without_recurrent_weights(B, V, H):
    """W_hh = 0: dA and ct of the probe reference equal the closed form per unit (cumulative products, grad and grad again)."""
    ref = G.gru_gp_reference(B, V, H, "whh0")
    dA, ct = G.gru_gp_whh0_closed(ref["d"])
    for k in range(8):
        assert float(G.block_err(ref["dA"][:, :, k], dA[:, :, k], (0, 2)).max()) < 1e-10, k
    assert float(G.block_err(ref["ct"], ct, (1,)).max()) < 1e-10
    assert bool((ref["tape"][:, :, 7] == 0).all()) and bool((ref["bounds"]["tape7"] == 0).all())      # W_hn h~ = 0 at every step


def test_gru_zero_reference_blocks_demand_exact_zeros():
    """h_{-1}, its tangent and W_hn h~_{-1} are exactly 0 at t = 0: bound 0 there, and anything but 0 is a violation."""
    ref = G.gru_gp_reference(3, 13, 48)
    for k in (4, 7, 9):
        assert float(ref["bounds"][f"tape{k}"][0]) == 0.0 and bool((ref["bounds"][f"tape{k}"][1:] > 0).all())
    tape = ref["tape"].clone()
    tape[0, 0, 9, 3] = 1e-30
    errs = G.gru_gp_errors(tape, ref["ct"], ref["dA"], ref["grads"], ref)
    assert [v[:2] for v in G.violations(errs, ref["bounds"])] == [("tape9", 0)]
    tape[0, 0, 9, 3] = -0.0
    assert not G.violations(G.gru_gp_errors(tape, ref["ct"], ref["dA"], ref["grads"], ref), ref["bounds"])


@pytest.mark.parametrize("case", GRU_CASES, ids=G.gru_gp_case_id)
def test_gru_emulation_stays_below_its_cap(case):
    """The float32 emulation (sequential fma chains) against float64, per step and block; prints the figures of the GPU file's
    docstring."""
    _, B, V, H, rec = case
    ref = G.gru_gp_reference(B, V, H, rec, G.gru_gp_case_seed(case))
    e = ref["e_emul"]
    tape = G.emul_max(e, [f"tape{k}" for k in range(10)])
    dA = G.emul_max(e, [f"dA{k}" for k in range(8)])
    ct, grads = G.emul_max(e, ["ct"]), G.emul_max(e, G.GRU_GRADS)
    print(f"GRU {G.gru_gp_case_id(case)}: tape {tape:.1e} dA {dA:.1e} ct {ct:.1e} grads {grads:.1e}")
    assert max(tape, dA, grads) < G.CAP["gru"] and ct < G.CAP["gru_ct"]
    assert not G.violations(e, ref["bounds"])
    assert max(float(b.max()) for b in ref["bounds"].values()) <= 10 * 2e-4


def test_gru_mutation_table():
    rows = []
    for mut in G.GRU_MUTATIONS:
        for case in GRU_CASES:
            if not G.gru_mutation_expressible(mut, case):
                continue
            _, B, V, H, rec = case
            ref = G.gru_gp_reference(B, V, H, rec, G.gru_gp_case_seed(case))
            d = ref["d"]
            tape, ct, dA = G.gru_gp_emulate(d["Gi"], d["GiT"], d["Whh"], d["bhh"], d["wc"], seq=False, mut=mut)
            errs = G.gru_gp_errors(tape, ct, dA, G.gru_gp_assemble(tape, dA, d["x"], d["xt"], d["Wih"]), ref)
            new = bool(G.violations(errs, ref["bounds"]))
            rows.append((mut, G.gru_gp_case_id(case), new, G.gru_old_measures_reject(tape, ct, dA, ref)))
    _print_table("GRU", rows)
    assert all(r[2] for r in rows), [r for r in rows if not r[2]]
    # the older measure lets the first-step mistake through on the decay case: nothing it looks at reaches step 0
    assert ("ht_init", "B2-V40-H64-plain", True, False) in rows


def _print_table(family, rows):
    print(f"{family}: mutation / case / rejected by the new measures / by the older measures")
    for r in rows:
        print(f"  {r[0]:18s} {r[1]:34s} {'yes' if r[2] else 'NO':4s} {'yes' if r[3] else 'no'}")
    missed = sorted({r[0] for r in rows if not r[3]})
    print(f"  the older measures miss, on at least one case: {missed}")


def test_gru_old_measure_is_blind_to_the_early_steps():
    decay, short = G.gru_old_measures_blind_share(G.gru_gp_reference(2, 40, 64)), G.gru_old_measures_blind_share(G.gru_gp_reference(3, 13, 48))
    print(f"share of (dA block, step) pairs a 100 % error in which the older L2 measure accepts: (2,40,64) {decay:.2f}, (3,13,48) {short:.2f}")
    assert decay > 0.3


# ====================================================================================================================== attention
@pytest.mark.parametrize("case", ATTN_CASES, ids=G.attn_gp_case_id)
def test_attention_closed_formulas_against_jvp_and_the_emulation_cap(case):
    """attn_gp_closed in float64 on an unrounded softmax equals jvp + grad on the definition to 1e-11 per position and block (the q
    third at t = 0 exactly 0 in both); the float32 emulation stays below its cap; figures printed."""
    ref = G.attn_gp_case_reference(case)
    d = ref["d"]
    exact = dict(d, P=G.attn_softmax(d["qkv"], d["B"], d["S"], d["C"], d["heads"]))
    errs = G.attn_gp_errors(*G.attn_gp_closed(exact), ref)
    assert max(float(v.max()) for v in errs.values()) < 1e-11, errs
    assert bool(ref["zero"]["dq"][0]) and float(ref["bounds"]["dq"][0]) == 0.0
    e = ref["e_emul"]
    o, inc = float(e["out_t"].max()), max(float(e[k].max()) for k in ("dq", "dk", "dv"))
    print(f"attention {G.attn_gp_case_id(case)}: out_t {o:.1e} inc {inc:.1e}")
    assert o < G.CAP["attn_out_t"] and inc < G.CAP["attn_inc"]


def test_attention_reference_reads_the_mask_at_its_index():
    """A dropout mask whose index is off by one (bh S S + i S + j + 1) changes out_t and the increment grossly."""
    case = ("short", 3, 10, 64, 8, 0.3, 1.0)
    ref = G.attn_gp_case_reference(case)
    shifted = lambda n, p, seed, site: R.dropout_mask_host(n + 1, p, seed, site)[1:]
    d = G.attn_gp_data(*case[1:6], mask_fn=shifted)
    assert bool((d["m"] != ref["d"]["m"]).any())
    assert G.violations(G.attn_gp_errors(*G.attn_gp_reference(d), ref), ref["bounds"])


def test_attention_mutation_table():
    rows = []
    for mut in G.ATTN_MUTATIONS:
        for case in ATTN_CASES:
            if not G.attn_mutation_expressible(mut, case):
                continue
            ref = G.attn_gp_case_reference(case)
            out_t, inc = G.attn_gp_closed(ref["d"], torch.float32, mut)
            new = bool(G.violations(G.attn_gp_errors(out_t, inc, ref), ref["bounds"]))
            rows.append((mut, G.attn_gp_case_id(case), new, G.attn_old_measures_reject(out_t, inc, ref)))
    _print_table("attention", rows)
    assert all(r[2] for r in rows), [r for r in rows if not r[2]]
    assert {r[0] for r in rows} == set(G.ATTN_MUTATIONS)


# ====================================================================================================================== LayerNorm
@pytest.mark.parametrize("case", LN_CASES + [G.LN_WIDE_CASE], ids=G.ln_gp_case_id)
def test_layernorm_closed_formulas_against_jvp_and_the_emulation_cap(case):
    """ln_gp_closed in float64 with exact statistics equals jvp + grad on the definition; with the float32 statistics the kernels
    read it is the emulation, which stays below its cap in all three summation orders; figures printed."""
    ref = G.ln_gp_case_reference(case)
    d = ref["d"]
    r = d["r"]
    exact = dict(d, stats=torch.stack([r.mean(1), 1.0 / torch.sqrt(r.var(1, unbiased=False) + R.LN_EPS)], 1))
    errs = G.ln_gp_errors(G.ln_gp_closed(exact), ref)
    tol = 1e-7 if case[5] == "large_mean" else 1e-10          # (x - mean at mean 1000 loses 1e-13 relative in float64, squared terms more)
    assert max(float(v.max()) for v in errs.values()) < tol, {k: float(v.max()) for k, v in errs.items()}
    e = {k: float(v.max()) for k, v in ref["e_emul"].items()}
    print(f"LayerNorm {G.ln_gp_case_id(case)}: rt {e['rt']:.1e} yt {e['yt']:.1e} inc {e['inc']:.1e} inc_b {e['inc_b']:.1e} gw {e['gw']:.1e}")
    assert e["rt"] < G.CAP["ln_rt"] and e["yt"] < G.CAP["ln_yt"] and max(e["inc"], e["inc_b"], e["gw"]) < G.CAP["ln_inc"]


def test_layernorm_reference_reads_the_mask_at_its_index():
    case = (37, 96, 0.3, "layer", 0, "plain")
    ref = G.ln_gp_case_reference(case)
    d = G.ln_gp_data(*case, mask_fn=lambda n, p, seed, site: R.dropout_mask_host(n + 1, p, seed, site)[1:])
    got = G.ln_gp_reference(d)
    assert G.violations(G.ln_gp_errors(got, ref), ref["bounds"])


def test_layernorm_mutation_table():
    rows = []
    for mut in G.LN_MUTATIONS:
        for case in LN_CASES:
            if not G.ln_mutation_expressible(mut, case):
                continue
            ref = G.ln_gp_case_reference(case)
            got = G.ln_gp_emulate(ref["d"], "pairwise", mut)
            new = bool(G.violations(G.ln_gp_errors(got, ref), ref["bounds"]))
            rows.append((mut, G.ln_gp_case_id(case), new, G.ln_old_measures_reject(got, ref)))
    _print_table("LayerNorm", rows)
    assert all(r[2] for r in rows), [r for r in rows if not r[2]]
    assert {r[0] for r in rows} == set(G.LN_MUTATIONS)


# ====================================================================================================================== case table
def test_case_table_covers_every_route():
    gru = {(B, V, H) for _, B, V, H, _ in GRU_CASES}
    assert {(1, 1, 16), (1, 2, 16), (3, 13, 48), (2, 13, 64), (2, 5, 80), (2, 3, 512), (2, 3, 384), (2, 40, 64)} <= gru
    assert any(H % 64 and H > 64 for _, _, H in gru) and any(H < 64 for _, _, H in gru) and any(H == 512 for _, _, H in gru)
    assert {rec for *_, rec in GRU_CASES} == set(G.GRU_RECIPES)
    assert all((B, V, H, "plain") in {c[1:] for c in GRU_CASES} for B, V, H in gru)
    ln = LN_CASES
    assert {(M, C) for M, C, *_ in ln} >= set(G.LN_SHAPES) and {c[2] for c in ln} == {0.0, 0.3}
    for M, C in G.LN_SHAPES:
        assert {c[3] for c in ln if c[:2] == (M, C)} == {"layer", "layer_no_g2", "final"}          # NULL operands as the engine passes them
        assert {c[2] for c in ln if c[:2] == (M, C) and c[3] != "final"} == {0.0, 0.3}
    assert any(M > 8192 for M, *_ in ln)                                              # ln_tangent's grid stride
    assert any(M % 4 for M, *_ in ln) and any(C < 64 for _, C, *_ in ln) and any(C % 64 and C > 64 for _, C, *_ in ln)
    assert all(G.ln_nblocks(M)[0] == 1 and G.ln_nblocks(M)[2] > (M + 3) // 4 for M, *_ in ln)      # one block; zero slabs
    assert {(c[0], c[4]) for c in ln if c[4]} == {(120, 60)} and {c[3] for c in ln if c[4]} == {"final", "layer"}
    assert {c[1] for c in ln if c[5] == "large_mean"} == {64, 1024}
    at = ATTN_CASES
    assert {c[1:5] for c in at if c[0] == "short"} >= set(G.ATTN_SHORT)
    assert {(c[2], c[3], c[4]) for c in at if c[0] == "long"} >= {(S, Cc, h) for S in G.ATTN_LONG_S for Cc, h in G.ATTN_LONG_SHAPES}
    assert {c[2] for c in at if c[0] == "long" and c[5] > 0} == set(G.ATTN_LONG_S)                # every S with dropout
    assert {c[2] for c in at if c[0] == "long" and c[2] <= 64} == {1, 37, 64}                      # both families at S <= 64
    assert {c[0] for c in at if c[6] == G.ATTN_PEAKED} == {"short", "long"}


def test_within_one_ulp():
    lam, inc = torch.tensor([1.0, 3.0]), torch.tensor([2.0 ** -24, 1e-3])
    want = (lam.double() + inc.double()).float()
    assert G.within_one_ulp(want, lam, inc) and G.within_one_ulp(torch.nextafter(want, torch.tensor(9.0)), lam, inc)
    assert not G.within_one_ulp(want + 2 * 2.0 ** -22, lam, inc) and not G.within_one_ulp(torch.tensor([float("nan"), 3.001]), lam, inc)


# ====================================================================================================================== argument checks
def test_penalty_arguments_are_checked_before_any_launch():
    """Every refusal include/cpc_hip.h states for the eight entry points returns CPC_EINVAL (-22): a NULL required pointer in every
    position (bt, rt_out, g2 and dr_b stay optional: with them NULL the size check still refuses), B, V, H, S, M, C, nblocks and the
    head size outside their ranges, drop_p outside [0, 1)."""
    lib = _hip.lib()
    P, N, s = C.c_void_p(0x1000), None, C.c_void_p(0)
    F, U64, U32 = C.c_float, C.c_ulonglong, C.c_uint

    def holes(n, optional=()):
        for i in range(n):
            if i not in optional:
                yield [N if j == i else P for j in range(n)]

    for ptrs in holes(6):
        assert lib.cpc_gru_gp_fwd(*ptrs, 2, 4, 64, s) == -22
    for ptrs in holes(4):
        assert lib.cpc_gru_gp_bwd(*ptrs, 2, 4, 64, s) == -22
    for B, V, H in ((0, 4, 64), (-1, 4, 64), (2, 0, 64), (2, -2, 64), (2, 4, 0), (2, 4, -16), (2, 4, 513), (2, 4, 1024)):
        assert lib.cpc_gru_gp_fwd(P, P, P, P, P, P, B, V, H, s) == -22, (B, V, H)
        assert lib.cpc_gru_gp_bwd(P, P, P, P, B, V, H, s) == -22, (B, V, H)
    tail = (F(0.0), U64(0), U32(0), s)
    for name, S_max in (("cpc_attn", 64), ("cpc_attn128", 128)):
        tan, gp = getattr(lib, name + "_tangent"), getattr(lib, name + "_gp")
        for ptrs in holes(4):
            assert tan(*ptrs, 2, 8, 64, 2, *tail) == -22
        for ptrs in holes(5):
            assert gp(*ptrs, 2, 8, 64, 2, *tail) == -22
        shapes = [(0, 8, 64, 2), (2, 0, 64, 2), (2, S_max + 1, 64, 2), (2, 129, 64, 2), (2, 8, 64, 0), (2, 8, 64, 3), (2, 8, 12, 2),
                  (2, 8, 130, 1), (2, 8, 68, 1), (2, 8, 2, 1)]          # head sizes 6, 130, 68 and 2: no multiple of 4 or above 64
        for B, S, Cc, h in shapes:
            assert tan(P, P, P, P, B, S, Cc, h, *tail) == -22, (name, B, S, Cc, h)
            assert gp(P, P, P, P, P, B, S, Cc, h, *tail) == -22, (name, B, S, Cc, h)
        for p in (-0.1, 1.0, 1.5):
            assert tan(P, P, P, P, 2, 8, 64, 2, F(p), U64(0), U32(0), s) == -22, p
            assert gp(P, P, P, P, P, 2, 8, 64, 2, F(p), U64(0), U32(0), s) == -22, p
    for ptrs in holes(7, optional=(1, 5)):          # at, bt, r, stats, w, rt_out, yt
        assert lib.cpc_ln_tangent(*ptrs, 8, 64, *tail) == -22
    for ptrs in holes(9, optional=(1, 7)):          # g1, g2, rt, r, stats, w, dr, dr_b, slabs
        assert lib.cpc_ln_gp(*ptrs, 8, 64, 0, F(1.0), 2, *tail) == -22
    for M, Cc in ((0, 64), (-4, 64), (8, 0), (8, -64)):
        assert lib.cpc_ln_tangent(P, N, P, P, P, N, P, M, Cc, *tail) == -22, (M, Cc)
        assert lib.cpc_ln_gp(P, N, P, P, P, P, P, N, P, M, Cc, 0, F(1.0), 2, *tail) == -22, (M, Cc)
    assert lib.cpc_ln_gp(P, N, P, P, P, P, P, N, P, 8, 1028, 0, F(1.0), 2, *tail) == -22          # C > 1024 (cpc_ln_tangent accepts it)
    assert lib.cpc_ln_gp(P, N, P, P, P, P, P, N, P, 8, 2048, 0, F(1.0), 2, *tail) == -22
    for nb in (0, -1):
        assert lib.cpc_ln_gp(P, N, P, P, P, P, P, N, P, 8, 64, 0, F(1.0), nb, *tail) == -22
    for p in (-0.1, 1.0, 1.5):
        assert lib.cpc_ln_tangent(P, P, P, P, P, P, P, 8, 64, F(p), U64(0), U32(0), s) == -22, p
        assert lib.cpc_ln_gp(P, P, P, P, P, P, P, P, P, 8, 64, 0, F(1.0), 2, F(p), U64(0), U32(0), s) == -22, p
