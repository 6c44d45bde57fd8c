"""Float64 references for prediction anchors ("Prediction anchors"), shared by test_anchors_host.py and test_anchors_gpu.py.
Nothing here touches a device.

  * the whole model with A anchors s steps apart, composed from the oracle's encoder, GRU cell, score functions and info_nce_loss and
    from lstm_reference / gru_stacked_reference for the cells; gradients by torch autograd (AnchorOracle);
  * the LSTM backward sweep with a gradient injected at every hidden state, float64 and with the kernels' bf16 roundings, in the manner
    of lstm_reference.lstm_run (lstm_run_steps, lstm_steps_reference);
  * cpc_anchor_target_grad restated in numpy (anchor_target_grad).

Anchor a = 0 .. A-1 has the shift d_a = (A - 1 - a) s: its context is h_{V - d_a} of the one recurrence that starts at frame T - K - V,
its targets are frames [T - K - d_a, T - d_a); head a K + k is step k of anchor a.
"""
import numpy as np
import torch

from oracle import cpc_oracle as O
import gru_stacked_reference as G
import lstm_reference as L
from context_reference import BF16, F32, ident, rounded, to_bf16  # noqa: F401

LSTM_PREFIX = "autoregressive_model.lstmCell."


def shifts(A, s):
    return [(A - 1 - a) * s for a in range(A)]


def context_after(z, params, context):
    """h after all the frames of z (B, E, n): context = ("gru", num_layers) or ("lstm",)."""
    if context[0] == "gru":
        return G.stacked_gru_forward(z, params, context[1])
    return L.lstm_model_reference(z, params, LSTM_PREFIX)[0]


def stacked_heads(enc, params, V, K, A, s, context):
    """enc (B, E, T) -> predicted_z (B, A K, E), targets (B, E, A K), z (B, E, V), c = h_V (B, H).  A recurrence over the first n
    frames of z IS the first n steps of the recurrence over all of z, so c_a is computed as the context of z[:, :, :V - d_a]."""
    T, E = enc.shape[2], enc.shape[1]
    z = enc[:, :, T - K - V:T - K]
    w_p = params["prediction_model.weight"]
    preds, targs, c = [], [], None
    for d in shifts(A, s):
        c = context_after(z[:, :, :V - d], params, context)
        preds.append((c @ w_p.t()).view(-1, K, E))
        targs.append(enc[:, :, T - K - d:T - d])
    return torch.cat(preds, 1), torch.cat(targs, 2), z, c


def _is_buffer(k):
    return ("running_" in k) or k.endswith("num_batches_tracked")


class AnchorOracle:
    """The reference train step in float64 with A anchors: the oracle's encoder, stacked_heads, the oracle's score functions,
    info_nce_loss on the A K heads (score_over_all_timesteps=False), adam_update; differentiated by torch autograd."""

    def __init__(self, params, V, K, A, s, context, score="softplus", regularization=1.0, lr=1e-4, strides=None):
        self.params = {k: v.detach().clone().double().requires_grad_(True) for k, v in params.items() if not _is_buffer(k)}
        self.m = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.V, self.K, self.A, self.s, self.context = V, K, A, s, context
        self.score, self.regularization, self.lr = O.SCORE_FUNCTIONS[score], regularization, lr
        self.strides = strides
        self.t = 0

    def encode(self, batch):
        x = batch.double().unsqueeze(1)
        return O.encoder_forward(x, self.params) if self.strides is None else O.encoder_forward(x, self.params, self.strides)

    def forward(self, batch, A=None, s=None):
        return stacked_heads(self.encode(batch), self.params, self.V, self.K, self.A if A is None else A, self.s if s is None else s,
                             self.context)

    def loss(self, batch):
        pred, targ, _, _ = self.forward(batch)
        return O.info_nce_loss(self.score(pred, targ), False, self.regularization)

    def loss_and_grads(self, batch):
        for p in self.params.values():
            p.grad = None
        loss, smax = self.loss(batch)
        loss.backward()
        return loss.detach(), smax.detach(), {k: p.grad for k, p in self.params.items()}

    def functional_grads(self, batch, w_pred, w_targ):
        """Gradients of sum(w_pred * predicted_z) + sum(w_targ * targets)."""
        for p in self.params.values():
            p.grad = None
        pred, targ, _, _ = self.forward(batch)
        ((pred * w_pred.double()).sum() + (targ * w_targ.double()).sum()).backward()
        return pred.detach(), targ.detach(), {k: p.grad for k, p in self.params.items()}

    def step(self, batch):
        loss, smax, grads = self.loss_and_grads(batch)
        self.t += 1
        with torch.no_grad():
            for k, p in self.params.items():
                O.adam_update(p, grads[k], self.m[k], self.v[k], self.t, self.lr)
        return float(loss), float(smax)

    def validation(self, batch):
        """What validate() measures: the last anchor's K heads (today's model)."""
        with torch.no_grad():
            pred, targ, _, _ = self.forward(batch, A=1, s=1)
            return O.validation_terms(self.score(pred, targ), False)


# ---------------------------------------------------------------------------------------------------- LSTM sweep with injected gradients
def lstm_run_steps(Gi, w, b, dh_last, dHs, h0=None, c0=None, rnd=ident):
    """lstm_reference.lstm_run with a gradient at every hidden state: dHs (B, V, H) (as the device stores it) reaches h_{t+1} from
    outside the recurrence, step t starts from d = dh + dHs[:, t]; dh_last (B, H) or None (zeros).  Roundings as lstm_run's; the sum
    d is f32 on the device (here: unrounded).  Returns Hall, h_V, cell_V, dG."""
    B, V, H4 = Gi.shape
    H = H4 // 4
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    cell = torch.zeros(B, H, dtype=torch.float64) if c0 is None else c0
    hall, tape = [rnd(h)], []
    for t in range(V):
        a = Gi[:, t] + rnd(h) @ w.T + b
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        g = torch.tanh(a[:, 2 * H:3 * H])
        cp = cell
        cell = f * cp + i * g
        tc = torch.tanh(cell)
        h = o * tc
        tape.append((rnd(i), rnd(f), rnd(g), rnd(o), rnd(cp), rnd(tc)))
        hall.append(rnd(h))
    dh = torch.zeros(B, H, dtype=torch.float64) if dh_last is None else dh_last
    dcell = torch.zeros(B, H, dtype=torch.float64)
    dG = torch.zeros(B, V, 4 * H, dtype=torch.float64)
    for t in range(V - 1, -1, -1):
        i, f, g, o, cp, tc = tape[t]
        d = dh if dHs is None else dh + dHs[:, t]
        do_pre = d * tc * o * (1 - o)
        dct = dcell + d * o * (1 - tc * tc)
        di_pre = dct * g * i * (1 - i)
        df_pre = dct * cp * f * (1 - f)
        dg_pre = dct * i * (1 - g * g)
        dG[:, t] = torch.cat([rnd(di_pre), rnd(df_pre), rnd(dg_pre), rnd(do_pre)], 1)
        dcell = dct * f
        dh = dG[:, t] @ w
    return torch.stack(hall, 1), h, cell, dG


def lstm_steps_autograd(Gi, w, b, dh_last, dHs):
    """The same through float64 autograd (no rounding): d sum_t <dHs[:, t], h_{t+1}> + <dh_last, h_V> / d Gi."""
    B, V, H4 = Gi.shape
    H = H4 // 4
    x = Gi.clone().requires_grad_(True)
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    total = 0.0
    for t in range(V):
        a = x[:, t] + h @ w.T + b
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        c = f * c + i * torch.tanh(a[:, 2 * H:3 * H])
        h = o * torch.tanh(c)
        if dHs is not None:
            total = total + (h * dHs[:, t]).sum()
    if dh_last is not None:
        total = total + (h * dh_last).sum()
    total.backward()
    return x.grad


_STEPS = {}


def lstm_steps_reference(dt, B, V, H, mode, with_dh):
    """lstm_reference.lstm_reference's data (same seed) plus dHs ~ N(0, 1) stored in dt: mode "dense", or "one" (non-zero at step
    V // 2 only).  with_dh False: no gradient at the last state.  Returns the inputs, the float64 dG and the per-step bounds of
    test_lstm_fwd_bwd_per_step: f32 5e-5 on the gate blocks, bf16 4 x the per-step error of the bf16 emulation.  Computed once per
    argument set; callers do not modify it."""
    key = (dt, B, V, H, mode, with_dh)
    if key in _STEPS:
        return _STEPS[key]
    w_hh, b_hh, Gi, dh, _, _ = L.lstm_data(B, V, H)
    g = torch.Generator().manual_seed(77 + B * 1000 + H + V)
    dHs = torch.randn(B, V, H, generator=g)
    if mode == "one":
        keep = torch.zeros(V)
        keep[V // 2] = 1.0
        dHs = dHs * keep.view(1, V, 1)
    wr, br, gir, dhr, dhsr = rounded(w_hh, dt), b_hh.double(), rounded(Gi, dt), dh.double() if with_dh else None, rounded(dHs, dt)
    hall, _, _, dG = lstm_run_steps(gir, wr, br, dhr, dhsr)
    names = L.LSTM_BLOCKS[1:]
    if dt == F32:
        tol = {k: torch.full((V,), L.LSTM_TOL_F32[k], dtype=torch.float64) for k in names}
    else:
        em = lstm_run_steps(gir, wr, br, dhr, dhsr, rnd=to_bf16)
        e_model = L.lstm_step_errors(em[0], em[3], hall, dG)
        tol = {k: L.LSTM_MODEL_FACTOR * e_model[k] for k in names}
    ref = dict(w_hh=w_hh, b_hh=b_hh, gir=gir, dh=dh if with_dh else None, dHs=dhsr, wr=wr, br=br, dhr=dhr, hall=hall, dG=dG, tol=tol)
    _STEPS[key] = ref
    return ref


def gate_violations(dG, ref):
    """[(block, step, error, bound)] of the four gate blocks of dG (B, V, 4H) against the reference's per-step bounds."""
    errs = L.lstm_step_errors(ref["hall"], dG, ref["hall"], ref["dG"])
    bad = []
    for k in L.LSTM_BLOCKS[1:]:
        for t, (e, b) in enumerate(zip(errs[k].tolist(), ref["tol"][k].tolist())):
            if not e <= b:
                bad.append((k, t, e, b))
    return bad, {k: float(errs[k].max()) for k in L.LSTM_BLOCKS[1:]}


# ---------------------------------------------------------------------------------------------------- cpc_anchor_target_grad
def anchor_target_grad(dT, dtop, first_row, stride, row_lo, row_hi, accumulate):
    """dT (A, B, K, E) float, dtop (B, rows, E) float: returns a copy of dtop with rows [row_lo, row_hi) of every item set to (or, with
    accumulate, increased by) the sum over the anchors a, ascending, whose window [first_row + a stride, first_row + a stride + K)
    covers the row.  Uncovered rows: zeros, or untouched with accumulate.  Everything else unchanged.  No rounding here: the callers
    use data whose sums are exact in the storage type."""
    dT, out = np.asarray(dT, dtype=np.float64), np.array(dtop, dtype=np.float64, copy=True)
    A, B, K, E = dT.shape
    for r in range(row_lo, row_hi):
        acc, covered = np.zeros((B, E)), False
        for a in range(A):
            k = r - first_row - a * stride
            if 0 <= k < K:
                acc, covered = acc + dT[a, :, k, :], True
        if accumulate:
            if covered:
                out[:, r, :] = acc + out[:, r, :]
        else:
            out[:, r, :] = acc
    return out
