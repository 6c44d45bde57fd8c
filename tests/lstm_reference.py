"""Plain float64 reference of the LSTM recurrence kernels (csrc/lstm.hip) and a float64 emulation of where they round to their storage
type.  Shared by test_lstm_gpu.py (the kernels against this reference) and test_lstm_host.py (this reference against torch's own
nn.LSTMCell, the cap on the emulation's error and the sensitivity of the per-step verdict to deliberate mistakes).  Nothing here touches
a device.  The method is context_reference.py's for the GRU; its measures, caps and factors are imported from there.
"""
import math

import torch

from context_reference import (BF16, F32, GRU_MODEL_CAP, GRU_MODEL_FACTOR, GRU_TOL_F32, ident, per_step_err, rounded,  # noqa: F401
                               rel_err, to_bf16)

LSTM_BLOCKS = ("Hall", "di", "df", "dg", "do")
LSTM_TOL_F32 = {"Hall": GRU_TOL_F32["Hall"], "di": GRU_TOL_F32["dr"], "df": GRU_TOL_F32["dr"], "dg": GRU_TOL_F32["dr"],
                "do": GRU_TOL_F32["dr"]}          # 2e-5 for the hidden states, 5e-5 for the gate blocks
LSTM_MODEL_CAP = GRU_MODEL_CAP            # the bf16 emulation alone stays below this at every step of every case
LSTM_MODEL_FACTOR = GRU_MODEL_FACTOR      # device <= 4 e_model(t): the f32 summation order of the MFMAs and the device's exp / rcp


# (family, storage type, H, B, V) of every kernel case of test_lstm_gpu.py
def lstm_cases():
    cases = []
    for H in (32, 96, 160, 256):          # 4-wave kernels, bf16: waves with unequal or no tiles, a partial batch tile
        for B in (1, 17):
            for V in (1, 2, 13):
                cases.append(("streaming", BF16, H, B, V))
    for H in (16, 48, 256):               # 4-wave kernels, f32 (H = 256: the 65 792-byte backward tile)
        for B in (1, 17):
            for V in (1, 13):
                cases.append(("streaming", F32, H, B, V))
    for H in (288, 512):                  # 8-wave kernels
        for dt in (F32, BF16):
            cases.append(("wide", dt, H, 17, 13))
    for dt in (F32, BF16):
        cases.append(("long", dt, 64, 7, 40))
    return cases


def lstm_case_state(case):
    """Short cases start from a random carried pair (with V = 1 and h_0 = 0 the recurrent weights would not matter, with cell_0 = 0 the
    forget gate would not); the others from zeros."""
    return case[4] <= 2


def lstm_case_id(case):
    fam, dt, H, B, V = case
    return f"{fam}-{'f32' if dt == F32 else 'bf16'}-H{H}-B{B}-V{V}"


def lstm_data(B, V, H, seed=None, with_state=False):
    """gru_data's recipe with four gates: W_hh ~ N(0, 1/H), b_hh ~ 0.1 N, Gi, dh_last ~ N(0, 1), h0, c0 ~ 0.5 N; seed B 1000 + H + V."""
    g = torch.Generator().manual_seed(B * 1000 + H + V if seed is None else seed)
    w_hh = torch.randn(4 * H, H, generator=g) / math.sqrt(H)
    b_hh = torch.randn(4 * H, generator=g) * 0.1
    Gi = torch.randn(B, V, 4 * H, generator=g)
    dh = torch.randn(B, H, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.5 if with_state else None
    c0 = torch.randn(B, H, generator=g) * 0.5 if with_state else None
    return w_hh, b_hh, Gi, dh, h0, c0


def lstm_run(Gi, w, b, dh_last, h0=None, c0=None, rnd=ident, mutation=None):
    """nn.LSTMCell stepped over V inputs and its backward through time, written out in float64.  Gate order i, f, g, o.
    Gi (B, V, 4H) input projections, w (4H, H), b (4H), dh_last (B, H) the gradient at the last hidden state, h0 / c0 (B, H) or None.
    Returns Hall (B, V+1, H), h_V, cell_V (B, H), dG (B, V, 4H) = [d a_i | d a_f | d a_g | d a_o].

    rnd is applied where the kernels of csrc/lstm.hip store in their storage type (ident: the pure float64 reference):
      forward   the LDS copy of h that feeds the MFMAs, the stored Hall, and the six tape values i, f, g, o, cell_{t-1}, tanh(cell_t);
                the masters of h and cell, h_out and cell_out stay f32 (here: unrounded);
      backward  the gate values are the tape's; the four blocks of dG, stored and (the same rounded values, from the LDS tile) fed to
                the MFMAs of dh <- dG W_hh; dh and dcell stay f32.
    mutation (test_lstm_host.py's sensitivity checks): "drop_cell_carry": dcell loses its dct f term for t < V - 3; "swap_fg": the f and
    g row blocks of W_hh change places."""
    B, V, H4 = Gi.shape
    H = H4 // 4
    if mutation == "swap_fg":
        w = torch.cat([w[:H], w[2 * H:3 * H], w[H:2 * H], w[3 * H:]], 0)
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
    dh, dcell = dh_last, torch.zeros(B, H, dtype=torch.float64)
    dG = torch.zeros(B, V, 4 * H, dtype=torch.float64)
    for t in range(V - 1, -1, -1):
        i, f, g, o, cp, tc = tape[t]
        do_pre = dh * tc * o * (1 - o)
        dct = dcell + dh * o * (1 - tc * tc)
        di_pre = dct * g * i * (1 - i)
        df_pre = dct * cp * f * (1 - f)
        dg_pre = dct * i * (1 - g * g)
        dG[:, t] = torch.cat([rnd(di_pre), rnd(df_pre), rnd(dg_pre), rnd(do_pre)], 1)
        dcell = dct * f
        if mutation == "drop_cell_carry" and t < V - 3:
            dcell = torch.zeros_like(dcell)
        dh = dG[:, t] @ w
    return torch.stack(hall, 1), h, cell, dG


def lstm_step_errors(hall, dG, ref_hall, ref_dG):
    """Per-step errors {block: (V,)} of the hidden states h_1 .. h_V and of the four blocks of dG."""
    H = ref_hall.shape[2]
    hall, dG = torch.as_tensor(hall).detach().double().cpu(), torch.as_tensor(dG).detach().double().cpu()
    out = {"Hall": per_step_err(hall[:, 1:], ref_hall[:, 1:])}
    for i, name in enumerate(LSTM_BLOCKS[1:]):
        out[name] = per_step_err(dG[:, :, i * H:(i + 1) * H], ref_dG[:, :, i * H:(i + 1) * H])
    return out


def lstm_violations(errs, tol):
    """[(block, step, error, bound)] where a per-step error is not within its bound (a NaN is a violation)."""
    bad = []
    for k in LSTM_BLOCKS:
        for t, (e, b) in enumerate(zip(errs[k].tolist(), tol[k].tolist())):
            if not e <= b:
                bad.append((k, t, e, b))
    return bad


_REFS = {}


def lstm_reference(dt, B, V, H, seed=None, with_state=False, zero_weights=False):
    """Inputs as the device stores them, the float64 reference, and the per-step tolerances {block: (V,)}; computed once per argument
    set and shared (callers do not modify it).  f32: the constants above.  bf16: 4 x e_model(t), e_model = the error of the emulation
    (lstm_run with bf16 rounding) against float64."""
    key = (dt, B, V, H, seed, with_state, zero_weights)
    if key in _REFS:
        return _REFS[key]
    w_hh, b_hh, Gi, dh, h0, c0 = lstm_data(B, V, H, seed, with_state)
    if zero_weights:          # ... and input projections that differ in every (b, t, j): a shuffled ramp over [-3, 3]
        w_hh, b_hh = torch.zeros_like(w_hh), torch.zeros_like(b_hh)
        n = Gi.numel()
        Gi = torch.linspace(-3, 3, n)[torch.randperm(n, generator=torch.Generator().manual_seed(n))].reshape(Gi.shape)
    wr, br, gir, dhr = rounded(w_hh, dt), b_hh.double(), rounded(Gi, dt), dh.double()
    h0r, c0r = (None, None) if h0 is None else (h0.double(), c0.double())
    hall, hV, cV, dG = lstm_run(gir, wr, br, dhr, h0r, c0r)
    if dt == F32:
        tol = {k: torch.full((V,), v, dtype=torch.float64) for k, v in LSTM_TOL_F32.items()}
        e_model = None
    else:
        em = lstm_run(gir, wr, br, dhr, h0r, c0r, rnd=to_bf16)
        e_model = lstm_step_errors(em[0], em[3], hall, dG)
        tol = {k: LSTM_MODEL_FACTOR * v for k, v in e_model.items()}
    ref = dict(w_hh=w_hh, b_hh=b_hh, Gi=Gi, dh=dh, h0=h0, c0=c0, wr=wr, br=br, gir=gir, dhr=dhr, h0r=h0r, c0r=c0r, hall=hall, hV=hV,
               cV=cV, dG=dG, tol=tol, e_model=e_model)
    _REFS[key] = ref
    return ref


def lstm_closed_form_zero_weights(gir, h0=None, c0=None):
    """W_hh = 0, b_hh = 0: cell_t = sigmoid(a_f) cell_{t-1} + sigmoid(a_i) tanh(a_g), h_t = sigmoid(a_o) tanh(cell_t) elementwise (no
    matrix product at all); h0 only shows in Hall[:, 0]."""
    B, V, H4 = gir.shape
    H = H4 // 4
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    cell = torch.zeros(B, H, dtype=torch.float64) if c0 is None else c0
    hs = [h]
    for t in range(V):
        a = gir[:, t]
        cell = torch.sigmoid(a[:, H:2 * H]) * cell + torch.sigmoid(a[:, :H]) * torch.tanh(a[:, 2 * H:3 * H])
        hs.append(torch.sigmoid(a[:, 3 * H:]) * torch.tanh(cell))
    return torch.stack(hs, 1), cell


def lstm_cell_autograd(Gi, w, b, dh_last, h0=None, c0=None):
    """The same recurrence through float64 torch.nn.LSTMCell under autograd; Gi enters as the cell's input through an identity W_ih, so
    that its gradient is dG.  Returns Hall, h_V, cell_V, dG."""
    B, V, H4 = Gi.shape
    H = H4 // 4
    cell_mod = torch.nn.LSTMCell(H4, H).double()
    with torch.no_grad():
        cell_mod.weight_ih.copy_(torch.eye(H4, dtype=torch.float64))
        cell_mod.bias_ih.zero_()
        cell_mod.weight_hh.copy_(w)
        cell_mod.bias_hh.copy_(b)
    x = Gi.clone().requires_grad_(True)
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    c = torch.zeros(B, H, dtype=torch.float64) if c0 is None else c0
    hall = [h]
    for t in range(V):
        h, c = cell_mod(x[:, t], (h, c))
        hall.append(h)
    h.backward(dh_last)
    return torch.stack(hall, 1).detach(), h.detach(), c.detach(), x.grad


def lstm_model_reference(z, params, prefix="", h0=None, c0=None):
    """AudioLSTMModel in float64 under autograd: z (B, E, V), params {name: tensor} with the lstmCell names -> (h_V, cell_V)."""
    w_ih, w_hh = params[prefix + "weight_ih"], params[prefix + "weight_hh"]
    b_ih, b_hh = params.get(prefix + "bias_ih"), params.get(prefix + "bias_hh")
    B, _, V = z.shape
    H = w_hh.shape[1]
    h = torch.zeros(B, H, dtype=z.dtype) if h0 is None else h0
    c = torch.zeros(B, H, dtype=z.dtype) if c0 is None else c0
    for t in range(V):
        a = z[:, :, t] @ w_ih.T + h @ w_hh.T
        if b_ih is not None:
            a = a + b_ih + b_hh
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        c = f * c + i * torch.tanh(a[:, 2 * H:3 * H])
        h = o * torch.tanh(c)
    return h, c


def _is_buffer(k):
    return ("running_" in k) or k.endswith("num_batches_tracked")


class LstmOracle:
    """The reference train step (oracle.OracleTrainer's loop body) in float64 with the LSTM context: the oracle's encoder,
    lstm_model_reference, the predictor, the oracle's score functions, info_nce_loss, validation_terms and adam_update, differentiated
    by torch autograd."""

    PREFIX = "autoregressive_model.lstmCell."

    def __init__(self, params, visible_steps, prediction_steps, score="softplus", all_timesteps=False, regularization=1.0, lr=1e-4,
                 scalogram=None):
        from oracle import cpc_oracle as O
        self.O = O
        self.buffers = {k: (v.detach().clone().double() if v.is_floating_point() else v.detach().clone()) for k, v in params.items()
                        if _is_buffer(k)}
        self.params = {k: v.detach().clone().double().requires_grad_(True) for k, v in params.items() if not _is_buffer(k)}
        self.m = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.V, self.K = visible_steps, prediction_steps
        self.score, self.all_timesteps, self.regularization, self.lr = O.SCORE_FUNCTIONS[score], all_timesteps, regularization, lr
        self.scalogram = scalogram
        self.t = 0

    def forward(self, batch, training=True):
        O = self.O
        p = {**self.params, **self.buffers}
        x = batch.double()
        if self.scalogram is not None:
            enc = O.scalogram_encoder_forward(x, p, self.scalogram, training)
        else:
            enc = O.encoder_forward(x.unsqueeze(1), p)
        K, V = self.K, self.V
        targets, z = enc[:, :, -K:], enc[:, :, -(V + K):-K]
        c, _ = lstm_model_reference(z, p, self.PREFIX)
        pred = (c @ p["prediction_model.weight"].t()).view(-1, K, enc.shape[1])
        return pred, targets, z, c

    def loss_and_grads(self, batch):
        for p in self.params.values():
            p.grad = None
        pred, targ, _, _ = self.forward(batch)
        loss, smax = self.O.info_nce_loss(self.score(pred, targ), self.all_timesteps, self.regularization)
        loss.backward()
        return loss.detach(), smax.detach(), {k: p.grad for k, p in self.params.items()}

    def step(self, batch):
        loss, smax, grads = self.loss_and_grads(batch)
        self.t += 1
        with torch.no_grad():
            for k, p in self.params.items():
                self.O.adam_update(p, grads[k], self.m[k], self.v[k], self.t, self.lr)
        return float(loss), float(smax)

    def validation(self, batch):
        with torch.no_grad():
            pred, targ, _, _ = self.forward(batch, training=False)
            return self.O.validation_terms(self.score(pred, targ), self.all_timesteps)
