"""float64 references for the stacked GRU context (AudioGRUModel(num_layers > 1)): the backward sweep of one layer that receives a
gradient at every hidden state (cpc_gru_bwd_steps), its bf16 emulation, the cases of the kernel tests, and the whole model composed
from the oracle's pieces with torch autograd.  Shared by test_gru_stacked_host.py and test_gru_stacked_gpu.py; nothing here touches a
device, and the oracle is imported, not edited.
"""
import torch

from context_reference import (BF16, F32, GRU_MODEL_FACTOR, GRU_TOL_F32, gru_data, gru_step_errors, ident, rounded, to_bf16)
from oracle import cpc_oracle as O


# ------------------------------------------------------------------------------------------------------------------ one layer
def gru_run_steps(Gi, w, b, dc, dhs, h0=None, rnd=ident, mutation=None):
    """context_reference.gru_run with a gradient dhs (B, V, H) that arrives at h_{t+1} from outside the recurrence: step t starts from
    d = dh + dhs[:, t], and both the gate derivatives and the d u term that goes on to step t - 1 use this d.  dc (B, H) or None (zeros).
    rnd is applied at the same places as in gru_run (the dhs the caller hands in are already in the storage type).
    Returns Hall (B, V+1, H), c (B, H), dG (B, V, 4H).
    mutation: "shift" reads dhs[:, t + 1] (zero beyond the end) instead of dhs[:, t]; "after_keep" adds dhs only after the keep term
    d u has been formed from the recurrent dh alone."""
    B, V, H3 = Gi.shape
    H = H3 // 3
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    hall, tape = [rnd(h)], []
    for t in range(V):
        gh = rnd(h) @ w.T + b
        r = torch.sigmoid(Gi[:, t, :H] + gh[:, :H])
        u = torch.sigmoid(Gi[:, t, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        n = torch.tanh(Gi[:, t, 2 * H:] + r * q)
        tape.append((rnd(r), rnd(u), rnd(n), rnd(q), rnd(h)))
        h = (1 - u) * n + u * h
        hall.append(rnd(h))
    c = h
    dh = torch.zeros(B, H, dtype=torch.float64) if dc is None else dc
    dG = torch.zeros(B, V, 4 * H, dtype=torch.float64)
    for t in range(V - 1, -1, -1):
        r, u, n, q, hp = tape[t]
        if mutation == "shift":
            ext = dhs[:, t + 1] if t + 1 < V else torch.zeros_like(dh)
        else:
            ext = dhs[:, t]
        if mutation == "after_keep":
            keep = dh * u
            d = dh + ext
        else:
            d = dh + ext
            keep = d * u
        dn_pre = d * (1 - u) * (1 - n * n)
        du_pre = d * (hp - n) * u * (1 - u)
        dr_pre = dn_pre * q * r * (1 - r)
        dnr = dn_pre * r
        dG[:, t] = torch.cat([rnd(dr_pre), rnd(du_pre), rnd(dn_pre), rnd(dnr)], 1)
        dh = keep + torch.cat([rnd(dr_pre), rnd(du_pre), rnd(dnr)], 1) @ w
    return torch.stack(hall, 1), c, dG


# (H, B, V) of every kernel case: B = 1 and 17 leave rows of a 16-row workgroup to mask, V = 1 has no step to prefetch, V = 2 is the
# first prefetched step, H = 96 and 224 have waves with unequal or no tiles, H = 288 and 512 run the 8-wave form, (64, 7, 40) is long
def stacked_cases():
    cases = [(H, B, V) for H in (32, 64, 128, 256) for B in (1, 17, 33) for V in (1, 2, 13)]
    return cases + [(96, 17, 13), (224, 1, 13), (288, 17, 13), (512, 17, 13), (64, 7, 40)]


def stacked_case_id(case):
    return "H%d-B%d-V%d" % case


def stacked_case_seed(case):
    """The data seed of gru_data: its default (B 1000 + H + V), except the long case, which keeps context_reference.gru_case_seed's
    seed 2 (with the default seed the emulation of the plain sweep already passes the cap there, see gru_case_seed)."""
    return 2 if case == (64, 7, 40) else None


def stacked_reference(dt, case, with_dc=True, mutation=None):
    """Inputs as the device stores them, the float64 reference and the per-step tolerances {block: (V,)} of one case.
    Data: gru_data's recipe; dhs ~ N(0, 1) from its own generator, rounded to the storage type; a carried h0 when V <= 2.
    f32: GRU_TOL_F32.  bf16: GRU_MODEL_FACTOR x the error of the bf16 emulation (gru_run_steps with bf16 rounding) at that step.
    mutation: the reference (and in bf16 the emulation) computed with that deliberate mistake instead -- 'what a wrong kernel gives'."""
    H, B, V = case
    w_hh, b_hh, Gi, dc, h0 = gru_data(B, V, H, stacked_case_seed(case), with_h0=V <= 2)
    g = torch.Generator().manual_seed(77 + 1000 * B + H + V)
    dhs = torch.randn(B, V, H, generator=g)
    if not with_dc:
        dc = None
    wr, br, gir, dhr = rounded(w_hh, dt), b_hh.double(), rounded(Gi, dt), rounded(dhs, dt)
    dcr = None if dc is None else dc.double()
    h0r = None if h0 is None else h0.double()
    hall, c, dG = gru_run_steps(gir, wr, br, dcr, dhr, h0r)
    out = dict(w_hh=w_hh, b_hh=b_hh, Gi=Gi, dc=dc, h0=h0, dhs=dhs, hall=hall, c=c, dG=dG)
    if dt == F32:
        out["tol"] = {k: torch.full((V,), v, dtype=torch.float64) for k, v in GRU_TOL_F32.items()}
        out["e_model"] = None
        if mutation:
            out["mutant"] = gru_run_steps(gir, wr, br, dcr, dhr, h0r, mutation=mutation)
    else:
        emu = gru_run_steps(gir, wr, br, dcr, dhr, h0r, rnd=to_bf16)
        out["e_model"] = gru_step_errors(emu[0], emu[2], hall, dG)
        out["tol"] = {k: GRU_MODEL_FACTOR * v for k, v in out["e_model"].items()}
        if mutation:
            out["mutant"] = gru_run_steps(gir, wr, br, dcr, dhr, h0r, rnd=to_bf16, mutation=mutation)
    return out


def zero_weight_gates(gir):
    """W_hh = 0, b_hh = 0 (gru_closed_form_zero_weights' setting): the gates depend on the input projections alone.
    Returns r, u, n (B, V, H) and the hidden states before each step hp (B, V, H), h_0 = 0; q = 0."""
    B, V, H3 = gir.shape
    H = H3 // 3
    r, u, n = torch.sigmoid(gir[..., :H]), torch.sigmoid(gir[..., H:2 * H]), torch.tanh(gir[..., 2 * H:])
    h, hp = torch.zeros(B, H, dtype=torch.float64), []
    for t in range(V):
        hp.append(h)
        h = (1 - u[:, t]) * n[:, t] + u[:, t] * h
    return r, u, n, torch.stack(hp, 1)


EXACT_N_STEPS = 7          # n = +-1 only at steps 0 .. 6: h then never needs more than 7 significant bits


def exact_gate_data(B, V, H, seed=0):
    """Input projections (B, V, 3H) for the zero-weight setting whose gates the bf16 tape holds exactly, so that the only rounding of
    weight between the closed form and a bf16 sweep is the store of its result.  Pre-activations of r and n are -12, 0 or +12 (exact
    in bf16): r in {6.1e-6, 0.5, 1 - 6.1e-6} (bf16 holds the last as 1: 6.1e-6 off), n in {-1, 0, +1} up to 8e-11, different in every
    (b, t, j); n = 0 from step EXACT_N_STEPS on.  The pre-activation of u is 0 everywhere, u = 0.5: h_t = (n_t + h_{t-1}) / 2 is then
    a dyadic number of at most EXACT_N_STEPS significant bits (bf16 holds 8), and the gradient handed down is d 2^-k, exact as well.
    (With u at the extremes too, h leaves its dyadic value by up to 1.2e-5 per step, stops being representable, and the tape's
    h_prev is back to a full rounding where |h| is small.)"""
    g = torch.Generator().manual_seed(1000 * B + H + V + seed)
    lvl = torch.tensor([-12.0, 0.0, 12.0])
    a_r = lvl[torch.randint(0, 3, (B, V, H), generator=g)]
    a_n = lvl[torch.randint(0, 3, (B, V, H), generator=g)]
    a_n[:, EXACT_N_STEPS:] = 0.0
    return torch.cat([a_r, torch.zeros(B, V, H), a_n], 2)


# ------------------------------------------------------------------------------------------------------------------ whole model
def gru_prefixes(num_layers):
    return ["autoregressive_model.gruCell."] + [f"autoregressive_model.upper_cells.{i}." for i in range(num_layers - 1)]


def stacked_gru_forward(z, params, num_layers, h0=None, return_states=False):
    """AudioGRUModel(num_layers).forward on z (B, E, V): at every step layer l's cell reads the new hidden state of layer l - 1
    (oracle gru_cell per layer).  h0: list of per-layer states or None (zeros).  Returns the top layer's last state (and all last states)."""
    pre = gru_prefixes(num_layers)
    B = z.shape[0]
    H = params[pre[0] + "weight_hh"].shape[1]
    hs = [torch.zeros(B, H, dtype=z.dtype) if h0 is None else h0[l] for l in range(num_layers)]
    for t in range(z.shape[2]):
        x = z[:, :, t]
        for l, p in enumerate(pre):
            hs[l] = O.gru_cell(x, hs[l], params[p + "weight_ih"], params[p + "weight_hh"], params.get(p + "bias_ih"), params.get(p + "bias_hh"))
            x = hs[l]
    return (hs[-1], hs) if return_states else hs[-1]


def _is_buffer(k):
    return ("running_" in k) or k.endswith("num_batches_tracked")


class StackedOracle:
    """The reference train step (oracle.OracleTrainer's loop body) in float64 with a stacked GRU context: the oracle's encoder, its
    gru_cell per layer, its score functions, info_nce_loss, validation_terms and adam_update, differentiated by torch autograd."""

    def __init__(self, params, visible_steps, prediction_steps, num_layers, score="softplus", all_timesteps=False, regularization=1.0,
                 lr=1e-4, scalogram=None):
        self.buffers = {k: (v.detach().clone().double() if v.is_floating_point() else v.detach().clone()) for k, v in params.items()
                        if _is_buffer(k)}
        self.params = {k: v.detach().clone().double().requires_grad_(True) for k, v in params.items() if not _is_buffer(k)}
        self.m = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.V, self.K, self.L = visible_steps, prediction_steps, num_layers
        self.score, self.all_timesteps, self.regularization, self.lr = O.SCORE_FUNCTIONS[score], all_timesteps, regularization, lr
        self.scalogram = scalogram
        self.t = 0

    def forward(self, batch, training=True, params=None):
        p = {**(self.params if params is None else params), **self.buffers}
        x = batch.double()
        if self.scalogram is not None:
            enc = O.scalogram_encoder_forward(x, p, self.scalogram, training)
        else:
            enc = O.encoder_forward(x.unsqueeze(1), p)
        K, V = self.K, self.V
        targets, z = enc[:, :, -K:], enc[:, :, -(V + K):-K]
        c = stacked_gru_forward(z, p, self.L)
        pred = (c @ p["prediction_model.weight"].t()).view(-1, K, enc.shape[1])
        return pred, targets, z, c

    def loss_and_grads(self, batch):
        for p in self.params.values():
            p.grad = None
        pred, targ, _, _ = self.forward(batch)
        loss, smax = O.info_nce_loss(self.score(pred, targ), self.all_timesteps, self.regularization)
        loss.backward()
        return loss.detach(), smax.detach(), {k: p.grad for k, p in self.params.items()}

    def step(self, batch):
        loss, smax, grads = self.loss_and_grads(batch)
        self.t += 1
        with torch.no_grad():
            for k, p in self.params.items():
                O.adam_update(p, grads[k], self.m[k], self.v[k], self.t, self.lr)
        return float(loss), float(smax)

    def validation(self, batch):
        with torch.no_grad():
            pred, targ, _, _ = self.forward(batch, training=False)
            return O.validation_terms(self.score(pred, targ), self.all_timesteps)
