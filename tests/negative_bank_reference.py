"""Float64 torch restatement of the banked InfoNCE loss (include/cpc_hip.h, cpc_nce_loss_banked; DESIGN.md, "Negative bank").

A ring of ``slots`` slots of B prediction rows, N = slots B; ``valid`` a bit mask of the filled slots (bit ``cur`` always set); with
sp = f(S), f the identity or softplus, and V the rows of the valid slots:

    S[k][r][b'] = < R[r][k][:], targets[b'][:, k] >                      r in [0, N)
    loss = -mean_{b',k} sp[k][cur B + b'][b'] + mean_{k,b'} logsumexp_{r in V} sp[k][r][b']
           + reg * mean_{b,b'} (mean_k sp[k][cur B + b][b'])^2
    dsp[k][r][b'] = [r in V] exp(sp - lse[k][b']) / (B K) - [r == cur B + b'] / (B K) + [r in slot cur] 2 reg / (B^2 K) mean_k sp[k][r][b']
    dL/dS = dsp * f'(S)

banked_terms is the definition on given scores, banked_reference the values a kernel is compared with (gradient by autograd),
banked_gradient_formula the closed form above, banked_loss the whole loss from (ring, targets), differentiable in both."""
import torch
import torch.nn.functional as F


def row_mask(B, slots, valid):
    """bool [slots B]: the rows of the slots whose bit is set in ``valid``."""
    return torch.tensor([bool((valid >> s) & 1) for s in range(slots)]).repeat_interleave(B)


def banked_terms(S, B, cur, valid, softplus, reg):
    """S [K][N][B] (any float dtype, may require grad) -> dict of the loss, its three terms, the max score and lse [K][B]."""
    K, N, _ = S.shape
    slots = N // B
    assert N == slots * B and 0 <= cur < slots and (valid >> cur) & 1 and valid >> slots == 0
    sp = F.softplus(S) if softplus else S
    own = sp[:, cur * B:(cur + 1) * B, :]
    rows = row_mask(B, slots, valid).to(S.device)
    lse = torch.logsumexp(sp.masked_fill(~rows[None, :, None], float("-inf")), dim=1)
    t_valid = -torch.diagonal(own, dim1=1, dim2=2).mean()
    t_lse = lse.mean()
    t_reg = reg * (own.mean(dim=0) ** 2).mean()
    return dict(loss=t_valid + t_lse + t_reg, smax=own.max(), t_valid=t_valid, t_lse=t_lse, t_reg=t_reg, lse=lse, sp=sp)


def banked_reference(S, B, cur, valid, softplus, reg):
    """The float64 values for f32 scores S [K][N][B]: loss, out[0..5] as cpc_nce_loss_banked writes them, dS [K][N][B] and
    dST_cur [K][B][B] (dST_cur[k][b'][b] = dS[k][cur B + b][b'])."""
    lin = S.detach().double().requires_grad_(True)
    t = banked_terms(lin, B, cur, valid, softplus, reg)
    if bool(torch.isfinite(t["loss"])):
        t["loss"].backward()
    pre = (t["t_valid"] + t["t_lse"]).item()
    out = [t["loss"].item(), t["smax"].item(), t["t_valid"].item(), t["t_lse"].item(), t["t_reg"].item(), 1.0 if pre != pre else 0.0]
    dS = lin.grad
    dST = None if dS is None else dS[:, cur * B:(cur + 1) * B, :].transpose(1, 2).contiguous()
    return dict(loss=out[0], out=out, dS=dS, dST_cur=dST, lse=t["lse"].detach(), sp=t["sp"].detach())


def banked_gradient_formula(S, B, cur, valid, softplus, reg):
    """dL/dS by the closed form of the definition (no autograd), float64 [K][N][B]."""
    S = S.detach().double()
    K, N, _ = S.shape
    t = banked_terms(S, B, cur, valid, softplus, reg)
    sp, lse = t["sp"], t["lse"]
    rows = row_mask(B, N // B, valid)
    dsp = torch.exp(sp - lse[:, None, :]) * rows[None, :, None] / (B * K)
    own = slice(cur * B, (cur + 1) * B)
    dsp[:, own, :] -= torch.eye(B, dtype=torch.float64)[None] / (B * K)
    dsp[:, own, :] += 2.0 * reg / (B * B * K) * sp[:, own, :].mean(dim=0, keepdim=True)
    return dsp * (torch.sigmoid(S) if softplus else 1.0)


def banked_scores(ring, targets):
    """ring [N][K][E], targets [B][E][K] -> S [K][N][B]."""
    return torch.einsum("rke,bek->krb", ring, targets)


def banked_loss(ring, targets, cur, valid, softplus, reg):
    """The whole loss from the ring (slot cur: this step's predictions, attached to the graph where they should take a gradient; the
    other slots detached constants) and the targets [B][E][K].  Returns (loss, max score)."""
    t = banked_terms(banked_scores(ring, targets), targets.shape[0], cur, valid, softplus, reg)
    return t["loss"], t["smax"]
