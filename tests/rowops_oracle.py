"""Checker for the training-side row kernels (csrc/loss.hip, optim.hip, rowops.hip): every operation restated in plain fp64
torch on the CPU, with no project kernel behind it.  Inputs are taken as they are (already rounded to the kernel's input
type by the caller) and widened to fp64, so what a comparison against these functions measures is the kernel's own
arithmetic, not the rounding of its inputs.

Besides the values, the gradient functions return the SUM OF MAGNITUDES of the terms each output element is made of
(``mag``): an element-wise bound ``|got - ref| <= tol * mag`` stays meaningful where the terms cancel (a softmax
probability of 3e-5 next to a target entry of 0.9), which a bound relative to the tensor's maximum does not."""
import torch


def _d(t):
    return t.detach().double().cpu()


# ------------------------------------------------------------------------------------------------ loss
def log_softmax(z):
    """(lp [N, V], lse [N]) of logits z."""
    z = _d(z)
    mx = z.max(dim=-1, keepdim=True).values
    lse = mx + (z - mx).exp().sum(dim=-1, keepdim=True).log()
    return z - lse, lse.squeeze(-1)


def log_softmax_bwd(dlp, lp):
    """(dlogits, mag): dlogits = dlp - exp(lp) * sum_v dlp."""
    dlp, lp = _d(dlp), _d(lp)
    s = dlp.sum(dim=-1, keepdim=True)
    p = lp.exp()
    return dlp - p * s, dlp.abs() + p * s.abs()


def _onehot(target, V):
    """[N, V] indicator of the target column; rows whose target is outside [0, V) are all zero."""
    t = target.detach().cpu().long().view(-1)
    valid = (t >= 0) & (t < V)
    oh = torch.zeros(t.numel(), V, dtype=torch.float64)
    rows = torch.nonzero(valid).view(-1)
    oh[rows, t[rows]] = 1.0
    return oh, t


def smoothed_nll(lp, target, eps, ignore_index):
    """Per-row label-smoothed NLL [N] on log-probs: (1 - eps) * -lp[t] + eps / V * -sum(lp); 0 for ignored rows.  A target
    outside [0, V) that is not ``ignore_index`` contributes no NLL term (csrc/loss.hip, smoothed_nll_fwd_kernel)."""
    lp = _d(lp)
    V = lp.shape[-1]
    oh, t = _onehot(target, V)
    loss = (1.0 - eps) * -(lp * oh).sum(-1) + (eps / V) * -lp.sum(-1)
    return loss.masked_fill(t == ignore_index, 0.0)


def smoothed_nll_bwd(dloss, target, V, eps, ignore_index):
    """dlp [N, V] for an upstream per-row gradient dloss [N]: -g * eps / V everywhere, -g * (1 - eps) more at the target."""
    oh, t = _onehot(target, V)
    g = _d(dloss).view(-1).masked_fill(t == ignore_index, 0.0).unsqueeze(-1)
    return -g * (eps / V) - g * (1.0 - eps) * oh


def xent(z, target, eps, ignore_index, grad_scale):
    """The fused loss: (loss_rows [N], dlogits [N, V], mag [N, V]) with
    dlogits = grad_scale * (softmax(z) - eps / V - (1 - eps) * [c == t]) and mag the same terms added by magnitude.
    Ignored rows: loss 0, gradient 0, mag 0.  Out-of-range, not ignored target: no NLL term in the loss and no column gets
    the (1 - eps) term (what xent_fused_kernel does; such a target never comes out of a vocabulary)."""
    lp, _ = log_softmax(z)
    V = lp.shape[-1]
    oh, t = _onehot(target, V)
    loss = smoothed_nll(lp, target, eps, ignore_index)
    p = lp.exp()
    keep = (t != ignore_index).double().unsqueeze(-1)
    dl = grad_scale * (p - eps / V - (1.0 - eps) * oh) * keep
    mag = grad_scale * (p + eps / V + (1.0 - eps) * oh) * keep
    return loss, dl, mag


# ------------------------------------------------------------------------------------------------ optimizer
def clip_coef(sumsq, max_norm, grad_scale):
    """The factor every gradient element is multiplied by (comment above clip_scale / in clip_adam_kernel):
    grad_scale * min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6)); grad_scale alone without a norm or with max_norm <= 0."""
    if sumsq is None or max_norm <= 0:
        return float(grad_scale)
    total_norm = grad_scale * float(sumsq) ** 0.5
    return float(grad_scale) * min(1.0, max_norm / (total_norm + 1e-6))


def adam_step(p, g, m, v, sumsq, max_norm, grad_scale, lr, b1, b2, eps, step):
    """One clipped Adam step (torch.optim.Adam's arithmetic, no weight decay): new (p, m, v) in fp64."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    g = g * clip_coef(sumsq, max_norm, grad_scale)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / (1.0 - b2 ** step) ** 0.5 + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


# ------------------------------------------------------------------------------------------------ embeddings
def embed_grads(ids, pos, types, dsum, V, P, NT, pad_id):
    """(dword [V, d], dpos [P, d], dtype [NT, d]): the rows of dsum [n, d] summed per word / position / type id; the
    ``pad_id`` word row gets nothing.  ``pos`` / ``types`` are full [n] id vectors (the caller spells out n % seq_len / 0)."""
    dsum = _d(dsum)
    d = dsum.shape[1]
    ids, pos, types = (t.detach().cpu().long().view(-1) for t in (ids, pos, types))
    keep = ids != pad_id
    dword = torch.zeros(V, d, dtype=torch.float64).index_add_(0, ids[keep], dsum[keep])
    dpos = torch.zeros(P, d, dtype=torch.float64).index_add_(0, pos, dsum)
    dtyp = torch.zeros(NT, d, dtype=torch.float64).index_add_(0, types, dsum)
    return dword, dpos, dtyp


def embed_grad_mags(ids, pos, types, dsum, V, P, NT, pad_id):
    """embed_grads over |dsum|: what a bound on sums whose order is free (fp32 atomics) is scaled by."""
    return embed_grads(ids, pos, types, _d(dsum).abs(), V, P, NT, pad_id)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd_bwd(x, gamma, beta, dy, eps):
    """(y, mean, rstd, dx, dgamma, dbeta) of y = (x - mean) * rstd * gamma + beta over the last axis (biased variance)."""
    x, gamma, beta, dy = _d(x), _d(gamma), _d(beta), _d(dy)
    d = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / (var + eps).sqrt()
    xh = (x - mean) * rstd
    y = xh * gamma + beta
    dg = dy * gamma
    c1 = dg.sum(-1, keepdim=True) / d
    c2 = (dg * xh).sum(-1, keepdim=True) / d
    dx = rstd * (dg - c1 - xh * c2)
    return y, mean.squeeze(-1), rstd.squeeze(-1), dx, (dy * xh).sum(0), dy.sum(0)


LN_TOL = {torch.float32: 1e-5, torch.bfloat16: 1.5e-2}   # of the row's largest |y|; bf16: two roundings of 2^-7 and slack


def layernorm_bounds(x, y_ref, rstd_ref, dtype):
    """Element-wise bounds (y [rows, 1], mean [rows], rstd [rows]) of a LayerNorm forward over the rows ``x`` in ``dtype``:
    y within LN_TOL of the row's largest |y_ref|; an fp32 sum of d terms is off by a few ulp of sum|x|, so the mean by that
    over d; rstd is well conditioned.  One definition for tests/test_gpu_row_edges.py and tests/test_gpu_dense_ln_edges.py."""
    y_ref, rstd_ref = _d(y_ref), _d(rstd_ref)
    return LN_TOL[dtype] * y_ref.abs().max(dim=-1, keepdim=True).values, 1e-5 * _d(x).abs().mean(-1), 1e-5 * rstd_ref


def layernorm_dx_bound(dx_ref, dtype):
    """Element-wise bound [rows, 1] of imt_layernorm_bwd's dx: twice the forward tolerance of the row's largest |dx_ref|."""
    return 2 * LN_TOL[dtype] * _d(dx_ref).abs().max(dim=-1, keepdim=True).values


def layernorm_param_grad_mags(x, dy, eps):
    """(sum_rows |dy * xhat|, sum_rows |dy|): the magnitudes the column sums dgamma / dbeta are made of."""
    x, dy = _d(x), _d(dy)
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / (((x - mean) ** 2).mean(-1, keepdim=True) + eps).sqrt()
    return (dy * (x - mean) * rstd).abs().sum(0), dy.abs().sum(0)
