"""tests/rowops_oracle.py against torch autograd in fp64 and the stored loss vectors, plus the refusals of the row kernels'
C entry points that are decided on the host (no GPU anywhere in this file)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from imagetranslate_amd import _lib as L
from tests import rowops_oracle as RO

ERR, UNSUPPORTED = -1, -2


def _close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), err


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("V", [3, 37, 1030])
def test_xent_matches_autograd(V):
    from oracle.reference_model import SmoothedNLLLoss
    g = torch.Generator().manual_seed(V)
    N, eps, gs = 9, 0.1, 1.0 / 9
    z = (torch.randn(N, V, generator=g) * 3).double()
    tgt = torch.randint(1, V, (N,), generator=g)
    tgt[2] = 0  # ignored
    zr = z.clone().requires_grad_(True)
    lp_ref = F.log_softmax(zr, dim=-1)
    loss_ref = SmoothedNLLLoss(ignore_index=0, epsilon=eps)(lp_ref, tgt)
    (loss_ref.sum() * gs).backward()
    lp, lse = RO.log_softmax(z)
    _close(lp, lp_ref)
    _close(lse, torch.logsumexp(z, -1))
    _close(RO.smoothed_nll(lp, tgt, eps, 0), loss_ref.view(-1))
    loss, dl, mag = RO.xent(z, tgt, eps, 0, gs)
    _close(loss, loss_ref.view(-1))
    _close(dl, zr.grad)
    assert float(loss[2]) == 0.0 and float(dl[2].abs().max()) == 0.0 and float(mag[2].abs().max()) == 0.0
    assert bool((mag >= dl.abs() - 1e-15).all())
    # the same gradient through the two backward forms
    dlp = RO.smoothed_nll_bwd(torch.full((N,), gs, dtype=torch.float64), tgt, V, eps, 0)
    dz, mag2 = RO.log_softmax_bwd(dlp, lp)
    _close(dz, zr.grad)
    assert bool((mag2 >= dz.abs() - 1e-15).all())
    # backward forms against autograd on their own
    lpr = lp.clone().requires_grad_(True)
    w = torch.randn(N, generator=g).double()
    (SmoothedNLLLoss(ignore_index=0, epsilon=eps)(lpr, tgt).view(-1) * w).sum().backward()
    _close(RO.smoothed_nll_bwd(w, tgt, V, eps, 0), lpr.grad)
    zr2 = z.clone().requires_grad_(True)
    up = torch.randn(N, V, generator=g).double()
    (F.log_softmax(zr2, -1) * up).sum().backward()
    _close(RO.log_softmax_bwd(up, lp)[0], zr2.grad)


def test_xent_out_of_range_target_has_no_nll_term():
    g = torch.Generator().manual_seed(1)
    N, V, eps, gs = 4, 11, 0.1, 0.25
    z = torch.randn(N, V, generator=g).double()
    tgt = torch.tensor([3, V + 5, -7, 0])
    loss, dl, mag = RO.xent(z, tgt, eps, 0, gs)
    lp, lse = RO.log_softmax(z)
    p = lp.exp()
    for r in (1, 2):
        _close(loss[r], (eps / V) * -lp[r].sum())
        _close(dl[r], gs * (p[r] - eps / V))
        _close(mag[r], gs * (p[r] + eps / V))
    assert float(loss[3]) == 0.0 and float(dl[3].abs().max()) == 0.0
    _close(RO.smoothed_nll(lp, tgt, eps, 0), loss)
    dlp = RO.smoothed_nll_bwd(torch.ones(N), tgt, V, eps, 0)
    _close(dlp[1], torch.full((V,), -eps / V, dtype=torch.float64))


def test_xent_replays_stored_loss_vectors():
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "loss_kat.json")))
    assert len(kat["cases"]) >= 3
    for case in kat["cases"]:
        z = torch.tensor(case["logits"], dtype=torch.float32)
        tgt = torch.tensor(case["target"], dtype=torch.long)
        loss, dl, _ = RO.xent(z, tgt, case["epsilon"], case["ignore_index"], 1.0 / len(case["target"]))
        _close(loss, torch.tensor(case["loss"], dtype=torch.float64).view(-1), 1e-6)   # the vectors were stored from fp32
        _close(dl, torch.tensor(case["dlogits_mean"], dtype=torch.float64), 1e-6)


# ------------------------------------------------------------------------------------------------ optimizer
def test_adam_step_matches_torch_adam_with_clipping():
    g = torch.Generator().manual_seed(2)
    n, lr, b1, b2, eps, max_norm = 1001, 1e-3, 0.9, 0.98, 1e-8, 1.0
    p0 = torch.randn(n, generator=g).double()
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pr], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros(n).double(), torch.zeros(n).double()
    clipped = []
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=g).double() * (5.0 if step % 2 else 0.001)
        pr.grad = grad.clone()
        torch.nn.utils.clip_grad_norm_([pr], max_norm)
        opt.step()
        ss = float((grad ** 2).sum())
        clipped.append(RO.clip_coef(ss, max_norm, 1.0) < 1.0)
        p, m, v = RO.adam_step(p, grad, m, v, ss, max_norm, 1.0, lr, b1, b2, eps, step)
        _close(p, pr.detach())
        _close(m, opt.state[pr]["exp_avg"])
        _close(v, opt.state[pr]["exp_avg_sq"])
    assert clipped == [True, False, True]


def test_clip_coef():
    assert RO.clip_coef(None, 1.0, 0.5) == 0.5 and RO.clip_coef(1e30, 0.0, 0.5) == 0.5
    assert RO.clip_coef(0.25, 1.0, 1.0) == 1.0                      # norm 0.5 < max_norm
    assert abs(RO.clip_coef(16.0, 1.0, 1.0) - 1.0 / (4.0 + 1e-6)) < 1e-15
    assert abs(RO.clip_coef(16.0, 1.0, 0.5) - 0.5 / (2.0 + 1e-6)) < 1e-15   # the norm is that of the SCALED gradient
    # a unit-scale call on the pre-scaled gradient is the same factor overall
    g = torch.tensor([3.0, -4.0]).double()
    a = g * RO.clip_coef(float((g ** 2).sum()), 1.0, 0.5)
    b = (0.5 * g) * RO.clip_coef(float(((0.5 * g) ** 2).sum()), 1.0, 1.0)
    _close(a, b)


# ------------------------------------------------------------------------------------------------ embeddings, LayerNorm
def test_embed_grads_match_autograd():
    g = torch.Generator().manual_seed(3)
    V, P, NT, d, n, pad = 13, 7, 6, 12, 40, 0
    word = torch.randn(V, d, generator=g).double().requires_grad_(True)
    pos = torch.randn(P, d, generator=g).double().requires_grad_(True)
    typ = torch.randn(NT, d, generator=g).double().requires_grad_(True)
    ids = torch.randint(0, V, (n,), generator=g)
    ids[::3] = pad
    pid = torch.randint(0, P, (n,), generator=g)
    tid = torch.randint(0, NT, (n,), generator=g)
    dsum = torch.randn(n, d, generator=g).double()
    out = F.embedding(ids, word, padding_idx=pad) + pos[pid] + typ[tid]
    (out * dsum).sum().backward()
    dw, dp, dt = RO.embed_grads(ids, pid, tid, dsum, V, P, NT, pad)
    _close(dw, word.grad)
    _close(dp, pos.grad)
    _close(dt, typ.grad)
    assert float(dw[pad].abs().max()) == 0.0
    mw, mp, mt = RO.embed_grad_mags(ids, pid, tid, dsum, V, P, NT, pad)
    assert bool((mw >= dw.abs() - 1e-12).all() and (mp >= dp.abs() - 1e-12).all() and (mt >= dt.abs() - 1e-12).all())


@pytest.mark.parametrize("rows,d", [(1, 4), (5, 516), (33, 128)])
def test_layernorm_matches_autograd(rows, d):
    g = torch.Generator().manual_seed(4)
    eps = 1e-12
    x = (torch.randn(rows, d, generator=g) * 2 + 0.5).double()
    gamma, beta = torch.randn(d, generator=g).double(), torch.randn(d, generator=g).double()
    dy = torch.randn(rows, d, generator=g).double()
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    ref = F.layer_norm(xr, (d,), gr, br, eps=eps)
    ref.backward(dy)
    y, mean, rstd, dx, dgamma, dbeta = RO.layernorm_fwd_bwd(x, gamma, beta, dy, eps)
    _close(y, ref, 1e-11)
    _close(mean, x.mean(-1))
    _close(rstd, 1.0 / (x.var(-1, unbiased=False) + eps).sqrt(), 1e-11)
    _close(dx, xr.grad, 1e-10)
    _close(dgamma, gr.grad, 1e-11)
    _close(dbeta, br.grad)
    mg, mb = RO.layernorm_param_grad_mags(x, dy, eps)
    assert bool((mg >= dgamma.abs() - 1e-9).all() and (mb >= dbeta.abs() - 1e-9).all())


# ------------------------------------------------------------------------------------------------ host refusals
@pytest.fixture(scope="module")
def lib():
    return L.load()


A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000   # well-formed addresses: never dereferenced on the host


def test_loss_entry_points_refuse_a_leading_dimension_off_the_vector_width(lib):
    for dtype in (L.IMT_F32, L.IMT_BF16):
        for ld in (1030, 1031, 1029):
            assert lib.imt_log_softmax_fwd(dtype, A, ld, B, 1032, C, 9, 1030, None) == ERR and b"log_softmax_fwd" in lib.imt_last_error()
            assert lib.imt_xent_fused_fwd_bwd(dtype, A, ld, B, C, 9, 1030, 0.1, 0, 1.0, None) == ERR and b"xent_fused" in lib.imt_last_error()
        assert lib.imt_log_softmax_fwd(dtype, A, 1032, B, 1030, C, 9, 1030, None) == ERR   # the output's, too
    # nothing to do is accepted without a launch
    assert lib.imt_log_softmax_fwd(L.IMT_F32, A, 1030, B, 1030, C, 0, 1030, None) == 0
    assert lib.imt_xent_fused_fwd_bwd(L.IMT_F32, A, 1030, B, C, 0, 1030, 0.1, 0, 1.0, None) == 0


def test_layernorm_refuses_rows_wider_than_1024(lib):
    for dtype in (L.IMT_F32, L.IMT_BF16):
        assert lib.imt_layernorm_fwd(dtype, A, B, C, D, A, B, 3, 1028, 1e-12, 0.0, 0, None) == UNSUPPORTED
        assert b"1028" in lib.imt_last_error()
        assert lib.imt_layernorm_bwd(dtype, A, B, C, D, A, B, C, D, 3, 1028, 0.0, 0, None, 0.0, 0, None, None) == UNSUPPORTED
        assert b"1028" in lib.imt_last_error()
        assert lib.imt_layernorm_fwd(dtype, A, B, C, D, A, B, 3, 1026, 1e-12, 0.0, 0, None) == ERR   # not a multiple of 4
        assert lib.imt_layernorm_bwd(dtype, A, B, C, D, A, B, C, D, 3, 1026, 0.0, 0, None, 0.0, 0, None, None) == ERR


def test_optimizer_entry_points_refuse_step_zero_and_misaligned_buffers(lib):
    adam = lambda p, g, m, v, pb, step: lib.imt_clip_adam(p, g, m, v, pb, 4096, None, 1.0, 1.0, 1e-3, 0.9, 0.98, 1e-8, step, 1, None)  # noqa: E731
    assert adam(A, B, C, D, None, 0) == ERR and b"step" in lib.imt_last_error()
    assert adam(A, B, C, D, None, -3) == ERR and b"step" in lib.imt_last_error()
    for bad in range(5):
        ptrs = [A, B, C, D, 0x50000]
        ptrs[bad] += 4 if bad < 4 else 2
        assert adam(*ptrs, 1) == ERR and b"alignment" in lib.imt_last_error(), bad
    assert adam(None, B, C, D, None, 1) == ERR and b"null" in lib.imt_last_error()
    assert lib.imt_sumsq(A + 4, 4096, B, C, None) == ERR and b"alignment" in lib.imt_last_error()
    assert lib.imt_sumsq(A, 4096, None, C, None) == ERR and b"null" in lib.imt_last_error()
    assert lib.imt_clip_scale(A + 8, 4096, B, 1.0, 1.0, None) == ERR and b"alignment" in lib.imt_last_error()
    assert lib.imt_clip_scale(None, 4096, B, 1.0, 1.0, None) == ERR and b"null" in lib.imt_last_error()
    # empty buffers are accepted without a launch
    assert lib.imt_sumsq(A + 4, 0, B, C, None) == 0 and lib.imt_clip_scale(A + 4, 0, B, 1.0, 1.0, None) == 0
    assert adam(A + 4, B, C, D, None, 0) == ERR   # (n > 0: the step check comes before the alignment check)
