"""ImageMassSeq2Seq's image branches without a GPU: the oracle's closed forms against fp64 autograd, the -10000 mask
semantics, negative sampling in the dataset, the C ABI of the contrastive tail and its host-side validation, and the trainer's
refusals."""
import ctypes
import marshal
import os
import random
import re

import pytest
import torch

from imagetranslate_amd import _lib as L
from tests import multimodal_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = -1
NEW = ("imt_attn_pool_plan", "imt_attn_pool_fwd", "imt_attn_pool_bwd", "imt_contrastive")


def _pool_case(rows=4, S=9, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, S, d, generator=g, dtype=torch.float64)
    w = torch.randn(d, generator=g, dtype=torch.float64) * 0.5
    b = torch.randn((), generator=g, dtype=torch.float64)
    lens = [S, 1, 0, 5][:rows]
    mask = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    return x, w, b, mask


# ------------------------------------------------------------------------------------------------ oracle
def test_oracle_pool_gradients_equal_fp64_autograd():
    x, w, b, mask = _pool_case()
    for m in (mask, None):
        xg, wg, bg = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        u, p, norm = M.attn_pool(xg, wg, bg, m)
        du = torch.randn(u.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        (u * du).sum().backward()
        dx, dw, db = M.attn_pool_grads(x, w, m, u.detach(), p.detach(), norm.detach(), du)
        assert torch.allclose(dx, xg.grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(dw, wg.grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(db, bg.grad, rtol=1e-10, atol=1e-12)


def test_oracle_contrastive_gradients_equal_fp64_autograd():
    g = torch.Generator().manual_seed(2)
    B, Nn, d = 5, 30, 16
    img = torch.nn.functional.normalize(torch.randn(B, d, generator=g, dtype=torch.float64), dim=-1).requires_grad_()
    txt = torch.nn.functional.normalize(torch.randn(B + Nn, d, generator=g, dtype=torch.float64), dim=-1).requires_grad_()
    loss = M.contrastive(img, txt)
    loss.backward()
    d_img, d_txt = M.contrastive_grads(img.detach(), txt.detach())
    assert torch.allclose(d_img, img.grad, rtol=1e-10, atol=1e-13)
    assert torch.allclose(d_txt, txt.grad, rtol=1e-10, atol=1e-13)
    # the restatement against the reference's own expression (src/image_model.py:260-263)
    cross = img.detach() @ txt.detach().t()
    want = torch.sum(torch.log(torch.sum(torch.exp(cross), dim=-1) + 1e-4) - (torch.diagonal(cross[:, :B], 0) + 1e-4)) / B
    assert float(loss.detach()) == float(want)


def test_all_masked_row_pools_to_the_uniform_average():
    """masked_fill sets the scores to exactly -10000: a row with every position masked has equal scores, so it pools to the
    plain mean (an additive -10000 penalty would keep the scores' differences)."""
    x, w, b, mask = _pool_case()
    u, p, norm = M.attn_pool(x, w, b, mask)
    assert not bool(mask[2].any())
    assert torch.allclose(p[2], torch.full_like(p[2], 1.0 / x.size(1)), rtol=0, atol=1e-15)
    mean = x[2].mean(0)
    assert torch.allclose(u[2], mean / (mean.norm() + 1e-4), rtol=1e-12, atol=1e-15)
    assert torch.allclose(p[1], torch.eye(x.size(1), dtype=x.dtype)[0], rtol=0, atol=1e-300)  # one real position takes everything
    # and no gradient reaches the scores of masked positions
    du = torch.ones_like(u)
    _, dw, db = M.attn_pool_grads(x[2:3], w, mask[2:3], u[2:3], p[2:3], norm[2:3], du[2:3])
    assert float(dw.abs().max()) == 0.0 and float(db) == 0.0


# ------------------------------------------------------------------------------------------------ dataset
class _TP:
    languages = {"<xa>": 0}

    def pad_token_id(self):
        return 0

    def id2token(self, i):
        return "<xa>"


class _Feats:
    def get(self, paths):
        return torch.zeros(len(paths), 49, 8)


def _caption_file(tmp_path, n_caps, seed=0):
    rng = random.Random(seed)
    caps = sorted([(i % 7, [5] + [rng.randrange(6, 90) for _ in range(rng.randrange(2, 11))] + [4]) for i in range(n_caps)],
                  key=lambda c: len(c[1]))
    path = str(tmp_path / ("caps%d.bin" % n_caps))
    with open(path, "wb") as fw:
        marshal.dump(({i: "img%d.jpg" % i for i in range(7)}, caps), fw)
    return path, caps


@pytest.mark.parametrize("n_caps,max_img", [(12, 4), (50, 8), (90, 40)])
def test_negative_samples_count_padding_and_seed(tmp_path, n_caps, max_img):
    from imagetranslate_amd.dataset import ImageCaptionDataset
    path, caps = _caption_file(tmp_path, n_caps)
    mk = lambda seed, neg=True: ImageCaptionDataset("", path, 50, _TP(), max_img, use_neg_samples=neg, features=_Feats(), neg_seed=seed)
    ds = mk(3)
    all_caps = sorted(tuple(c[1]) for c in caps)
    state = random.getstate()
    items = [ds[i] for i in range(len(ds))]
    assert random.getstate() == state, "the global random state must not be touched"
    for it in items:
        B = it["captions"].size(0)
        neg, neg_mask = it["neg"], it["neg_mask"]
        assert neg.size(0) == min(n_caps, max(30, B))                       # src/dataset.py:392
        assert torch.equal(neg_mask, neg != 0)
        rows = [tuple(r[m].tolist()) for r, m in zip(neg, neg_mask)]
        assert all(bool(m[:int(m.sum())].all()) for m in neg_mask), "padding goes after the caption"
        assert int(neg_mask.sum(1).max()) == neg.size(1)
        # without replacement, from all captions: as a multiset the rows are a sub-multiset of the captions
        pool = list(all_caps)
        for r in rows:
            pool.remove(r)
    again = mk(3)
    for i, it in enumerate(items):
        assert torch.equal(again[i]["neg"], it["neg"])
    if n_caps > 30:
        other = mk(4)
        assert any(not torch.equal(other[i]["neg"], it["neg"]) for i, it in enumerate(items))
    plain = mk(3, neg=False)[0]
    assert "neg" not in plain and "neg_mask" not in plain


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "imt_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(imt_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW:
        assert name in declared, "%s is not declared in include/imt_hip.h" % name
        assert name in L.SIGNATURES, "%s has no binding in _lib.SIGNATURES" % name
        assert hasattr(lib, name), "libimt_hip.so does not export %s" % name
    assert "pool.hip" in open(os.path.join(ROOT, "imagetranslate_amd", "csrc", "Makefile")).read()


def test_pool_plan_reports_the_lds_fit_switch():
    lib = L.load()
    assert lib.imt_attn_pool_plan(0, 37, 128) == 1 and lib.imt_attn_pool_plan(1, 49, 128) == 1
    assert lib.imt_attn_pool_plan(0, 200, 512) == 2 and lib.imt_attn_pool_plan(1, 200, 512) == 2
    # the switch sits where S * d elements stop fitting beside the small arrays in 64 KiB
    small = lambda S, d: 64 + 2 * ((S + 3) // 4 * 4) * 4 + 4096 + 4 * d
    for dtype, size in ((0, 4), (1, 2)):
        d = 512
        S = max(s for s in range(1, 200) if small(s, d) + s * d * size <= 65536)
        assert lib.imt_attn_pool_plan(dtype, S, d) == 1 and lib.imt_attn_pool_plan(dtype, S + 1, d) == 2


def test_host_validation_of_the_contrastive_tail():
    """Every bad argument is refused with IMT_ERR_BAD_ARG before anything is enqueued (no GPU here: a launch would fail)."""
    lib = L.load()
    P = 0x1000  # never dereferenced on the host
    fwd = lambda dtype=0, x=P, w=P, b=P, u=P, probs=P, norm=P, rows=3, S=8, d=128: lib.imt_attn_pool_fwd(
        dtype, x, w, b, None, u, probs, norm, rows, S, d, None)
    bwd = lambda dtype=0, x=P, dx=P, dw=P, db=P, ws=P, du=P, rows=3, S=8, d=128: lib.imt_attn_pool_bwd(
        dtype, x, P, None, P, P, P, du, None, dx, dw, db, ws, rows, S, d, None)
    for call in (fwd, bwd):
        assert call(dtype=7) == ERR and b"dtype" in lib.imt_last_error()
        assert call(S=0) == ERR and b"S must be at least 1" in lib.imt_last_error()
        assert call(S=-3) == ERR
        assert call(S=4097) == ERR and b"not taken" in lib.imt_last_error()
        assert call(d=130) == ERR and b"multiple of 4" in lib.imt_last_error()
        assert call(d=0) == ERR
        assert call(d=1028) == ERR and b"not taken" in lib.imt_last_error()
        assert call(rows=-1) == ERR
        assert call(x=None) == ERR and b"null pointer" in lib.imt_last_error()
        assert call(rows=0) == 0                                      # an empty batch is accepted without a launch
    for name in ("w", "b", "u", "probs", "norm"):
        assert fwd(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name
    for name in ("dx", "dw", "db", "ws", "du"):
        assert bwd(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name
    assert lib.imt_attn_pool_plan(0, 0, 128) == ERR and lib.imt_attn_pool_plan(0, 8, 6) == ERR and lib.imt_attn_pool_plan(3, 8, 8) == ERR
    con = lambda img=P, txt=P, loss=P, d_img=P, d_txt=P, ws=P, B=5, N=35, d=128: lib.imt_contrastive(
        img, txt, loss, d_img, d_txt, ws, B, N, d, None)
    assert con(B=0) == ERR
    assert con(N=4) == ERR and b"fewer text vectors" in lib.imt_last_error()
    assert con(N=4097) == ERR and b"not taken" in lib.imt_last_error()
    assert con(d=126) == ERR and b"multiple of 4" in lib.imt_last_error()
    assert con(d=2048) == ERR
    for name in ("img", "txt", "loss", "d_img", "d_txt", "ws"):
        assert con(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name


def test_wrappers_have_no_cpu_fallback():
    from imagetranslate_amd import hip_ops as O
    with pytest.raises(L.ImtError):
        O.attn_pool_fwd(torch.zeros(2, 3, 8), torch.zeros(8), torch.zeros(1))
    with pytest.raises(L.ImtError):
        O.contrastive(torch.zeros(2, 8), torch.zeros(4, 8))


# ------------------------------------------------------------------------------------------------ trainer
def _options(*argv):
    from imagetranslate_amd.train_image_mt import get_option_parser
    return get_option_parser().parse_args(list(argv))[0]


def test_trainer_refuses_image_dir_without_features(tmp_path):
    from imagetranslate_amd import train_image_mt as T
    assert T.load_image_data(_options("--train", "x"), None) is None      # no --image: no image batches, nothing read
    empty = tmp_path / "images"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="features.pt"):
        T.load_image_data(_options("--image", str(empty), "--train", str(tmp_path / "caps.bin")), None)
    with pytest.raises(FileNotFoundError, match="features.pt"):
        T.load_image_data(_options("--image", str(tmp_path / "missing"), "--train", "x"), None)
    torch.save({"paths": [], "feats": torch.zeros(0, 49, 8)}, str(empty / "features.pt"))
    with pytest.raises(ValueError, match="--train"):
        T.load_image_data(_options("--image", str(empty)), None)


def test_trainer_refuses_back_translation_over_image_batches(tmp_path):
    from imagetranslate_amd import train_image_mt as T
    with pytest.raises(NotImplementedError, match="image batches"):
        T.train(_options("--image", str(tmp_path), "--train", "x", "--langs", "en,fa", "--fstep", "10"))
    with pytest.raises(ValueError, match="--mmode"):
        T.ImageMTTrainer(model=None, mm_mode="both")
