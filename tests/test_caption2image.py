"""Caption2Image without a GPU: the oracle's closed forms against fp64 autograd, the C ABI of the three new entry points and
their host-side validation, the state-dict keys, save / load, the two command lines and the three hops of translate_batch."""
import os
import pickle
import re

import pytest
import torch

from imagetranslate_amd import _lib as L
from tests import caption2image_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = -1
NEW = ("imt_sent_pool_fwd", "imt_sent_pool_bwd", "imt_l2_dist")


# ------------------------------------------------------------------------------------------------ oracle
def _pool_case(rows=4, S=9, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, S, d, generator=g, dtype=torch.float64)
    w = torch.randn(d, generator=g, dtype=torch.float64) * 0.5
    b = torch.randn((), generator=g, dtype=torch.float64)
    mask = torch.arange(S)[None, :] < torch.tensor([S, 1, 0, 5][:rows])[:, None]
    keep = torch.rand(rows, S, d, generator=g) >= 0.3
    return x, w, b, mask, keep


@pytest.mark.parametrize("drop", [False, True])
def test_oracle_pool_gradients_equal_fp64_autograd(drop):
    x, w, b, mask, keep = _pool_case()
    keep, p = (keep, 0.3) if drop else (None, 0.0)
    for m in (mask, None):
        xg, wg, bg = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        v, probs = C.sent_pool(xg, wg, bg, m, keep, p)
        dv = torch.randn(v.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        (v * dv).sum().backward()
        dx, dw, db = C.sent_pool_grads(x, w, m, probs.detach(), dv, keep, p)
        assert torch.allclose(dx, xg.grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(dw, wg.grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(db, bg.grad, rtol=1e-10, atol=1e-12)
        if drop:
            assert float(dx[~keep].abs().max()) == 0.0, "no gradient reaches a dropped element"


def test_oracle_pool_restates_the_reference_expressions():
    """src/image_model.py:430-436 written out: F.dropout's scaling, Linear + squeeze, masked_fill_, Softmax(dim=1), einsum."""
    x, w, b, mask, keep = _pool_case()
    xd = x * keep / (1 - 0.3)
    scores = torch.nn.functional.linear(xd, w[None, :], b[None]).squeeze(-1)
    scores.masked_fill_(~mask, -10000.0)
    want = torch.einsum("bfd,bf->bd", xd, torch.nn.Softmax(dim=1)(scores))
    v, probs = C.sent_pool(x, w, b, mask, keep, 0.3)
    assert torch.allclose(v, want, rtol=1e-13, atol=1e-15)
    # an all-masked row pools to the plain average of the (dropped) row, a single real position takes everything
    assert torch.allclose(probs[2], torch.full_like(probs[2], 1.0 / x.size(1)), rtol=0, atol=1e-15)
    assert torch.allclose(v[2], xd[2].mean(0), rtol=1e-12, atol=1e-15)
    assert torch.allclose(v[1], xd[1, 0], rtol=0, atol=1e-300)


def test_oracle_l2_gradient_equals_fp64_autograd():
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(5, 49 * 8, generator=g, dtype=torch.float64).requires_grad_()
    target = torch.randn(5, 49 * 8, generator=g, dtype=torch.float64)
    loss = C.l2_dist(pred, target)
    assert float(loss.detach()) == pytest.approx(float(((pred.detach() - target) ** 2).sum().sqrt() / 5), rel=1e-14)
    loss.backward()
    assert torch.allclose(C.l2_dist_grad(pred.detach(), target), pred.grad, rtol=1e-12, atol=1e-15)
    same = target.clone().requires_grad_()
    C.l2_dist(same, target).backward()
    assert float(same.grad.abs().max()) == 0.0 and float(C.l2_dist_grad(target, target).abs().max()) == 0.0


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


def test_host_validation_of_the_caption2image_tail():
    """Every bad argument is refused with IMT_ERR_BAD_ARG before anything is enqueued (no GPU here: a launch would fail)."""
    lib = L.load()
    P = 0x1000  # never dereferenced on the host
    fwd = lambda dtype=0, x=P, w=P, b=P, v=P, probs=P, rows=3, S=8, d=128, p=0.1: lib.imt_sent_pool_fwd(
        dtype, x, w, b, None, v, probs, rows, S, d, p, 7, None)
    bwd = lambda dtype=0, x=P, w=P, probs=P, dv=P, dx=P, dw=P, db=P, ws=P, rows=3, S=8, d=128, p=0.1: lib.imt_sent_pool_bwd(
        dtype, x, w, None, probs, dv, dx, dw, db, ws, rows, S, d, p, 7, None)
    for call in (fwd, bwd):
        assert call(dtype=7) == ERR and b"dtype" in lib.imt_last_error()
        assert call(S=0) == ERR and b"S must be at least 1" in lib.imt_last_error()
        assert call(S=-3) == ERR
        assert call(S=4097) == ERR and b"not taken" in lib.imt_last_error()
        assert call(d=130) == ERR and b"multiple of 4" in lib.imt_last_error()
        assert call(d=0) == ERR
        assert call(d=1028) == ERR and b"not taken" in lib.imt_last_error()
        assert call(p=1.0) == ERR and b"dropout_p" in lib.imt_last_error()
        assert call(p=-0.1) == ERR and b"dropout_p" in lib.imt_last_error()
        assert call(p=float("nan")) == ERR
        assert call(rows=-1) == ERR
        assert call(x=None) == ERR and b"null pointer" in lib.imt_last_error()
        assert call(rows=0) == 0                                      # an empty batch is accepted without a launch
        assert call(rows=0, x=None) == 0
    for name in ("w", "b", "v", "probs"):
        assert fwd(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name
    for name in ("w", "probs", "dv", "dx", "dw", "db", "ws"):
        assert bwd(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name
    l2 = lambda dtype=0, pred=P, target=P, loss=P, dpred=P, ws=P, B=5, n=49 * 128: lib.imt_l2_dist(
        dtype, pred, target, loss, dpred, ws, B, n, None)
    assert l2(dtype=2) == ERR and b"dtype" in lib.imt_last_error()
    assert l2(B=0) == ERR and b"B must be at least 1" in lib.imt_last_error()
    assert l2(B=-2) == ERR
    assert l2(n=49 * 128 + 2) == ERR and b"multiple of 4" in lib.imt_last_error()
    assert l2(n=0) == ERR and l2(n=-4) == ERR
    for name in ("pred", "target", "loss", "dpred", "ws"):
        assert l2(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name


def test_wrappers_have_no_cpu_fallback():
    from imagetranslate_amd import hip_ops as O
    with pytest.raises(L.ImtError):
        O.sent_pool_fwd(torch.zeros(2, 3, 8), torch.zeros(8), torch.zeros(1))
    with pytest.raises(L.ImtError):
        O.sent_pool_bwd(torch.zeros(2, 3, 8), torch.zeros(8), None, torch.zeros(2, 3), torch.zeros(2, 8), torch.zeros(8), torch.zeros(1))
    with pytest.raises(L.ImtError):
        O.l2_dist(torch.zeros(2, 8), torch.zeros(2, 8))


# ------------------------------------------------------------------------------------------------ the model
def _toy(seed=0, **kw):
    from imagetranslate_amd.image_model import Caption2Image
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    torch.manual_seed(seed)
    tp = SyntheticTextProcessor(300)
    return tp, Caption2Image(tp, enc_layer=2, embed_dim=128, intermediate_dim=256, **kw)


def _layer_keys(i):
    pre = "encoder.encoder.layer.%d." % i
    names = ["attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
             "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"]
    return [pre + n + s for n in names for s in (".weight", ".bias")]


EXPECTED_KEYS = (["encoder.embeddings.word_embeddings.weight", "encoder.embeddings.position_embeddings.weight",
                  "encoder.embeddings.token_type_embeddings.weight", "encoder.embeddings.LayerNorm.weight",
                  "encoder.embeddings.LayerNorm.bias"] + _layer_keys(0) + _layer_keys(1)
                 + ["input_attention.weight", "input_attention.bias", "decoder.weight", "decoder.bias"])


def test_state_dict_keys_and_shapes_are_the_references():
    tp, model = _toy(num_attention_heads=4)
    sd = model.state_dict()
    assert list(sd.keys()) == EXPECTED_KEYS
    d = 128
    assert tuple(sd["input_attention.weight"].shape) == (1, d) and tuple(sd["input_attention.bias"].shape) == (1,)
    assert tuple(sd["decoder.weight"].shape) == (49 * d, d) and tuple(sd["decoder.bias"].shape) == (49 * d,)
    assert tuple(sd["encoder.embeddings.token_type_embeddings.weight"].shape) == (len(tp.languages), d)
    # the restatement the GPU tests compare against has the same keys and shapes
    ref = C.Caption2Image(tp, enc_layer=2, embed_dim=128, intermediate_dim=256, num_attention_heads=4)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    from imagetranslate_amd.image_model import Caption2Image
    assert model.config.num_attention_heads == 4
    assert Caption2Image(tp, enc_layer=1, embed_dim=96, intermediate_dim=192).config.num_attention_heads == 12   # the reference's
    with pytest.raises(ValueError):
        model.set_compute_dtype(torch.float64)
    assert model.set_compute_dtype("bf16")._imt_compute_dtype == torch.bfloat16


def test_save_load_round_trip_and_reference_config(tmp_path):
    from imagetranslate_amd.image_model import Caption2Image
    tp, model = _toy(num_attention_heads=4)
    out = str(tmp_path / "c2i")
    model.save(out)
    with open(os.path.join(out, "mt_config"), "rb") as fp:
        assert pickle.load(fp) == (2, 128, 256)                        # the reference's 3-tuple, nothing else in it
    again = Caption2Image.load(out, None, text_processor=tp).cpu()
    assert again.config.num_attention_heads == 4 and (again.enc_layer, again.embed_dim, again.intermediate_dim) == (2, 128, 256)
    a, b = model.state_dict(), again.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # a directory as the reference writes it: the 3-tuple and the weights only -> the reference's 12 heads
    ref_dir = str(tmp_path / "ref")
    os.makedirs(ref_dir)
    with open(os.path.join(ref_dir, "mt_config"), "wb") as fp:
        pickle.dump((1, 96, 192), fp)
    torch.manual_seed(1)
    donor = Caption2Image(tp, enc_layer=1, embed_dim=96, intermediate_dim=192)
    torch.save(donor.state_dict(), os.path.join(ref_dir, "mt_model.state_dict"))
    loaded = Caption2Image.load(ref_dir, None, text_processor=tp).cpu()
    assert loaded.config.num_attention_heads == 12 and len(loaded.encoder.encoder.layer) == 1
    assert all(torch.equal(v, loaded.state_dict()[k]) for k, v in donor.state_dict().items())
    # anything but three plain integers is refused, and nothing in the file is executed
    with open(os.path.join(ref_dir, "mt_config"), "wb") as fp:
        pickle.dump((1, 96, 192, 4), fp)
    with pytest.raises(ValueError, match="3-tuple"):
        Caption2Image.load(ref_dir, None, text_processor=tp)
    with open(os.path.join(ref_dir, "mt_config"), "wb") as fp:
        pickle.dump((1, 96, os.getcwd), fp)
    with pytest.raises(pickle.UnpicklingError):
        Caption2Image.load(ref_dir, None, text_processor=tp)


def test_forward_refuses_the_cpu():
    tp, model = _toy(num_attention_heads=4)
    src = torch.randint(6, 300, (2, 5))
    with pytest.raises(L.ImtError):
        model(src, src != 0, torch.zeros(2, dtype=torch.long))


# ------------------------------------------------------------------------------------------------ command lines
def test_both_option_parsers_accept_the_reference_command_lines():
    from imagetranslate_amd import train_txt2image, translate_img
    from imagetranslate_amd.option_parser import get_img_options_parser
    argv = ["--tok", "tok", "--pretrained", "captioner", "--train", "train.bin", "--dev", "dev.bin", "--image", "images",
            "--model", "out", "--enc", "4", "--embed", "512", "--intermediate", "1024", "--lr", "0.0002", "--warmup", "4000",
            "--clip", "1", "--step", "1000", "--img_capacity", "60", "--max-image", "16", "--fp16", "--beam", "4",
            "--max_len_a", "1.1", "--max_len_b", "5", "--len-penalty", "0.8", "--mask", "0.3", "--mmode", "mixed"]
    o, rest = get_img_options_parser().parse_args(argv)
    assert not rest and (o.tokenizer_path, o.pretrained_path, o.train_path, o.dev_path, o.image_dir, o.model_path) == \
        ("tok", "captioner", "train.bin", "dev.bin", "images", "out")
    assert (o.encoder_layer, o.embed_dim, o.intermediate_layer_dim, o.learning_rate, o.warmup, o.clip, o.step) == \
        (4, 512, 1024, 0.0002, 4000, 1, 1000)
    assert (o.img_capacity, o.max_image, o.fp16, o.fp32, o.heads, o.seed) == (60, 16, True, False, 12, 1234)
    # the flags whose feature is not built are refused by this trainer too, before anything is loaded
    for flag in (["--dict", "d"], ["--cont"], ["--save-opt"], ["--lm", "x"]):
        bad = get_img_options_parser().parse_args(argv + flag)[0]
        with pytest.raises(NotImplementedError):
            train_txt2image.Caption2ImageTrainer.train(bad)
    with pytest.raises(ValueError, match="--pretrained"):
        train_txt2image.Caption2ImageTrainer.train(get_img_options_parser().parse_args(["--tok", "tok"])[0])
    argv = ["--input", "in.txt", "--src", "en", "--target", "fa", "--output", "out.txt", "--batch", "256", "--tok", "tok",
            "--cache_size", "100", "--model", "c2i", "--caption-model", "captioner", "--verbose", "--beam", "3", "--max_len_a", "1.2",
            "--max_len_b", "4", "--len-penalty", "0.7", "--capacity", "120", "--fp16"]
    o, rest = translate_img.get_lm_option_parser().parse_args(argv)
    assert not rest and (o.input_path, o.src_lang, o.target_lang, o.output_path, o.batch, o.tokenizer_path, o.cache_size) == \
        ("in.txt", "en", "fa", "out.txt", 256, "tok", 100)
    assert (o.model_path, o.caption_model_path, o.verbose, o.beam_width, o.max_len_a, o.max_len_b, o.len_penalty_ratio) == \
        ("c2i", "captioner", True, 3, 1.2, 4, 0.7)
    assert (o.total_capacity, o.fp16) == (120, True)
    d = translate_img.get_lm_option_parser().parse_args([])[0]
    assert (d.batch, d.cache_size, d.beam_width, d.max_len_a, d.max_len_b, d.len_penalty_ratio, d.total_capacity, d.verbose) == \
        (512, 300, 4, 1.3, 5, 0.8, 150, False)


# ------------------------------------------------------------------------------------------------ the three hops
class _Tok:
    def decode(self, ids):
        return " ".join("t%d" % int(i) for i in ids)


class _TP:
    tokenizer = _Tok()

    def pad_token_id(self):
        return 0

    def sep_token_id(self):
        return 4


class _Txt2Img:
    """Records its inputs; the 'embedding' of a sentence carries the sum of its token ids."""

    def __init__(self):
        self.calls = []

    def __call__(self, inputs, mask, langs):
        self.calls.append((inputs.clone(), mask.clone(), langs.clone()))
        return (inputs * mask).sum(1, keepdim=True).float().expand(-1, 49 * 4).contiguous()


class _Generator:
    max_len_a, max_len_b = 1.3, 5

    def __init__(self, outs):
        self.outs, self.calls = list(outs), []

    def __call__(self, **kw):
        self.calls.append(kw)
        return self.outs[len(self.calls) - 1]


def _mt_batch():
    src = torch.tensor([[5, 11, 12, 13, 4], [5, 21, 4, 0, 0]])
    return {"src_texts": src.unsqueeze(0), "src_pad_mask": (src != 0).unsqueeze(0), "dst_texts": torch.tensor([[6], [6]]).unsqueeze(0),
            "src_langs": torch.tensor([[0, 0]]), "dst_langs": torch.tensor([[1, 1]]), "pad_idx": torch.tensor([[5, 3]])}


@pytest.mark.parametrize("verbose", [False, True])
def test_translate_batch_runs_three_hops_each_fed_the_previous_output(verbose):
    from imagetranslate_amd import translate_img as T
    hop1 = [torch.tensor([6, 31, 32, 4]), torch.tensor([6, 41])]
    hop2 = [torch.tensor([5, 51]), torch.tensor([5, 61, 62, 63, 4])]
    hop3 = [torch.tensor([6, 71, 4]), torch.tensor([6, 81, 82])]
    gen, t2i = _Generator([hop1, hop2, hop3]), _Txt2Img()
    batch = _mt_batch()
    src = batch["src_texts"][0]
    out = T.translate_batch(batch, t2i, gen, _TP(), verbose=verbose)
    assert len(gen.calls) == 3 and len(t2i.calls) == 3
    want_len = min(int(1.3 * 5 + 5), 512)
    firsts = [torch.tensor([6, 6]), src[:, 0], torch.tensor([6, 6])]
    langs = [torch.tensor([1, 1]), torch.tensor([0, 0]), torch.tensor([1, 1])]
    fed = [(src, src != 0, torch.tensor([0, 0])),
           (torch.tensor([[6, 31, 32, 4], [6, 41, 0, 0]]), None, torch.tensor([1, 1])),
           (torch.tensor([[5, 51, 0, 0, 0], [5, 61, 62, 63, 4]]), None, torch.tensor([0, 0]))]
    for k, call in enumerate(gen.calls):
        assert set(call) == {"first_tokens", "max_len", "tgt_langs", "image_embed", "pad_idx"}
        assert torch.equal(call["first_tokens"], firsts[k]) and torch.equal(call["tgt_langs"], langs[k]), k
        assert call["max_len"] == want_len and call["pad_idx"] == 0
        inputs, mask, in_langs = t2i.calls[k]
        assert torch.equal(inputs, fed[k][0]) and torch.equal(mask, inputs != 0) and torch.equal(in_langs, fed[k][2]), k
        assert tuple(call["image_embed"].shape) == (2, 49, 4)
        assert torch.equal(call["image_embed"][:, 0, 0], inputs.sum(1).float()), "hop %d decodes the embedding of its own input" % k
    mt, src_text, second, third = out
    assert mt == ["t31 t32 t4", "t41"] and second == ["t51", "t61 t62 t63 t4"] and third == ["t71 t4", "t81 t82"]
    if verbose:
        assert src_text == ["t11 t12 t13", "t21"]                     # cut before </s>, language tag removed
        assert T.format_outputs(*out, verbose=True) == ("t11 t12 t13\nt31 t32 t4\nt51\nt71 t4\n****\n"
                                                        "t21\nt41\nt61 t62 t63 t4\nt81 t82\n****\n")
    else:
        assert src_text is None and T.format_outputs(*out, verbose=False) == "t31 t32 t4\nt41\n"


def test_translate_batch_caps_max_len_at_512():
    from imagetranslate_amd import translate_img as T
    src = torch.full((1, 450), 9)
    batch = {"src_texts": src.unsqueeze(0), "src_pad_mask": (src != 0).unsqueeze(0), "dst_texts": torch.tensor([[[6]]]),
             "src_langs": torch.tensor([[0]]), "dst_langs": torch.tensor([[1]]), "pad_idx": torch.tensor([[449]])}
    gen = _Generator([[torch.tensor([6, 7])]] * 3)
    T.translate_batch(batch, _Txt2Img(), gen, _TP())
    assert [c["max_len"] for c in gen.calls] == [512] * 3
