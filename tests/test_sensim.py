"""SenSim without a GPU: the oracle's closed forms against fp64 autograd of the reference's formula, the C ABI of the three new
entry points and their host-side validation, the state-dict keys, save / load, init_from_lm's refusals, the trainer's negative
draw and the command lines."""
import os
import pickle
import re

import pytest
import torch

from imagetranslate_amd import _lib as L
from tests import sensim_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = -1
NEW = ("imt_sensim_loss", "imt_pair_dot", "imt_pair_dot_bwd")
MAX_N, MAX_D = 4096, 1024


# ------------------------------------------------------------------------------------------------ oracle
def _unit(n, d, g):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g, dtype=torch.float64), dim=-1)


@pytest.mark.parametrize("B,nsn,ntn,d", [(1, 0, 0, 4), (5, 30, 17, 16), (3, 0, 7, 8)])
def test_oracle_two_sided_loss_equals_fp64_autograd_of_the_reference_formula(B, nsn, ntn, d):
    g = torch.Generator().manual_seed(B + nsn)
    sneg, src, tneg, tgt = (_unit(n, d, g).requires_grad_() for n in (nsn, B, ntn, B))
    # src/sen_sim.py:94-103 written out
    tcat, scat = torch.cat([tneg, tgt]), torch.cat([sneg, src])
    nominator = torch.sum(src * tgt, dim=-1) + 1e-4
    cross_all = torch.cat([torch.mm(src, tcat.T), torch.mm(tgt, scat.T)], dim=1)
    want = torch.sum(torch.log(torch.sum(torch.exp(cross_all), dim=-1) + 1e-4) - nominator) / len(src)
    want.backward()
    sc, tc, want = scat.detach(), tcat.detach(), want.detach()
    assert float(S.two_sided_loss(sc, tc, B)) == pytest.approx(float(want), rel=1e-14)
    d_scat, d_tcat = S.two_sided_grads(sc, tc, B)
    for got, parts in ((d_scat, (sneg, src)), (d_tcat, (tneg, tgt))):
        assert torch.allclose(got, torch.cat([p.grad for p in parts]), rtol=1e-12, atol=1e-15)
    # the sides are not interchangeable: the negatives of one side score against the other side's sentences
    if nsn != ntn:
        other = S.two_sided_loss(torch.cat([tneg, src]).detach(), torch.cat([sneg, tgt]).detach(), B)
        assert abs(float(other) - float(want)) > 1e-6


def test_oracle_one_sided_loss_and_pair_dots():
    g = torch.Generator().manual_seed(2)
    src, tgt = _unit(6, 12, g), _unit(6, 12, g)
    cross = torch.mm(src, tgt.T)   # :105-108
    want = torch.sum(torch.log(torch.sum(torch.exp(cross), dim=-1) + 1e-4) - (torch.diagonal(cross[:, :], 0) + 1e-4)) / len(cross)
    assert float(S.one_sided_loss(src, tgt)) == pytest.approx(float(want), rel=1e-14)
    from tests.multimodal_oracle import contrastive
    assert float(contrastive(src, tgt)) == pytest.approx(float(want), rel=1e-14), "imt_contrastive's formula with N = B"
    a, b = src.clone().requires_grad_(), tgt.clone().requires_grad_()
    gup = torch.randn(6, generator=g, dtype=torch.float64)
    out = S.pair_dot(a, b)
    assert torch.allclose(out, torch.sum(src * tgt, dim=-1), rtol=0, atol=1e-16)
    (out * gup).sum().backward()
    da, db = S.pair_dot_grads(src, tgt, gup)
    assert torch.allclose(da, a.grad, rtol=1e-14, atol=0) and torch.allclose(db, b.grad, rtol=1e-14, atol=0)


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


def test_argument_validation_without_gpu():
    """Every refused case is answered with IMT_ERR_BAD_ARG before anything is enqueued (no GPU here: a launch would fail)."""
    lib = L.load()
    P = 0x1000  # never dereferenced on the host
    loss = lambda scat=P, tcat=P, out=P, d_scat=P, d_tcat=P, ws=P, B=4, Ns=10, Nt=8, d=128: lib.imt_sensim_loss(
        scat, tcat, out, d_scat, d_tcat, ws, B, Ns, Nt, d, None)
    assert loss(B=0) == ERR and b"B must be at least 1" in lib.imt_last_error()
    assert loss(B=-1) == ERR
    assert loss(Ns=3) == ERR and b"fewer vectors" in lib.imt_last_error()
    assert loss(Nt=3) == ERR and b"fewer vectors" in lib.imt_last_error()
    assert loss(Ns=MAX_N + 1) == ERR and b"not taken" in lib.imt_last_error()
    assert loss(Nt=MAX_N + 1) == ERR and b"not taken" in lib.imt_last_error()
    assert loss(d=130) == ERR and b"multiple of 4" in lib.imt_last_error()
    assert loss(d=0) == ERR and loss(d=-4) == ERR
    assert loss(d=MAX_D + 4) == ERR and b"not taken" in lib.imt_last_error()
    for name in ("scat", "tcat", "out", "d_scat", "d_tcat", "ws"):
        assert loss(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name
    dot = lambda a=P, b=P, out=P, rows=3, d=128: lib.imt_pair_dot(a, b, out, rows, d, None)
    bwd = lambda a=P, b=P, g=P, da=P, db=P, rows=3, d=128: lib.imt_pair_dot_bwd(a, b, g, da, db, rows, d, None)
    for call in (dot, bwd):
        assert call(d=130) == ERR and b"multiple of 4" in lib.imt_last_error()
        assert call(d=0) == ERR
        assert call(d=MAX_D + 4) == ERR and b"not taken" in lib.imt_last_error()
        assert call(rows=-1) == ERR
        assert call(a=None) == ERR and b"null pointer" in lib.imt_last_error()
        assert call(rows=0) == 0                                      # an empty batch is accepted without a launch
        assert call(rows=0, a=None) == 0
    for name in ("b", "out"):
        assert dot(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name
    for name in ("b", "g", "da", "db"):
        assert bwd(**{name: None}) == ERR and b"null pointer" in lib.imt_last_error(), name


def test_wrappers_have_no_cpu_fallback():
    from imagetranslate_amd import hip_ops as O
    with pytest.raises(L.ImtError):
        O.sensim_loss(torch.zeros(3, 8), torch.zeros(2, 8), 2)
    with pytest.raises(L.ImtError):
        O.pair_dot(torch.zeros(2, 8), torch.zeros(2, 8))
    with pytest.raises(L.ImtError):
        O.pair_dot_bwd(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2))


# ------------------------------------------------------------------------------------------------ the model
def _toy(seed=0, **kw):
    from imagetranslate_amd.sen_sim import SenSim
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    torch.manual_seed(seed)
    tp = SyntheticTextProcessor(300)
    return tp, SenSim(tp, enc_layer=2, embed_dim=128, intermediate_dim=256, **kw)


def test_state_dict_keys_and_shapes_are_the_oracles():
    tp, model = _toy(num_attention_heads=4)
    sd = model.state_dict()
    ref = S.SenSim(tp, enc_layer=2, embed_dim=128, intermediate_dim=256, num_attention_heads=4)
    assert list(sd.keys()) == list(ref.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert all(k.startswith("encoder.") or k in ("input_attention.weight", "input_attention.bias") for k in sd)
    assert tuple(sd["input_attention.weight"].shape) == (1, 128) and tuple(sd["input_attention.bias"].shape) == (1,)
    assert tuple(sd["encoder.embeddings.token_type_embeddings.weight"].shape) == (len(tp.languages), 128)
    assert {id(p) for p in model.flat_param_order()} == {id(p) for p in model.parameters()}
    from imagetranslate_amd.sen_sim import SenSim
    assert model.config.num_attention_heads == 4
    assert SenSim(tp, enc_layer=1, embed_dim=96, intermediate_dim=192).config.num_attention_heads == 12   # the reference's
    with pytest.raises(ValueError):
        model.set_compute_dtype(torch.float64)
    assert model.set_compute_dtype("bf16")._imt_compute_dtype == torch.bfloat16


def test_save_load_round_trip(tmp_path):
    from imagetranslate_amd.sen_sim import SenSim
    tp, model = _toy(num_attention_heads=4)
    out = str(tmp_path / "sim")
    model.save(out)
    with open(os.path.join(out, "mt_config"), "rb") as fp:
        assert pickle.load(fp) == (2, 128, 256)                        # the reference's 3-tuple, nothing else in it
    assert sorted(os.listdir(out)) == ["imt_config.json", "mt_config", "mt_model.state_dict"]
    again, tp2 = SenSim.load(out, None, text_processor=tp)
    again = again.cpu()
    assert tp2 is tp and again.config.num_attention_heads == 4
    assert (again.enc_layer, again.embed_dim, again.intermediate_dim) == (2, 128, 256)
    a, b = model.state_dict(), again.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # anything but three plain integers is refused, and nothing in the file is executed
    with open(os.path.join(out, "mt_config"), "wb") as fp:
        pickle.dump((1, 96, os.getcwd), fp)
    with pytest.raises(pickle.UnpicklingError):
        SenSim.load(out, None, text_processor=tp)


def test_init_from_lm_copies_a_matching_encoder_and_refuses_another():
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    tp, model = _toy(num_attention_heads=4)
    kw = dict(lang_dec=False, dec_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4)
    torch.manual_seed(5)
    lm = Seq2Seq(tp, enc_layer=2, **kw)
    pool_w = model.input_attention.weight.detach().clone()
    encoder = model.encoder
    assert not torch.equal(model.encoder.embeddings.word_embeddings.weight, lm.encoder.embeddings.word_embeddings.weight)
    model.init_from_lm(lm)
    assert model.encoder is encoder and model.encoder is not lm.encoder, "the weights are copied, the module is not rebound"
    theirs = lm.encoder.state_dict()
    assert all(torch.equal(v, theirs[k]) for k, v in model.encoder.state_dict().items())
    assert torch.equal(model.input_attention.weight, pool_w)
    for bad in (Seq2Seq(tp, enc_layer=1, **kw), Seq2Seq(tp, enc_layer=2, **dict(kw, intermediate_dim=128)),
                Seq2Seq(tp, enc_layer=2, **dict(kw, num_attention_heads=8)),
                Seq2Seq(SyntheticTextProcessor(301), enc_layer=2, **kw)):
        with pytest.raises(ValueError, match="init_from_lm"):
            model.init_from_lm(bad)

    class _OneMoreLanguage(SyntheticTextProcessor):
        def __init__(self, n):
            super().__init__(n)
            self.languages = dict(self.languages, **{"<zz>": len(self.languages)})
    with pytest.raises(ValueError, match="token_type_embeddings"):
        model.init_from_lm(Seq2Seq(_OneMoreLanguage(300), enc_layer=2, **kw))
    assert all(torch.equal(v, theirs[k]) for k, v in model.encoder.state_dict().items()), "a refusal leaves the weights alone"


def test_forward_refuses_the_cpu():
    tp, model = _toy(num_attention_heads=4)
    src = torch.randint(6, 300, (2, 5))
    langs = torch.zeros(2, dtype=torch.long)
    with pytest.raises(L.ImtError):
        model(src, src != 0, langs, src, src != 0, langs)


# ------------------------------------------------------------------------------------------------ trainer
def test_negative_draw_is_reproducible_and_differs_between_steps():
    from imagetranslate_amd.train_txt_sim import draw_negative
    n = 1000
    a = [[draw_negative(7, step, side, n) for step in range(50)] for side in (0, 1)]
    b = [[draw_negative(7, step, side, n) for step in reversed(range(50))][::-1] for side in (0, 1)]
    assert a == b, "the draw depends on (seed, step, side) alone"
    assert all(0 <= v < n for row in a for v in row)
    assert len(set(a[0])) > 40 and len(set(a[1])) > 40, "steps draw different batches"
    assert a[0] != a[1], "the two sides draw independently"
    assert [draw_negative(8, step, 0, n) for step in range(50)] != a[0], "another seed, other draws"
    assert all(draw_negative(7, step, 0, 1) == 0 for step in range(5))


def test_command_lines_parse_and_off_path_flags_are_refused(monkeypatch):
    from imagetranslate_amd import train_txt_sim as T
    from imagetranslate_amd.option_parser import get_img_options_parser
    argv = ["--tok", "tok", "--train_mt", "train.mt", "--dev_mt", "dev.mt", "--src-neg", "neg.src", "--dst-neg", "neg.dst", "--model", "out",
            "--enc", "4", "--embed", "512", "--intermediate", "1024", "--lr", "0.0002", "--warmup", "4000", "--step", "1000",
            "--batch", "4000", "--capacity", "100", "--beam", "4", "--output", "sims.txt"]
    o, rest = get_img_options_parser().parse_args(argv)
    assert not rest and (o.mt_train_path, o.mt_dev_path, o.src_neg, o.dst_neg, o.model_path, o.output) == \
        ("train.mt", "dev.mt", "neg.src", "neg.dst", "out", "sims.txt")
    for flag in (["--dict", "d"], ["--cont"], ["--save-opt"], ["--lm", "x"]):
        bad = get_img_options_parser().parse_args(argv + flag)[0]
        with pytest.raises(NotImplementedError):
            T.SenSimTrainer.train(bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one process"):
        T.SenSimTrainer.train(o)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(NotImplementedError, match="one process"):
        T.SenSimTrainer(model=None, world_size=2)
    with pytest.raises(ValueError, match="--src-neg"):
        T.SenSimTrainer.train(get_img_options_parser().parse_args(["--tok", "tok", "--train_mt", "x"])[0])
