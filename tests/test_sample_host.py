"""Host side of sampled decoding, WITHOUT a GPU: the layout of imt_sample_args, every refusal of imt_sample_step before a
launch, the fp64 oracle of the step (tests/sample_oracle.py) on its own, and the new flags of the entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

from imagetranslate_amd import _lib as L
from tests.sample_oracle import kept_mask, sample_step_reference

ERR = -1
FREQ_LOGITS = [2.0, 1.0, 0.5, 0.0, -0.5, -1.0, -2.0, -3.0]
FREQ_CASES = [(0.7, 5, 11), (1.0, 0, 12), (1.5, 3, 13)]  # (temperature, topk, seed)
FREQ_ROWS, FREQ_CAP = 32768, 0.01


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_sample_args_layout(lib):
    assert lib.imt_abi_sizeof(b"imt_sample_args") == ctypes.sizeof(L.SampleArgs)
    assert "imt_sample_args" in L.ABI_STRUCTS and "imt_sample_step" in L.SIGNATURES


def _sample_args(**kw):
    """A well-formed imt_sample_args (pointers are never dereferenced on the host) with the given fields replaced."""
    a = L.SampleArgs()
    a.B, a.n, a.rep, a.V, a.step, a.t_max = 2, 4, 4, 100, 3, 8
    a.ld, a.temperature, a.topk, a.seed, a.pad_idx, a.eos = 104, 1.0, 0, 7, 0, 4
    for i, (f, t) in enumerate(L.SampleArgs._fields_):
        if t is ctypes.c_void_p:
            setattr(a, f, 0x10000 * (i + 1))
    for f, v in kw.items():
        setattr(a, f, v)
    return a


def test_sample_step_argument_checks(lib):
    bad = lambda **kw: lib.imt_sample_step(ctypes.byref(_sample_args(**kw)), None)
    assert lib.imt_sample_step(None, None) == ERR and b"null args" in lib.imt_last_error()
    assert bad(B=0) == ERR
    for n in (0, 33):
        assert bad(n=n, rep=n) == ERR and b"out of range" in lib.imt_last_error(), n
    for rep in (0, 2, 3, 5):
        assert bad(rep=rep) == ERR and b"rep must be" in lib.imt_last_error(), rep
    assert bad(step=2, rep=1) == ERR and b"first step" in lib.imt_last_error()      # rep == 1 at step > 1
    assert bad(step=0) == ERR and b"outside" in lib.imt_last_error()
    for step in (8, 9):                                                             # step >= t_max
        assert bad(step=step) == ERR and b"outside" in lib.imt_last_error(), step
    for t in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert bad(temperature=t) == ERR and b"temperature" in lib.imt_last_error(), t
    assert bad(B=1 << 16, n=32, rep=32, V=2048) == ERR and b"2^32" in lib.imt_last_error()  # B*n*V == 2^32
    assert bad(B=1 << 20, n=32, rep=32, V=30000) == ERR and b"2^32" in lib.imt_last_error()
    assert bad(ld=99) == ERR and b"ld" in lib.imt_last_error()
    for f in ("logits", "scores_in", "eos_in", "max_lens", "hist_in"):
        assert bad(**{f: None}) == ERR and b"null input" in lib.imt_last_error(), f
    for f in ("scores_out", "eos_out", "hist_out", "parent_out", "tokens_out"):
        assert bad(**{f: None}) == ERR and b"null output" in lib.imt_last_error(), f
    for f in ("slots_in", "slots_out"):                                             # exactly one of the slot tables
        assert bad(**{f: None}) == ERR and b"slots_in/slots_out" in lib.imt_last_error(), f


def _plain_step(logits, n, rep, step, temperature, topk, seed, t_max=4):
    """The oracle on ``logits`` [B*rep, V] with nothing masked and an empty history."""
    rows, V = logits.shape
    B = rows // rep
    z = lambda *s, dtype: torch.zeros(*s, dtype=dtype)
    return sample_step_reference(logits, z(rows, dtype=torch.float32), z(rows, dtype=torch.uint8),
                                 torch.full((B,), 100, dtype=torch.int64), z(rows, t_max, dtype=torch.int64),
                                 z(rows, t_max, dtype=torch.int32), step, B, n, rep, V, t_max, temperature, topk, seed, pad=0, eos=V + 7)


def test_oracle_topk_one_is_the_argmax_with_lowest_index_on_ties():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 50, generator=g)
    x[::2, 40] = x[::2].max(dim=1).values  # a second maximum at a HIGHER index in every other row: never chosen unless it is first
    x[1::4, 3] = 9.0
    x[1::4, 17] = 9.0                      # two equal maxima: index 3 wins
    ref = _plain_step(x, n=4, rep=4, step=2, temperature=0.6, topk=1, seed=5)
    want = torch.from_numpy(np.argmax(x.numpy(), axis=1))  # numpy: the first maximum
    assert torch.equal(ref["tokens"], want)
    assert bool((ref["tokens"][1::4] == 3).all())
    assert kept_mask(x.numpy(), 1).sum(axis=1).tolist() == [1] * 64
    lp = torch.log_softmax(x.double(), -1)[torch.arange(64), want]
    assert float((ref["scores"] - lp).abs().max()) < 1e-12  # the model's log-probability, not the filtered one (which is 0)


def freq_case(temperature, topk, seed):
    """(logits [FREQ_ROWS, 8], n, rep, step, expected frequencies, kept indices) of one frequency case."""
    x = torch.tensor(FREQ_LOGITS, dtype=torch.float32)
    kept = list(range(len(FREQ_LOGITS) if topk <= 0 else topk))  # the logits are strictly decreasing
    p = torch.zeros(len(FREQ_LOGITS), dtype=torch.float64)
    p[kept] = torch.softmax(x.double()[kept] / temperature, 0)
    return x.repeat(FREQ_ROWS, 1), 16, 16, 2, p, kept


@pytest.mark.parametrize("temperature,topk,seed", FREQ_CASES)
def test_oracle_frequencies(temperature, topk, seed):
    logits, n, rep, step, p, kept = freq_case(temperature, topk, seed)
    ref = _plain_step(logits, n, rep, step, temperature, topk, seed)
    freq = torch.bincount(ref["tokens"], minlength=len(FREQ_LOGITS)).double() / FREQ_ROWS
    dev = float((freq - p).abs().max())
    print("T %.1f topk %d seed %d: largest deviation %.4f" % (temperature, topk, seed, dev))
    assert set(ref["tokens"].tolist()) <= set(kept), "a draw outside the kept set"
    assert dev <= FREQ_CAP, dev


def test_new_flags_parse():
    from imagetranslate_amd import caption, train_image_mt, translate
    from imagetranslate_amd.option_parser import get_img_options_parser
    argv = ["--sampling", "--sampling-topk", "10", "--temperature", "0.8", "--nsamples", "3", "--seed", "5"]
    for parser in (translate.get_option_parser(), caption.get_lm_option_parser()):
        o, rest = parser.parse_args(argv)
        assert not rest and o.sampling is True
        assert (o.sampling_topk, o.nsamples, o.seed) == (10, 3, 5) and math.isclose(o.temperature, 0.8)
        d = parser.parse_args([])[0]
        assert (d.sampling, d.sampling_topk, d.temperature, d.nsamples) == (False, 0, 1.0, 1)
    o, rest = train_image_mt.get_option_parser().parse_args(["--bt-sampling", "--bt-topk", "10", "--bt-temperature", "0.9"])
    assert not rest and o.bt_sampling is True and o.bt_topk == 10 and math.isclose(o.bt_temperature, 0.9)
    d = train_image_mt.get_option_parser().parse_args([])[0]
    assert (d.bt_sampling, d.bt_topk, d.bt_temperature) == (False, 0, 1.0)  # the greedy phase of before
    pinned = {o.dest for o in get_img_options_parser().option_list}
    assert not pinned & {"bt_sampling", "bt_topk", "bt_temperature", "sampling", "sampling_topk", "temperature", "nsamples"}


def test_decoder_refuses_bad_sampling_arguments():
    from imagetranslate_amd.seq_gen import BeamDecoder
    for kw in (dict(nsamples=0), dict(nsamples=33), dict(temperature=0.0), dict(temperature=float("nan")),
               dict(temperature=float("inf"))):
        with pytest.raises(ValueError):
            BeamDecoder(None, sampling=True, **kw)
    d = BeamDecoder(None)  # defaults: the search of before
    assert d.sampling is False and d.beam_width == 5
