"""imt_sample_step (csrc/sample.hip) through the C ABI against the fp64 oracle of tests/sample_oracle.py.

Tokens are compared on every draw whose oracle gap (best minus second-best perturbed value) is at least GAP = 1e-4 -- the
threshold of tests/util.beam_reference_is_unambiguous: the perturbed values are below ~40 in magnitude, so fp32 rounding of
x / T - log(-log u) stays under 1e-5 -- and a case may leave out at most 1 % of its draws; the inputs below leave out NONE, which
is asserted.  Scores are compared within 1e-5 (max |difference| / max |reference|).  The kept set needs no margin: it is decided by
exact comparisons of fp32 logits.

Kernel paths covered: 16-byte and scalar row sweeps (ld % 4, pointer alignment, V % 4 != 0), no filter / radix select / ties
at the k-th place (the extra ordered sweep), rep == 1 and rep == n, more than one sweep trip per pass (V = 30000 > 16384)."""
import functools

import pytest
import torch

from tests.sample_oracle import sample_step_reference
from tests.test_sample_host import FREQ_CAP, FREQ_CASES, FREQ_LOGITS, FREQ_ROWS, freq_case
from tests.util import call_beam_step, call_sample_step, rel_err

pytestmark = pytest.mark.gpu
GAP = 1e-4
PAD, EOS = 0, 4


def compare(got, ref, step, what, max_left_out=0.0):
    """Kernel outputs ``got`` against the oracle's ``ref`` for one step; returns the number of draws left out (gap < GAP)."""
    sure = ref["masked"] | (ref["gap"] >= GAP)
    left_out = int((~sure).sum())
    assert left_out <= max_left_out * sure.numel(), "%s: %d of %d draws too close to call" % (what, left_out, sure.numel())
    bad = (got["tokens"] != ref["tokens"]) & sure
    assert not bool(bad.any()), "%s: tokens differ in rows %s" % (what, bad.nonzero().flatten().tolist()[:8])
    ok = got["tokens"] == ref["tokens"]  # (rows too close to call: every output below follows the token)
    e = rel_err(got["scores"][ok], ref["scores"][ok])
    assert e <= 1e-5, "%s: scores %.3e" % (what, e)
    assert torch.equal(got["eos"][ok].bool(), ref["eos"][ok].bool()), what
    assert torch.equal(got["parent"], ref["parent"]), what
    assert torch.equal(got["hist"][ok, :step + 1], ref["hist"][ok, :step + 1]), what
    assert torch.equal(got["slots"][ok, :step + 1], ref["slots"][ok, :step + 1]), what
    if bool(ok.all()):
        want = torch.zeros_like(got["eos_count"])
        want[step] = ref["eos_count"]
        assert torch.equal(got["eos_count"], want), what
    return left_out


# ------------------------------------------------------------------------------------------- parity over 12 steps
PARITY = [  # (B, n, V, temperature, topk, seed): R = B * n rows
    (12, 4, 1000, 1.0, 0, 3), (12, 4, 1000, 0.8, 10, 4), (2, 4, 30000, 1.0, 0, 5), (2, 4, 30000, 0.9, 40, 6), (11, 3, 257, 1.3, 1, 7)]
STEPS, T_MAX = 12, 16


@functools.lru_cache(maxsize=None)
def parity_reference(B, n, V, temperature, topk, seed):
    """The oracle's 12 steps of one case: [(inputs of the step, oracle outputs)], every step continuing the ORACLE's state, so a
    kernel step is judged on its own.  Odd sentences may grow to 6 + (b % 7) tokens only: the later steps mask their rows."""
    g = torch.Generator().manual_seed(seed)
    max_lens = torch.tensor([6 + (b % 7) if b % 2 else T_MAX for b in range(B)], dtype=torch.int64)
    scores, eos_in = torch.zeros(B, dtype=torch.float32), torch.zeros(B, dtype=torch.uint8)
    hist, slots = torch.zeros(B, T_MAX, dtype=torch.int64), torch.zeros(B, T_MAX, dtype=torch.int32)
    hist[:, 0] = 5
    slots[:, 0] = torch.arange(B, dtype=torch.int32)
    out = []
    for step in range(1, STEPS + 1):
        rep = 1 if step == 1 else n
        logits = torch.randn(B * rep, V, generator=g) * 3
        inputs = dict(logits=logits, scores=scores, eos_in=eos_in, max_lens=max_lens, hist=hist, slots_in=slots, step=step, rep=rep)
        ref = sample_step_reference(logits, scores, eos_in, max_lens, hist, slots, step, B, n, rep, V, T_MAX, temperature, topk,
                                    seed, PAD, EOS)
        out.append((inputs, ref))
        scores, eos_in, hist, slots = ref["scores"].float(), ref["eos"].to(torch.uint8), ref["hist"], ref["slots"]
    return out


@pytest.mark.parametrize("B,n,V,temperature,topk,seed", PARITY)
def test_parity_with_fp64_oracle(cuda, B, n, V, temperature, topk, seed):
    left_out = masked = 0
    for inp, ref in parity_reference(B, n, V, temperature, topk, seed):
        got = call_sample_step(inp["logits"], inp["scores"], inp["eos_in"], inp["max_lens"], inp["hist"], inp["slots_in"], inp["step"],
                               B, n, inp["rep"], V, T_MAX, temperature, topk, seed)
        left_out += compare(got, ref, inp["step"], "step %d" % inp["step"], max_left_out=0.01)
        masked += int(ref["masked"].sum())
    print("R %d V %d T %.1f topk %d: %d draws left out, %d masked rows" % (B * n, V, temperature, topk, left_out, masked))
    assert left_out == 0, "the inputs were chosen so that the oracle decides every draw"
    assert 0 < masked < B * n * STEPS


def _fresh(rows, t_max=8, step=1):
    """An empty search state of ``rows`` input rows: (scores, eos_in, hist, slots)."""
    hist, slots = torch.zeros(rows, t_max, dtype=torch.int64), torch.zeros(rows, t_max, dtype=torch.int32)
    hist[:, :step] = torch.arange(rows * step).view(rows, step) % 97 + 5
    slots[:, :step] = torch.arange(rows * step, dtype=torch.int32).view(rows, step) % rows
    return torch.linspace(-3, 0, rows), torch.zeros(rows, dtype=torch.uint8), hist, slots


def _one_step(logits, B, n, rep, step, temperature, topk, seed, max_lens=None, eos_in=None, t_max=8, **layout):
    rows, V = logits.shape
    scores, eos0, hist, slots = _fresh(rows, t_max, step)
    eos_in = eos0 if eos_in is None else eos_in
    max_lens = torch.full((B,), 100, dtype=torch.int64) if max_lens is None else max_lens
    got = call_sample_step(logits, scores, eos_in, max_lens, hist, slots, step, B, n, rep, V, t_max, temperature, topk, seed, **layout)
    ref = sample_step_reference(logits, scores, eos_in, max_lens, hist, slots, step, B, n, rep, V, t_max, temperature, topk, seed,
                                PAD, EOS)
    return got, ref, scores


def test_first_step_with_32_samples(cuda):
    """n = 32 at step 1 (rep == 1): the 32 children of a sentence share its row, start from its cached position and differ."""
    logits = torch.randn(3, 64, generator=torch.Generator().manual_seed(21)) * 3
    got, ref, _ = _one_step(logits, 3, 32, 1, 1, 1.0, 0, 77)
    assert compare(got, ref, 1, "n = 32") == 0
    assert got["parent"].tolist() == [b for b in range(3) for _ in range(32)]
    assert all(len(set(got["tokens"][b * 32:(b + 1) * 32].tolist())) > 4 for b in range(3))


@pytest.mark.parametrize("V,ld,offset,topk", [(1001, 1004, 0, 0), (1001, 1004, 4, 7), (1001, 1005, 0, 7), (1000, 1000, 1, 7),
                                              (1000, 1003, 3, 0), (5, 8, 0, 3)])
def test_padded_and_unaligned_rows(cuda, V, ld, offset, topk):
    """Rows ``ld`` apart with NaN in the columns [V, ld) -- never read -- and row starts on and off 16-byte alignment."""
    logits = torch.randn(12, V, generator=torch.Generator().manual_seed(V + ld + offset)) * 3
    got, ref, _ = _one_step(logits, 4, 3, 3, 2, 0.9, topk, 31, ld=ld, offset=offset, pad_fill=float("nan"))
    assert compare(got, ref, 2, "V %d ld %d offset %d" % (V, ld, offset)) == 0
    assert bool(torch.isfinite(got["scores"]).all())


def test_topk_values(cuda):
    """topk 0, V and V + 5 are the whole vocabulary (the same bits); 1 is the argmax; V - 1 drops the single smallest logit."""
    V = 300
    logits = torch.randn(20, V, generator=torch.Generator().manual_seed(8)) * 3
    outs = {}
    for topk in (0, 1, V - 1, V, V + 5):
        got, ref, _ = _one_step(logits, 5, 4, 4, 3, 1.1, topk, 19)
        assert compare(got, ref, 3, "topk %d" % topk) == 0
        outs[topk] = got
    for topk in (V, V + 5):
        assert torch.equal(outs[topk]["tokens"], outs[0]["tokens"]) and torch.equal(outs[topk]["scores"], outs[0]["scores"])
    assert torch.equal(outs[1]["tokens"], logits.argmax(dim=1))
    assert not bool((outs[V - 1]["tokens"] == logits.argmin(dim=1)).any())


def test_ties_at_the_kth_place(cuda):
    """Six equal maxima and topk = 4: only the four LOWEST of their indices may be drawn, and each of the four is."""
    rows, V = 2000, 3000
    g = torch.Generator().manual_seed(13)
    logits = torch.randn(rows, V, generator=g).clamp_(max=2.5)
    where = torch.stack([torch.randperm(V, generator=g)[:6].sort().values for _ in range(rows)])
    logits.scatter_(1, where, 3.0)
    got, ref, _ = _one_step(logits, rows, 1, 1, 1, 1.0, 4, 23)
    rank = (where == got["tokens"][:, None]).int().argmax(dim=1)
    assert bool((where == got["tokens"][:, None]).any(dim=1).all()), "a token outside the six maxima"
    assert int(rank.max()) <= 3, "one of the two highest indices was drawn"
    assert sorted(set(rank.tolist())) == [0, 1, 2, 3]
    assert compare(got, ref, 1, "ties", max_left_out=0.01) <= 0.01 * rows


def test_masked_rows(cuda):
    """Finished rows and, at step > 1, rows over their length limit take PAD and keep their score; at step 1 the limit is not
    looked at (the rule of beam_row_topk_kernel)."""
    B, n, V = 6, 2, 200
    logits = torch.randn(B * n, V, generator=torch.Generator().manual_seed(17)) * 3
    max_lens = torch.tensor([100, 3, 100, 2, 100, 100])  # sentences 1 and 3 are over the limit at step 3
    eos_in = torch.zeros(B * n, dtype=torch.uint8)
    eos_in[[0, 5]] = 1
    got, ref, scores = _one_step(logits, B, n, n, 3, 1.0, 0, 3, max_lens=max_lens, eos_in=eos_in)
    assert compare(got, ref, 3, "masked, step 3") == 0
    masked = [0, 5, 2, 3, 6, 7]
    free = [r for r in range(B * n) if r not in masked]
    assert ref["masked"].nonzero().flatten().tolist() == sorted(masked)
    assert bool((got["tokens"][masked] == PAD).all()) and torch.equal(got["scores"][masked], scores[masked])
    assert got["eos"][masked].tolist() == [1, 1, 0, 0, 0, 0]
    assert bool((got["scores"][free] < scores[free]).all())
    # the same limits at step 1: every row is sampled
    got, ref, scores = _one_step(logits[:B], B, n, 1, 1, 1.0, 0, 3, max_lens=max_lens)
    assert compare(got, ref, 1, "masked, step 1") == 0
    assert not bool(ref["masked"].any()) and bool((got["scores"] < scores[got["parent"].long()]).all())


def test_two_calls_give_the_same_bits(cuda):
    inp, _ = parity_reference(*PARITY[3])[5]
    B, n, V, temperature, topk, seed = PARITY[3]
    run = lambda: call_sample_step(inp["logits"], inp["scores"], inp["eos_in"], inp["max_lens"], inp["hist"], inp["slots_in"],
                                   inp["step"], B, n, inp["rep"], V, T_MAX, temperature, topk, seed)
    first, second = run(), run()
    for key in first:
        assert torch.equal(first[key], second[key]), key
    assert torch.equal(first["scores"].view(torch.int32), second["scores"].view(torch.int32))


@pytest.mark.parametrize("temperature,topk,seed", FREQ_CASES)
def test_frequencies(cuda, temperature, topk, seed):
    logits, n, rep, step, p, kept = freq_case(temperature, topk, seed)
    B = FREQ_ROWS // rep
    scores, eos_in, hist, slots = _fresh(FREQ_ROWS, 4, step)
    got = call_sample_step(logits, scores, eos_in, torch.full((B,), 100, dtype=torch.int64), hist, slots, step, B, n, rep,
                           len(FREQ_LOGITS), 4, temperature, topk, seed, eos=100)
    freq = torch.bincount(got["tokens"], minlength=len(FREQ_LOGITS)).double() / FREQ_ROWS
    dev = float((freq - p).abs().max())
    print("T %.1f topk %d seed %d: largest deviation %.4f" % (temperature, topk, seed, dev))
    assert set(got["tokens"].tolist()) <= set(kept), "a draw outside the kept set"
    assert dev <= FREQ_CAP, dev


# ------------------------------------------------------------------------------------------- what the two steps share
# V = 7: one quad and the tail; 4099 / 16389: the first indices of the scalar / the 16-byte sweep's second trip, and a tail
@pytest.mark.parametrize("V", [7, 4099, 16389])
@pytest.mark.parametrize("vec", [False, True])  # rows V apart (odd: the scalar kernels) or padded to 16 bytes (the 16-byte ones)
@pytest.mark.parametrize("step", [1, 3])
def test_greedy_sampling_is_beam_one(cuda, step, vec, V):
    """imt_beam_step with beam = 1 and imt_sample_step with n = 1, topk = 1 are the same greedy step: every integer output
    equal, the scores within the 1e-5 of compare() (the two kernels round the log-sum-exp differently)."""
    layout = dict(ld=(V + 3) // 4 * 4 if vec else V, pad_fill=float("nan"))
    B, t_max = 5, 8
    logits = torch.randn(B, V, generator=torch.Generator().manual_seed(100 * step + V)) * 3
    logits[2, EOS] = logits[2].max() + 1.0                      # a row whose argmax is EOS
    eos_in = torch.tensor([1, 0, 0, 0, 0], dtype=torch.uint8)   # a finished row
    max_lens = torch.tensor([100, 2, 100, 100, 100])            # sentence 1 is past its limit at step 3 (step 1 does not look)
    live = [b for b in range(B) if not (eos_in[b] or (step > 1 and max_lens[b] < step + 1))]
    top2 = logits[live].topk(2, dim=1).values
    assert bool((top2[:, 0] > top2[:, 1]).all()), "the argmax of every live row must be decided"
    scores, _, hist, slots = _fresh(B, t_max, step)
    beam = call_beam_step(logits, scores, torch.zeros(B), eos_in, max_lens, hist, slots, step, B, 1, 1, V, t_max, 0.8, PAD, EOS,
                          **layout)
    samp = call_sample_step(logits, scores, eos_in, max_lens, hist, slots, step, B, 1, 1, V, t_max, 0.7, 1, 41, **layout)
    for key in ("tokens", "eos", "parent", "eos_count"):
        assert torch.equal(samp[key], beam[key]), key
    for key in ("hist", "slots"):
        assert torch.equal(samp[key][:, :step + 1], beam[key][:, :step + 1]), key
    e = rel_err(samp["scores"], beam["scores"])
    print("step %d V %d: scores differ by %.3e" % (step, V, e))
    assert e <= 1e-5, e
    want = torch.full((B,), PAD, dtype=torch.int64)
    want[live] = logits[live].argmax(dim=1)
    assert torch.equal(beam["tokens"], want) and int(beam["tokens"][2]) == EOS
    want_eos = eos_in.bool() | (want == EOS)
    assert torch.equal(beam["eos"].bool(), want_eos) and int(beam["eos_count"][step]) == int(want_eos.sum())


def test_sample_step_history_past_1024_positions(cuda):
    """The sampling kernel copies history and slot rows 1024 positions per trip: step 1026 is the first with a second trip.
    Columns past the step keep what the output buffers held."""
    n, V, t_max, step, fill = 2, 8, 1030, 1026, -7
    g = torch.Generator().manual_seed(9)
    hist, slots = torch.zeros(n, t_max, dtype=torch.int64), torch.zeros(n, t_max, dtype=torch.int32)
    hist[:, :step] = torch.randint(5, 1000, (n, step), generator=g)
    slots[:, :step] = torch.randint(0, n, (n, step), generator=g, dtype=torch.int32)
    got = call_sample_step(torch.randn(n, V, generator=g) * 3, torch.zeros(n), torch.zeros(n, dtype=torch.uint8),
                           torch.tensor([2000]), hist, slots, step, 1, n, n, V, t_max, 1.0, 0, 5, out_fill=fill)
    assert got["parent"].tolist() == [0, 1]
    assert torch.equal(got["hist"][:, :step], hist[:, :step]) and torch.equal(got["slots"][:, :step], slots[:, :step])
    assert torch.equal(got["hist"][:, step], got["tokens"]) and got["slots"][:, step].tolist() == [0, 1]
    assert bool((got["hist"][:, step + 1:] == fill).all()) and bool((got["slots"][:, step + 1:] == fill).all())
