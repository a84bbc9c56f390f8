"""imt_beam_step at real vocabulary sizes and wide beams, against a double-precision restatement of the reference's step
(src/seq_gen.py:193-227; tests/util.py ref_beam_step with dtype=float64).

Which row top-k kernel a case reaches, read from the dispatch at the bottom of csrc/decode.hip (imt_beam_step):
  * beam_row_topk_fast_kernel<4>: beam <= 4, ld % 4 == 0 and the logits pointer 16-byte aligned;
  * beam_row_topk_fast_kernel<8>: 5 <= beam <= 8, same layout;
  * beam_row_topk_kernel (general): beam 9..32, or ld % 4 != 0, or a pointer off 16-byte alignment.
A thread of the 1024-thread fast kernels owns the f32x4 at 4 * tid of every 4096-element sweep; it requests four sweeps
per trip of its loop (16384 elements), clamps the addresses of sweeps past the row, keeps its K best in registers and
handles V % 4 trailing elements one by one.  The vocabulary sizes below cross each of these: more than K elements per
thread (V > 1024 * K), one sweep, one trip, several trips, V % 4 != 0, and the minimum V == beam.

Tokens, parents, histories, slot tables, EOS flags and sizes are compared EXACTLY; that is only fair where the reference
itself is unambiguous, so every case first asserts -- on the CPU, before any kernel output is looked at -- that adjacent
candidates among each sentence's best beam + 1 are either bit-equal in fp64 (a constructed tie, decided by the lowest flat
index) or at least 1e-4 apart (scores here stay below 16 in magnitude, where 1e-4 is more than six times 16 fp32 ulps).
That is a condition on the inputs, met by the choice of seeds, not a tolerance for the kernel."""
import pytest
import torch

from tests.util import assert_close, beam_reference_is_unambiguous, call_beam_step, ref_beam_step

pytestmark = pytest.mark.gpu
PAD, RATIO, GAP = 0, 0.8, 1e-4
SWEEP, TRIP = 4096, 16384    # elements per sweep / per loop trip of the fast kernels (FAST_THREADS * 4, times NS = 4)


def _ld8(V):
    return (V + 7) // 8 * 8


def _make_case(seed, B, beam, V, step, t_max=8, logits="randn", eos_rows=True, over=True):
    """CPU inputs of one step: random logits ('randn': randn * 3; 'grid': randint(-12, 13) / 4), scores -rand * 5, a random
    history and slot table; for step > 1 a third of the rows already carry EOS and sentence 1 is over its length limit."""
    g = torch.Generator().manual_seed(seed)
    rep = 1 if step == 1 else beam
    rows, r_out = B * rep, B * beam
    eos = 4 if V > 4 else V - 1
    if logits == "grid":
        x = torch.randint(-12, 13, (rows, V), generator=g).float() / 4
    else:
        x = torch.randn(rows, V, generator=g) * 3
    hist = torch.randint(0, V - 1, (rows, t_max), generator=g)
    hist += (hist >= eos).long()                                   # any token but EOS
    hist[:, step:] = 0
    eos_in = torch.zeros(rows, dtype=torch.bool)
    if step > 1 and eos_rows:
        eos_in[torch.randperm(rows, generator=g)[:rows // 3]] = True
        hist[eos_in, step - 1] = eos
    scores = -torch.rand(rows, generator=g) * 5
    sizes = torch.randint(1, step + 1, (rows,), generator=g).float()
    max_lens = torch.full((B,), t_max + 1)
    if over:
        max_lens[0] = step + 1
        if B > 1:
            max_lens[1] = step                                     # over the limit when step > 1
    slots = torch.randint(0, r_out, (rows, t_max), generator=g, dtype=torch.int32)
    return dict(B=B, beam=beam, V=V, step=step, rep=rep, t_max=t_max, eos=eos, logits=x, scores=scores, sizes=sizes,
                eos_in=eos_in, max_lens=max_lens, hist=hist, slots=slots)


def _reference(c):
    """fp64 reference of the case, computed once; asserts the condition on the inputs (module docstring)."""
    if "ref" not in c:
        ref = ref_beam_step(c["logits"], c["scores"], c["sizes"], c["eos_in"], c["max_lens"], c["hist"], c["step"], c["B"],
                            c["beam"], c["rep"], c["V"], RATIO, PAD, c["eos"], dtype=torch.float64, return_sorted=True)
        ok, smallest = beam_reference_is_unambiguous(ref[5], c["beam"], GAP)
        print("beam %d V %d step %d: smallest non-zero gap among the best candidates %.2e, largest |score| %.2f"
              % (c["beam"], c["V"], c["step"], smallest, float(ref[0].abs().max())))
        assert ok, "inputs are ambiguous for an fp32 kernel (gap %.2e < %.0e): choose another seed" % (smallest, GAP)
        assert float(ref[0].abs().max()) < 16
        c["ref"] = ref
    return c["ref"]


def _run(c, ld=None, offset=0, pad_fill=0.0):
    _reference(c)
    return call_beam_step(c["logits"], c["scores"], c["sizes"], c["eos_in"], c["max_lens"], c["hist"], c["slots"], c["step"],
                          c["B"], c["beam"], c["rep"], c["V"], c["t_max"], RATIO, PAD, c["eos"], ld=ld, offset=offset,
                          pad_fill=pad_fill)


def _check(c, o):
    top, new_sizes, new_eos, new_hist, prow, _ = _reference(c)
    step, r_out = c["step"], c["B"] * c["beam"]
    assert torch.equal(o["tokens"], new_hist[:, step]), "tokens"
    assert torch.equal(o["parent"].long(), prow), "parents"
    assert torch.equal(o["hist"][:, :step + 1], new_hist), "token history"
    assert torch.equal(o["eos"].bool(), new_eos), "EOS flags"
    assert int(o["eos_count"][step]) == int(new_eos.sum())
    if c["beam"] > 1:
        assert torch.equal(o["sizes"], new_sizes), "sizes"
    assert torch.equal(o["slots"][:, :step], c["slots"][prow, :step]), "slot table (ancestors)"
    assert torch.equal(o["slots"][:, step], torch.arange(r_out, dtype=torch.int32)), "slot table (own row)"
    assert_close(o["scores"], top.float(), 1e-5, "beam scores")


def _run_and_check(c, **kw):
    o = _run(c, **kw)
    _check(c, o)
    return o


def _poison(step):
    return float("inf") if step == 1 else float("nan")


# ------------------------------------------------------------------------------------------------ random cases
FAST4 = [(b, V) for b in (1, 4) for V in (4, 257, 4099, 16389, 50003)]
FAST8 = [(b, V) for b in (5, 8) for V in (8, 8200, 16389, 30001, 65536)]
WIDE = [(b, V) for b in (9, 12, 32) for V in (32, 1000, 50003)]


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("beam,V", FAST4 + FAST8 + WIDE)
def test_beam_step_random_padded_rows(cuda, beam, V, step):
    """Rows ld = V rounded up to 8 apart in an aligned buffer: fast<4> (beam <= 4), fast<8> (beam 5..8), general (beam > 8).
    The pad columns [V, ld) hold +inf (first step) or NaN (later steps): the kernels may read only v < V."""
    reseed = {(32, 32, 1): 9, (32, 1000, 1): 3}.get((beam, V, step), 0)   # seeds for which the condition on the inputs holds
    c = _make_case(100000 * step + 1000 * beam + V % 1000 + 7919 * reseed, 3 if beam > 8 else 4, beam, V, step)
    _run_and_check(c, ld=_ld8(V), pad_fill=_poison(step))


@pytest.mark.parametrize("step", [1, 2])
def test_beam_step_odd_leading_dimension(cuda, step):
    """Contiguous rows of an odd length (ld = V = 4099, not a multiple of 4) take the general kernel at beam 4; the same
    logits in rows padded to 8 take fast<4>: both match the reference, and each other in every token and parent."""
    c = _make_case(77 + step, 4, 4, 4099, step)
    a = _run_and_check(c)
    b = _run_and_check(c, ld=_ld8(4099), pad_fill=_poison(step))
    for k in ("tokens", "parent", "cand_idx"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("beam", [4, 8])
def test_beam_step_unaligned_pointer(cuda, beam, step):
    """A view that starts at element 1 of a buffer (4 bytes off 16-byte alignment, ld % 4 == 0) takes the general kernel;
    the aligned copy takes fast<4> / fast<8>."""
    V = 16389
    c = _make_case(500 + 10 * beam + step, 4, beam, V, step)
    a = _run_and_check(c, ld=_ld8(V), offset=1, pad_fill=_poison(step))
    b = _run_and_check(c, ld=_ld8(V), pad_fill=_poison(3 - step))
    for k in ("tokens", "parent", "cand_idx"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("beam", [4, 8, 12])
def test_beam_step_pad_columns_are_never_read(cuda, beam):
    """Zero, +inf and NaN in the pad columns give bit-identical outputs, scores included."""
    V = 16389
    c = _make_case(900 + beam, 3, beam, V, 2)
    runs = [_run(c, ld=_ld8(V) + 8, pad_fill=f) for f in (0.0, float("inf"), float("nan"))]
    _check(c, runs[0])
    for o in runs[1:]:
        for k in ("scores", "sizes", "eos", "hist", "slots", "parent", "tokens", "cand_idx", "cand_scores"):
            assert torch.equal(o[k], runs[0][k]), k


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("beam", [4, 8, 12])
def test_beam_step_constant_row(cuda, beam, step):
    """A row whose logits are all equal: its candidates are the indices 0 .. beam-1, in order."""
    V = 50003
    c = _make_case(1300 + 10 * beam + step, 3, beam, V, step, eos_rows=False, over=False)
    rows = [b * c["rep"] + b % c["rep"] for b in range(c["B"])]
    c["logits"][rows] = 1.25
    c["scores"][:c["rep"]] = -14.0                                    # sentence 0: the constant row (log-prob -10.8) leads
    c["scores"][rows[0]] = 0.0
    o = _run_and_check(c, ld=_ld8(V), pad_fill=_poison(step))
    for r in rows:
        assert o["cand_idx"][r].tolist() == list(range(beam)), r
        assert bool((o["cand_scores"][r] == o["cand_scores"][r, 0]).all())
    assert o["tokens"][:beam].tolist() == list(range(beam))


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("V", [4099, 16389, 50003, 65536])
@pytest.mark.parametrize("beam", [4, 8, 12, 32])
def test_beam_step_grid_logits(cuda, beam, V, step):
    """Logits on a grid of quarter units: the best beam + 1 candidates of every sentence are exact ties (asserted on the
    fp64 reference), so the order is decided by the index alone."""
    c = _make_case(2000 + 100 * beam + V % 97 + step, 3, beam, V, step, logits="grid")
    vals = _reference(c)[5]
    assert bool((vals[:, :beam + 1] == vals[:, :1]).all()), "the best beam + 1 candidates must tie exactly"
    _run_and_check(c, ld=_ld8(V), pad_fill=_poison(step))


def _planted(beam, V):
    """Index sets that receive one equal maximum each (one set per sentence).  For the fast kernels a thread owns the
    f32x4 at 4 * tid of every sweep; the general kernel's thread v % 256 owns every 256th element."""
    return [
        [40, 41],                                                     # two in one f32x4
        [44, 46, 44 + SWEEP, 47 + SWEEP],                             # one thread, different sweeps of one trip
        [48, 48 + TRIP, 49 + 2 * TRIP],                               # one thread, different trips
        [52 + SWEEP * i for i in range(beam + 1)],                    # more than the thread's K slots (K >= beam)
        [52 + SWEEP * i for i in range(beam + 1)] + [60 + SWEEP],     # ... and another thread's, ordered between them
        [56, 156, 56 + 4 * 64 * 5],                                   # different waves (of either kernel)
        [60, (V & ~3) - 1, V & ~3, V - 1],                            # the scalar tail [V & ~3, V) and the last f32x4
    ]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("beam", [4, 8, 12])
def test_beam_step_planted_equal_maxima(cuda, beam, step):
    V = 50003
    assert V % 4 == 3 and 52 + SWEEP * beam < (V & ~3)
    sets = _planted(beam, V)
    c = _make_case(3100 + 10 * beam + step, len(sets), beam, V, step, eos_rows=False, over=False)
    rows = [b * c["rep"] + b % c["rep"] for b in range(c["B"])]
    c["scores"] -= 3.0
    for r, p in zip(rows, sets):
        c["logits"][r, p] = float(c["logits"][r].max()) + 2.0
        c["scores"][r] = 0.0                                          # the planted row leads its sentence
    o = _run_and_check(c, ld=_ld8(V), pad_fill=_poison(step))
    for b, (r, p) in enumerate(zip(rows, sets)):
        want = sorted(p)[:beam]
        assert o["cand_idx"][r, :len(want)].tolist() == want, (b, "row candidates")
        assert o["tokens"][b * beam:b * beam + len(want)].tolist() == want, (b, "tokens")
        assert bool((o["parent"][b * beam:b * beam + len(want)] == r).all())


@pytest.mark.parametrize("beam", [4, 8, 12])
def test_beam_step_identical_rows(cuda, beam):
    """Rows of a sentence with equal logits, scores and sizes: every candidate ties with its twins in the other rows, and
    the lower row wins."""
    V, B, step = 16389, 3, 2
    c = _make_case(4200 + beam, B, beam, V, step, eos_rows=False, over=False)
    for t in ("logits", "scores", "sizes"):
        c[t][1:beam] = c[t][0]                                        # sentence 0: all rows identical
        c[t][beam + 3] = c[t][beam + 1]                               # sentence 1: rows 1 and 3 identical, both leading
    c["scores"][[beam + 1, beam + 3]] = 0.0
    o = _run_and_check(c, ld=_ld8(V), pad_fill=_poison(step))
    assert o["parent"][:beam].tolist() == list(range(beam)), "one candidate per twin row, lowest row first"
    assert bool((o["tokens"][:beam] == o["tokens"][0]).all())


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_beam_step_history_past_64_positions(cuda):
    """beam_merge_kernel copies history and slot rows 64 positions per trip: step 100 of t_max 130."""
    c = _make_case(5001, 4, 4, 1000, 100, t_max=130)
    c["sizes"] = torch.randint(1, 100, c["sizes"].shape, generator=torch.Generator().manual_seed(1)).float()
    c["hist"][:, :100] = torch.randint(5, 1000, (16, 100), generator=torch.Generator().manual_seed(2))
    c["hist"][c["eos_in"], 99] = c["eos"]
    o = _run_and_check(c)
    prow = o["parent"].long()
    assert torch.equal(o["hist"][:, :100], c["hist"][prow, :100]) and torch.equal(o["hist"][:, 100], o["tokens"])
    assert torch.equal(o["slots"][:, :100], c["slots"][prow, :100])
    assert torch.equal(o["slots"][:, 100], torch.arange(16, dtype=torch.int32))


@pytest.mark.parametrize("step", [1, 5])
def test_beam_step_inference_batch(cuda, step):
    """64 sentences x beam 5 = 320 rows, the reference's inference batch."""
    c = _make_case(6000 + step + (23757 if step == 1 else 0), 64, 5, 1000, step)   # (a seed for which the condition on the inputs holds)
    g = torch.Generator().manual_seed(step)
    c["max_lens"] = torch.randint(step - 1, step + 4, (64,), generator=g)
    _run_and_check(c)
