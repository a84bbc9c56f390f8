"""The scorer on the GPU: the fused projection + log-sum-exp kernel (imt_score_rows) against an fp64 computation, its
dispatch and memory footprint, Seq2Seq.score against tests/score_oracle.py at toy and at benchmarked (C1) size in fp32 and
bf16, and the score_pairs entry point against the oracle's ranking.

Bars.  Op level and fp32 model level: 1e-4 of the largest |value|, the project's fp32 bar (fp32 accumulation measured at
<= 1.7e-7 against fp64, a bf16 rounding of the logits at >= 5.4e-4: the bar separates a kernel that keeps the logits in
fp32 from one that rounds them).  bf16 model level: the error of Seq2Seq.score against the oracle may not exceed 1.25 x the
error of scores gathered from the existing bf16 forward(log_softmax=True), nor the existing bf16 log-prob bar (4e-2)."""
import marshal
import math
import os

import pytest
import torch

from oracle import reference_model as R
from tests.score_oracle import oracle_rank, oracle_scores
from tests.test_gpu_c1 import C1, V as C1_V, _batch as c1_batch, _kinds_of_step, write_truth_log
from tests.test_score_host import TOY, toy_batch
from tests.util import beam_state_dict

pytestmark = pytest.mark.gpu


def _bf16_repr(t):
    return t.to(torch.bfloat16).float()


def _op_case(N, V, K, seed):
    """bf16-representable x [N, K], w [V, K], bias [V]; targets with the special cases of the issue; segment offsets."""
    g = torch.Generator().manual_seed(seed)
    x = _bf16_repr(torch.randn(N, K, generator=g))
    w = _bf16_repr(torch.randn(V, K, generator=g) * 0.05)
    bias = _bf16_repr(torch.randn(V, generator=g) * 0.5)
    tgt = torch.randint(0, V, (N,), generator=g)
    tgt[0] = V - 1                                   # last column (inside the ragged tile)
    if N >= 37:
        tgt[1] = 0                                   # first column
        x[2] *= 32.0                                 # logits of magnitude ~ 100: an unshifted exp overflows fp32
        x[7] *= 32.0
        x[3] = _bf16_repr(w[V - 1] * 8.0)            # this row's maximum sits in the last (ragged) column tile
        tgt[4], tgt[5], tgt[6] = -1, V, V + 5        # out of range: ignored rows
        tgt[20:26] = -100                            # a whole segment of ignored rows (below)
    # segments: [0, 8), [8, 20), [20, 26) all ignored, [26, 26) empty, then runs of 61 rows
    cuts = [0]
    if N >= 37:
        cuts += [8, 20, 26, 26]
    while cuts[-1] < N:
        cuts.append(min(N, cuts[-1] + 61))
    cuts.append(N)                                   # an empty segment at the end
    return x, w, bias, tgt, torch.tensor(cuts, dtype=torch.long)


def _fp64_reference(x, w, bias, tgt, off, normalize):
    """logprob, lse, per-segment score in fp64 (row blocks: no [N, V] fp64 matrix at the largest size)."""
    N, V = x.shape[0], w.shape[0]
    xd, wd = x.double(), w.double()
    bd = bias.double() if bias is not None else None
    valid = (tgt >= 0) & (tgt < V)
    safe = torch.where(valid, tgt, torch.zeros_like(tgt))
    lse = torch.empty(N, dtype=torch.float64, device=x.device)
    lp = torch.empty(N, dtype=torch.float64, device=x.device)
    amax = torch.empty(N, dtype=torch.long, device=x.device)
    for r0 in range(0, N, 1024):
        r1 = min(N, r0 + 1024)
        logits = xd[r0:r1] @ wd.t()
        if bd is not None:
            logits += bd
        lse[r0:r1] = torch.logsumexp(logits, dim=1)
        lp[r0:r1] = logits.gather(1, safe[r0:r1].unsqueeze(1)).squeeze(1) - lse[r0:r1]
        amax[r0:r1] = logits.argmax(1)
    lp = torch.where(valid, lp, torch.zeros_like(lp))
    seg = []
    for s in range(off.numel() - 1):
        a, b = int(off[s]), int(off[s + 1])
        tot, cnt = lp[a:b].sum(), int(valid[a:b].sum())
        seg.append(tot / cnt if (normalize and cnt) else tot)
    return lp, lse, torch.stack(seg), amax


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [512, 768])
@pytest.mark.parametrize("V", [250, 1000, 30000])
@pytest.mark.parametrize("N", [1, 37, 320, 8128])
def test_score_rows_against_fp64(cuda, N, V, K, dtype):
    from imagetranslate_amd import hip_ops as O
    assert V % 256 != 0 and (N == 1 or N % 256 != 0)   # ragged last column tile in every case, ragged rows too
    x, w, bias, tgt, off = [t.to(cuda) for t in _op_case(N, V, K, seed=N + V + K)]
    for use_bias in (True, False):
        b = bias if use_bias else None
        for normalize in (True, False):
            want_lp, want_lse, want_seg, amax = _fp64_reference(x, w, b, tgt, off, normalize)
            args = (x.to(dtype), w.to(dtype), None if b is None else b.to(dtype), tgt)
            (lp, lse, seg), kinds = _kinds_of_step(lambda: O.score_rows(*args, seg_offsets=off, normalize=normalize))
            # every (dtype, V, K) of this set is taken by the fused kernel: the special cases below went through it
            fused = "score_xl_bf16" if dtype == torch.bfloat16 else "score_xl_f32"
            assert kinds.get(fused, 0) == 1 and kinds.get("score_combine", 0) == 1, kinds
            assert not any(k.startswith("gemm") or k.startswith("log_softmax") for k in kinds), kinds
            assert lp.dtype == lse.dtype == seg.dtype == torch.float32
            e_lp = float((lp.double() - want_lp).abs().max()) / float(want_lp.abs().max().clamp(min=1e-30))
            e_lse = float((lse.double() - want_lse).abs().max()) / float(want_lse.abs().max())
            e_seg = float((seg.double() - want_seg).abs().max()) / float(want_seg.abs().max().clamp(min=1e-30))
            print("score_rows N %d V %d K %d %s bias %d norm %d: logprob %.2e lse %.2e seg %.2e (max |lp| %.1f)"
                  % (N, V, K, dtype, use_bias, normalize, e_lp, e_lse, e_seg, float(want_lp.abs().max())))
            assert torch.isfinite(lp).all() and torch.isfinite(lse).all() and torch.isfinite(seg).all()
            assert e_lp <= 1e-4 and e_lse <= 1e-4 and e_seg <= 1e-4, (e_lp, e_lse, e_seg)
            if N >= 37:
                # the two large-magnitude rows set the scale above; the ordinary rows also meet the bar on their own scale
                rest = torch.ones(N, dtype=torch.bool, device=cuda)
                rest[2] = rest[7] = False
                for got, ref64 in ((lp, want_lp), (lse, want_lse)):
                    assert float((got.double() - ref64)[rest].abs().max()) <= 1e-4 * float(ref64[rest].abs().max())
                assert float(want_lse[2]) > 89.0 and float(want_lse[7]) > 89.0, "fixture: exp(logit) must overflow fp32"
                assert int(amax[3]) >= 256 * ((V - 1) // 256), "row 3's maximum must sit in the ragged tile"
                assert float(lp[4]) == 0.0 and float(lp[5]) == 0.0 and float(lp[6]) == 0.0 and float(lp[22]) == 0.0
                assert float(seg[2]) == 0.0 and float(seg[3]) == 0.0, "a segment without counted rows scores 0"
            assert float(seg[-1]) == 0.0
            lp2, lse2, seg2 = O.score_rows(*args, seg_offsets=off, normalize=normalize)
            assert torch.equal(lp, lp2) and torch.equal(lse, lse2) and torch.equal(seg, seg2), "two calls are bit-identical"
    # without segments
    lp3, lse3, seg3 = O.score_rows(x.to(dtype), w.to(dtype), bias.to(dtype), tgt)
    assert seg3 is None
    want_lp, want_lse, _, _ = _fp64_reference(x, w, bias, tgt, off, True)
    assert float((lp3.double() - want_lp).abs().max()) <= 1e-4 * float(want_lp.abs().max().clamp(min=1e-30))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_score_rows_chunked_path_for_shapes_the_fused_kernel_does_not_take(cuda, dtype):
    """K = 520 is not a whole number of K tiles: the same numbers come from the existing kernels (fp32 logits, log-softmax,
    gather) in blocks of at most 2048 rows; same 1e-4 bar (the logits are never rounded to bf16 there either)."""
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd import hip_ops as O
    N, V, K = 2500, 1000, 520
    assert L.load().imt_score_supported(O.IMT_BF16 if dtype == torch.bfloat16 else O.IMT_F32, V, K) == 0
    x, w, bias, tgt, off = [t.to(cuda) for t in _op_case(N, V, K, seed=5)]
    want_lp, want_lse, want_seg, _ = _fp64_reference(x, w, bias, tgt, off, True)
    (lp, lse, seg), kinds = _kinds_of_step(lambda: O.score_rows(x.to(dtype), w.to(dtype), bias.to(dtype), tgt, seg_offsets=off))
    assert not any(k.startswith("score_") for k in kinds) and kinds.get("log_softmax_fwd", 0) == 2, kinds
    for got, want in ((lp, want_lp), (lse, want_lse), (seg, want_seg)):
        assert float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_score_rows_dispatch_and_memory_at_c1_size(cuda):
    """N 8128, V 30000, K 512, bf16: the fused kinds run, the chain's do not, and no [N, V] buffer exists -- peak allocated
    memory grows by less than a quarter of N * V * 2 bytes (the partials are 1.6 % of it)."""
    from imagetranslate_amd import hip_ops as O
    N, V, K = 8128, 30000, 512
    x, w, bias, tgt, off = [t.to(cuda) for t in _op_case(N, V, K, seed=9)]
    args = (x.bfloat16(), w.bfloat16(), bias.bfloat16(), tgt)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, kinds = _kinds_of_step(lambda: O.score_rows(*args, seg_offsets=off))
    grow = torch.cuda.max_memory_allocated() - base
    print("score_rows at C1 size: peak memory +%.1f MB (logits alone would be %.1f MB); kinds %s" % (grow / 1e6, N * V * 2 / 1e6, kinds))
    assert kinds.get("score_xl_bf16", 0) == 1 and kinds.get("score_combine", 0) == 1, kinds
    assert "log_softmax_fwd" not in kinds and not any(k.startswith("gemm") for k in kinds), kinds
    assert grow < N * V * 2 / 4, grow


# ------------------------------------------------------------------------------------------------ model level
def _toy_pair(lang_dec, tie_embed, seed=21):
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    torch.manual_seed(seed)
    ref = R.Seq2Seq(R.SyntheticTextProcessor(1000), lang_dec=lang_dec, tie_embed=tie_embed, **TOY).eval()
    ref.load_state_dict(beam_state_dict(ref.state_dict()))
    ours = Seq2Seq(SyntheticTextProcessor(1000), lang_dec=lang_dec, tie_embed=tie_embed, **TOY)
    ours.load_state_dict(ref.state_dict())
    return ref, ours.cuda().eval()


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max()) / max(float(b.detach().abs().max()), 1e-30)


@pytest.mark.parametrize("lang_dec,tie_embed", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["shared", "lang_dec", "tie", "lang_dec_tie"])
def test_toy_score_fp32_against_oracle(cuda, lang_dec, tie_embed):
    ref, ours = _toy_pair(lang_dec, tie_embed)
    ours.set_compute_dtype(torch.float32)
    args = toy_batch(B=7, S=24, T=20, seed=8)
    for normalize in (True, False):
        want, want_tok = oracle_scores(ref, *args, normalize=normalize)
        got, tok, off = ours.score(*args, normalize=normalize, return_token_logprobs=True)
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == (7,)
        e = _rel(got, want)
        print("toy score lang_dec %d tie %d normalize %d: %.2e" % (lang_dec, tie_embed, normalize, e))
        assert e <= 1e-4, e
        mask = args[3][:, 1:]
        assert off.tolist() == [0] + torch.cumsum(mask.sum(1), 0).tolist()
        assert _rel(tok, want_tok[mask]) <= 1e-4
    # token log-probs == the gather from the existing forward(log_softmax=True)
    with torch.no_grad():
        lp = ours(*args, log_softmax=True)
    picked = lp.gather(1, args[1][:, 1:][args[3][:, 1:]].to(cuda).unsqueeze(1)).squeeze(1)
    assert _rel(tok, picked) <= 1e-4
    # a sentence without any non-pad target position scores 0 (and does not disturb the others)
    src, tgt, sm, tm, sl, tl = args
    tgt2, tm2 = tgt.clone(), tm.clone()
    tgt2[2, 1:], tm2[2, 1:] = 0, False
    got2 = ours.score(src, tgt2, sm, tm2, sl, tl)
    assert float(got2[2]) == 0.0
    keep = [0, 1, 3, 4, 5, 6]
    assert _rel(got2[keep], ours.score(*args)[keep]) <= 1e-5


def test_toy_score_candidates_indexed_to_encoded_sources(cuda):
    """encoder_states + src_index: several sources encoded once, candidates indexed to them, equals per-source calls."""
    ref, ours = _toy_pair(False, False)
    ours.set_compute_dtype(torch.float32)
    src, tgt, sm, tm, sl, tl = toy_batch(B=7, S=24, T=20, seed=8)
    src, sm, sl = src[:3], sm[:3], sl[:3]
    index = torch.tensor([0, 0, 1, 2, 2, 2, 1])
    enc = ours.encode(src, sm, ours._lang_grid(sl, src.size(1), cuda))[0]
    got = ours.score(None, tgt, sm, tm, None, tl, encoder_states=enc, src_index=index)
    want, _ = oracle_scores(ref, src[index], tgt, sm[index], tm, sl[index], tl)
    assert _rel(got, want) <= 1e-4
    for s in range(3):
        rows = (index == s).nonzero().view(-1)
        n = rows.numel()
        one = ours.score(src[s:s + 1].expand(n, -1), tgt[rows], sm[s:s + 1].expand(n, -1), tm[rows], sl[s:s + 1].expand(n), tl[rows])
        assert _rel(got[rows], one) <= 1e-5, s
    with pytest.raises(ValueError):
        ours.score(None, tgt, sm, tm, None, tl, encoder_states=enc)   # 3 sources, 7 targets, no index


@pytest.fixture(scope="module")
def c1_pair(cuda):
    from imagetranslate_amd.seq2seq import Seq2Seq
    torch.manual_seed(20)
    tp = R.SyntheticTextProcessor(C1_V)
    ref = R.Seq2Seq(tp, lang_dec=False, **C1).eval()
    with torch.no_grad():   # tests/test_gpu_c1.py's recipe
        for k, p in ref.named_parameters():
            if p.dim() > 1:
                p.mul_(2.0)
            elif k.endswith("bias"):
                p.normal_(0.0, 0.02)
    ours = Seq2Seq(tp, lang_dec=False, **C1)
    ours.load_state_dict(ref.state_dict())
    return ref, ours.cuda().eval()


_C1_ORACLE = {}


def _c1_oracle(ref, args, ragged, normalize):
    key = (ragged, normalize)
    if key not in _C1_ORACLE:
        _C1_ORACLE[key] = oracle_scores(ref, *args, normalize=normalize, rows_per_block=8)
    return _C1_ORACLE[key]


@pytest.mark.parametrize("ragged", [False, True], ids=["c1", "c1ragged"])
def test_c1_score_fp32_against_oracle(c1_pair, ragged):
    ref, ours = c1_pair
    ours.set_compute_dtype(torch.float32)
    args = c1_batch(ragged=ragged)
    for normalize in (True, False):
        want, want_tok = _c1_oracle(ref, args, ragged, normalize)
        (got, tok, off), kinds = _kinds_of_step(lambda: ours.score(*args, normalize=normalize, return_token_logprobs=True))
        e, e_tok = _rel(got, want), _rel(tok, want_tok[args[3][:, 1:]])
        print("C1 %s fp32 score normalize %d: %.2e (tokens %.2e)" % ("ragged" if ragged else "plain", normalize, e, e_tok))
        assert kinds.get("score_xl_f32", 0) == 1 and kinds.get("score_combine", 0) == 1 and "log_softmax_fwd" not in kinds, kinds
        assert e <= 1e-4 and e_tok <= 1e-4, (e, e_tok)


@pytest.mark.parametrize("ragged", [False, True], ids=["c1", "c1ragged"])
def test_c1_score_bf16_not_worse_than_the_existing_chain(c1_pair, ragged):
    """e_new = max |Seq2Seq.score - oracle|, e_old = the same for scores gathered from the existing bf16
    forward(log_softmax=True).  Required: e_new <= 1.25 e_old and e_new <= 4e-2 of the largest |score|."""
    ref, ours = c1_pair
    args = c1_batch(ragged=ragged)
    want, _ = _c1_oracle(ref, args, ragged, True)
    ours.set_compute_dtype(torch.bfloat16)
    try:
        (got, kinds) = _kinds_of_step(lambda: ours.score(*args))
        with torch.no_grad():
            lp = ours(*args, log_softmax=True)
        mask = args[3][:, 1:]
        picked = lp.gather(1, args[1][:, 1:][mask].to(lp.device).unsqueeze(1)).squeeze(1).double().cpu()
        counts = mask.sum(1)
        old = torch.stack([c.sum() for c in picked.split(counts.tolist())]) / counts
        del lp
    finally:
        ours.set_compute_dtype(torch.float32)
    e_new = float((got.double().cpu() - want.double()).abs().max())
    e_old = float((old - want.double()).abs().max())
    scale = float(want.abs().max())
    line = "C1 %s bf16: e_new %.4e  e_old %.4e  (largest |score| %.4f; e_new / e_old %.3f; e_new relative %.3e)" % (
        "ragged" if ragged else "plain", e_new, e_old, scale, e_new / max(e_old, 1e-30), e_new / scale)
    print(line)
    write_truth_log("score_parity_" + ("c1ragged" if ragged else "c1"), [line])   # beside the suite's other parity logs
    assert kinds.get("score_xl_bf16", 0) == 1 and kinds.get("score_combine", 0) == 1, kinds
    assert torch.isfinite(got).all()
    assert e_new <= 1.25 * e_old, line
    assert e_new <= 4e-2 * scale, line


# ------------------------------------------------------------------------------------------------ ranking and entry point
def _ranking_files(d):
    """Tokenizer on tests/golden/sample_enfa, a 2 + 2 layer model with beam_state_dict-scaled random weights saved with
    Seq2Seq.save, and marshal --sens / --data files: 18 sources (both directions), 3-8 candidates each."""
    import random
    from imagetranslate_amd import train_tokenizer
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import TextProcessor
    gold = os.path.join(os.path.dirname(__file__), "golden", "sample_enfa")
    en = [ln.strip() for ln in open(os.path.join(gold, "en.txt"), encoding="utf-8")]
    fa = [ln.strip() for ln in open(os.path.join(gold, "fa.txt"), encoding="utf-8")]
    with open(os.path.join(d, "all.txt"), "w", encoding="utf-8") as fw:
        fw.write("\n".join(["<en> " + s + " </s>" for s in en if s] + ["<fa> " + t + " </s>" for t in fa if t]) + "\n")
    tok = os.path.join(d, "tok")
    train_tokenizer.main(["--data", os.path.join(d, "all.txt"), "--vocab_size", "1000", "--model", tok])
    tp = TextProcessor(tok)
    rnd = random.Random(RANK_SEED)
    good = [i for i in range(len(en)) if 3 <= len(en[i].split()) <= 40 and 3 <= len(fa[i].split()) <= 40]
    sentences, src2dst = {}, {}
    for k in range(18):
        i = good[rnd.randrange(len(good))]
        a, b, ta, tb = (en, fa, "<en>", "<fa>") if k % 2 == 0 else (fa, en, "<fa>", "<en>")
        sid = 10 * k + 1
        sentences[sid] = "%s %s </s>" % (ta, a[i])
        cands = [i] + rnd.sample([j for j in good if j != i], rnd.randint(2, 7))
        rnd.shuffle(cands)
        tids = []
        for c, j in enumerate(cands):
            tid = 1000 + 10 * sid + c
            sentences[tid] = "%s %s </s>" % (tb, b[j])
            tids.append(tid)
        src2dst[sid] = tids
    torch.manual_seed(RANK_SEED)
    ref = R.Seq2Seq(tp, lang_dec=True, **TOY).eval()
    ref.load_state_dict(beam_state_dict(ref.state_dict()))
    ours = Seq2Seq(tp, lang_dec=True, **TOY)
    ours.load_state_dict(ref.state_dict())
    model_dir = os.path.join(d, "model")
    ours.save(model_dir)
    sens_file, data_file = os.path.join(d, "sens.marshal"), os.path.join(d, "data.marshal")
    with open(sens_file, "wb") as fw:
        marshal.dump(sentences, fw)
    with open(data_file, "wb") as fw:
        marshal.dump(src2dst, fw)
    return tp, ref, tok, model_dir, sens_file, data_file, sentences, src2dst


RANK_SEED = 32   # chosen on the CPU with the oracle alone: every source's top-2 gap is >= 10 x the tolerance (asserted below)


def test_score_pairs_entry_point_ranks_like_the_oracle(cuda, tmp_path, capsys):
    from imagetranslate_amd import score_pairs
    d = str(tmp_path)
    tp, ref, tok, model_dir, sens_file, data_file, sentences, src2dst = _ranking_files(d)
    assert len(src2dst) >= 16 and all(3 <= len(v) <= 8 for v in src2dst.values())
    assert {sentences[s].split(" ")[0] for s in src2dst} == {"<en>", "<fa>"}
    want = oracle_rank(ref, tp, sentences, src2dst)
    scale = max(abs(s) for _, _, table in want.values() for s in table.values())
    tol = 1e-4 * scale
    for sid, (_, _, table) in want.items():
        top = sorted(table.values(), reverse=True)
        assert top[0] - top[1] >= 10 * tol, "fixture: source %d has a top-2 gap of %.3g (< 10 x %.3g)" % (sid, top[0] - top[1], tol)

    def run(extra, name):
        out = os.path.join(d, name)
        stats = score_pairs.main(["--tok", tok, "--model", model_dir, "--sens", sens_file, "--data", data_file, "--output", out] + extra)
        assert not stats.get("failed_batches"), stats
        with open(out, encoding="utf-8") as fp:
            return [ln.split("\t") for ln in fp.read().split("\n") if ln]

    by_text = {sentences[sid]: sid for sid in src2dst}
    for capacity in ("2000", "1"):      # everything in one pack / several packs
        lines = run(["--fp32", "--capacity", capacity], "out_fp32_%s.txt" % capacity)
        assert [by_text[ln[0]] for ln in lines] == list(src2dst.keys()), "one line per source, in table order, none left out"
        for src_text, tgt_text, score in lines:
            best, best_score, _ = want[by_text[src_text]]
            assert tgt_text == sentences[best], (src_text, tgt_text, sentences[best])
            assert abs(float(score) - best_score) <= tol, (float(score), best_score)
            assert score == str(__import__("numpy").float32(float(score)))
    # the reference's window: 1-based index, index <= resume skipped, stop at index >= end
    lines = run(["--fp32", "--resume", "3", "--end", "9"], "out_window.txt")
    assert [by_text[ln[0]] for ln in lines] == list(src2dst.keys())[3:8]
    # bf16 (the default): completes, one finite score per source
    lines = run([], "out_bf16.txt")
    assert [by_text[ln[0]] for ln in lines] == list(src2dst.keys())
    assert all(math.isfinite(float(ln[2])) for ln in lines)
    # score_candidates: the same without files
    from imagetranslate_amd.seq2seq import Seq2Seq
    model = Seq2Seq.load(Seq2Seq, model_dir, tok_dir=tok).cuda().eval()
    model.set_compute_dtype(torch.float32)
    for sid, best, score, table in score_pairs.score_candidates(model, tp, sentences, src2dst, 2000):
        assert best == want[sid][0] and set(table) == set(src2dst[sid])
        for tid, s in table.items():
            assert abs(float(s) - want[sid][2][tid]) <= tol


def test_score_refused_where_it_is_not_implemented(cuda):
    from imagetranslate_amd.image_model import ImageCaptioning
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    tp = SyntheticTextProcessor(300)
    args = toy_batch(B=2, S=8, T=8, V=300)
    cap = ImageCaptioning(tp, lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4)
    with pytest.raises(NotImplementedError):
        cap.score(*args)
    prop = Seq2Seq(tp, lang_dec=False, use_proposals=True, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256,
                   num_attention_heads=4).cuda().eval()
    with pytest.raises(NotImplementedError):
        prop.score(*args)
