"""Sentence mining end to end on the GPU: a toy SenSim (2 layers, d = 64, seeded) encodes two monolingual batch directories of
about 150 sentences each, ``python -m imagetranslate_amd.mine_pairs`` writes the mutual-best pairs, and every claim the output
makes is checked against fp64 similarities of the encoded vectors (tests/mine_oracle.py).  A randomly initialised encoder gives
crowded vectors, so the checks are tolerance-aware and not index-exact: 1e-4, the project's fp32 bar on cosines."""
import os

import numpy as np
import pytest
import torch

from tests import mine_oracle as MO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-4
K = 4


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(directory, tokenizer directory, text processor, saved model directory): the tokenizer of tests/golden/marshal_kat, 160
    lines of tests/golden/sample_enfa per side written by the package's own batch writer."""
    from imagetranslate_amd import create_mt_batches as C
    from imagetranslate_amd.sen_sim import SenSim
    from imagetranslate_amd.textprocessor import TextProcessor
    d = str(tmp_path_factory.mktemp("mine"))
    tok = os.path.join(GOLD, "marshal_kat", "tok")
    tp = TextProcessor(tok)
    lines = open(os.path.join(GOLD, "sample_enfa", "en.txt"), encoding="utf-8").read().split("\n")
    # the target side: half of the source sentences again (in reverse order, under the other language tag, so a pair's cosine
    # is high but not 1) among as many sentences the source side does not have -- mutual-best pairs exist, rivals too
    for side, tag, part in (("src", "<en>", lines[:160]), ("dst", "<fa>", lines[80:240][::-1])):
        with open(os.path.join(d, side + ".txt"), "w", encoding="utf-8") as fw:
            fw.write("\n".join(part) + "\n")
        os.makedirs(os.path.join(d, side))
        n = C.write(tp, os.path.join(d, side, "part"), os.path.join(d, side + ".txt"), tp.token_id(tag))
        assert n > 100
    torch.manual_seed(21)
    model = SenSim(tp, enc_layer=2, embed_dim=64, intermediate_dim=256, num_attention_heads=2)
    with torch.no_grad():
        model.input_attention.weight.mul_(3.0)   # pooling weights away from uniform
    out = os.path.join(d, "sim")
    model.save(out)
    return d, tok, tp, out


def _load(corpus):
    from imagetranslate_amd.dataset import MassDataset
    from imagetranslate_amd.sen_sim import SenSim
    d, tok, tp, out = corpus
    model, _ = SenSim.load(out, tok)
    model = model.set_compute_dtype(torch.float32).eval()
    data = lambda side: MassDataset(batch_pickle_dir=os.path.join(d, side) + os.sep, max_batch_capacity=50, max_batch=6000,
                                    pad_idx=tp.pad_token_id(), keep_pad_idx=False, max_seq_len=175, keep_examples=False)
    return model, data("src"), data("dst")


def test_encode_unit_is_encode_over_its_norm(cuda, corpus):
    model, src, _ = _load(corpus)
    assert len(src) > 1, "more than one batch"
    b = src[0]
    texts, langs = b["src_texts"], b["langs"]
    mask = texts != 0
    v = model.encode(texts, mask, langs.unsqueeze(-1).expand(-1, texts.size(-1)))
    want = v / (v.norm(dim=-1, keepdim=True) + 1e-4)
    for lg in (langs, langs.unsqueeze(-1).expand(-1, texts.size(-1))):   # per sentence, per position
        u = model.encode_unit(texts, mask, lg)
        assert u.dtype == torch.float32 and not u.requires_grad and tuple(u.shape) == (texts.size(0), 64)
        err = float((u - want).abs().max())
        assert err <= 1e-5, err
    assert float((u.norm(dim=-1) - 1.0).abs().max()) < 1e-3


def _runner_up(scores, cands, skip):
    best = -np.inf
    for j in cands:
        if j != skip and scores[j] > best:
            best = scores[j]
    return best


@pytest.mark.parametrize("margin", ["none", "ratio"])
def test_mine_pairs_end_to_end_against_fp64(cuda, corpus, margin, capsys):
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd import mine_pairs as P
    from imagetranslate_amd.seq_gen import get_outputs_until_eos
    d, tok, tp, out = corpus
    model, src, dst = _load(corpus)
    src_u, src_ids = P.encode_corpus(model, src)
    tgt_u, tgt_ids = P.encode_corpus(model, dst)
    N, M = len(src_ids), len(tgt_ids)
    assert tuple(src_u.shape) == (N, 64) and tuple(tgt_u.shape) == (M, 64) and N > 100 and M > 100
    assert sum(b["src_texts"].size(0) for b in src.batches) == N, "corpus order: the batches' rows, one after the other"
    sim = MO.similarities(src_u.cpu().numpy(), tgt_u.cpu().numpy())
    score, fwd, bwd = MO.rule_scores(sim, K, margin)
    everything = MO.mine_reference(sim, K, margin, -np.inf)
    assert len(everything) >= 4
    min_score = float(np.median([r[2] for r in everything]))   # about half of the mutual-best pairs fall below --min

    path = os.path.join(d, "pairs_%s.txt" % margin)
    P.main(["--model", out, "--tok", tok, "--src", os.path.join(d, "src"), "--dst", os.path.join(d, "dst"), "--output", path,
            "--k", str(K), "--margin", margin, "--min", repr(min_score), "--batch", "6000", "--capacity", "50", "--fp32"])
    assert "pairs" in capsys.readouterr().out
    lines = open(path, encoding="utf-8").read().split("\n")
    assert lines[-1] == "" and len(lines) > 1
    rows = [ln.split("\t") for ln in lines[:-1]]
    assert all(len(r) == 3 for r in rows), "source TAB target TAB score"

    # the same run through the importable functions: the file is its formatting
    s_idx, t_idx, sc = P.mine(src_u, tgt_u, K, margin, min_score)
    assert len(rows) == len(sc) >= 1
    text = lambda ids: tp.tokenizer.decode(get_outputs_until_eos(tp.sep_token_id(), ids, remove_first_token=True)[0].numpy())
    for r, s, t, v in zip(rows, s_idx, t_idx, sc):
        assert r[0] == text(src_ids[int(s)]) and r[1] == text(tgt_ids[int(t)]) and float(r[2]) == float(v)
    first = src_ids[int(s_idx[0])]
    ids = first[first != 0].tolist()
    assert rows[0][0] == tp.tokenizer.decode(np.array(ids[1:ids.index(tp.sep_token_id())])), "until </s>, language tag removed"
    keys = [(-float(v), int(s), int(t)) for s, t, v in zip(s_idx, t_idx, sc)]
    assert keys == sorted(keys), "by score descending, then (s, t) ascending"
    assert len(set(s_idx.tolist())) == len(s_idx) and len(set(t_idx.tolist())) == len(t_idx), "a sentence is in one pair at most"

    fval, fidx = O.knn_rows(src_u, tgt_u, K)
    fval, fidx = fval.cpu().numpy(), fidx.cpu().numpy()
    got = set()
    for s, t, v in zip(s_idx.tolist(), t_idx.tolist(), sc.tolist()):
        got.add((s, t))
        at = np.flatnonzero(fidx[s] == t)
        assert len(at) == 1, "the target is one of the source's forward neighbours"
        assert abs(float(fval[s, at[0]]) - sim[s, t]) <= TOL, "the pair's cosine against fp64"
        assert abs(v - score[s, t]) <= TOL * max(1.0, abs(score[s, t])), "the pair's score against the rule in fp64"
        assert v >= min_score
        # no rival on either side beats the pair by more than the tolerance in the rule's score
        assert score[s, fwd[s]].max() - score[s, t] <= TOL, ("a better target", s, t)
        assert score[bwd[:, t], t].max() - score[s, t] <= TOL, ("a better source", s, t)
    # every pair the oracle keeps with a clear lead on both sides and a score clear of --min is there
    clear = 0
    for s, t, v in MO.mine_reference(sim, K, margin, min_score):
        lead_s = v - _runner_up(score[s], np.flatnonzero(fwd[s]), t)
        lead_t = v - _runner_up(score[:, t], np.flatnonzero(bwd[:, t]), s)
        if lead_s > TOL and lead_t > TOL and v > min_score + TOL:
            clear += 1
            assert (s, t) in got, ("missing", s, t, v)
    print("\n[mine %s] %d x %d sentences, %d pairs written, %d of the oracle's are clear of the tolerance" % (margin, N, M, len(got), clear))
    assert clear >= 1
