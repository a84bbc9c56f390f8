"""Sentence-pair mining -- the step the reference does for its comparable corpora with src/comparable/ (score candidate pairs,
then keep a pair only if each side is the other's best, ``extract_best_comparable.py``): a saved ``SenSim`` encodes the sentences
of two monolingual batch directories (``--src``, ``--dst``: example files as ``create_batches`` writes them, what ``MassDataset``
reads) to unit vectors, ``imt_knn_rows`` finds every sentence's ``--k`` nearest neighbours on the other side in both directions
without the [N, M] similarity matrix, and ``--output`` receives one ``source \\t target \\t score`` line per pair that is each
other's best, best first.  ``--margin none`` scores a pair by its cosine; ``--margin ratio`` (default) by Artetxe & Schwenk's ratio
margin, the cosine over the mean of the two sides' average similarity to their k neighbours.  The reference's division by the
sentence length belongs to its word-sum score and is not taken over.  One process, one GPU."""
import os

import numpy as np
import torch

from . import dataset
from . import hip_ops as O
from .option_parser import get_img_options_parser
from .sen_sim import SenSim
from .seq_gen import get_outputs_until_eos

MARGINS = ("none", "ratio")
MIN_DENOMINATOR = 1e-6


def get_option_parser():
    parser = get_img_options_parser()
    parser.add_option("--src", dest="src_dir", type="string", default=None)
    parser.add_option("--dst", dest="dst_dir", type="string", default=None)
    parser.add_option("--k", dest="k", type="int", default=4)
    parser.add_option("--margin", dest="margin", type="choice", choices=list(MARGINS), default="ratio")
    parser.add_option("--min", dest="min_score", type="float", default=0.0)
    parser.add_option("--bf16-search", dest="bf16_search", action="store_true", default=False)
    return parser


@torch.no_grad()
def encode_corpus(model, data):
    """(unit vectors [n, d] fp32 on the model's device, the sentences' token ids in corpus order: one 1-D tensor each)."""
    pad = model.text_processor.pad_token_id()
    vecs, ids = [], []
    for i in range(len(data)):
        batch = data[i]
        texts = batch["src_texts"]
        vecs.append(model.encode_unit(texts, texts != pad, batch["langs"]))
        ids += list(texts)
    if not vecs:
        return torch.empty((0, model.embed_dim), device=model._device, dtype=torch.float32), ids
    return torch.cat(vecs), ids


def _best_of(score, neighbour):
    """Per row of ``score`` [n, k]: the place of the highest score, ties to the lowest ``neighbour`` index."""
    top = score.max(dim=1, keepdim=True).values
    cand = torch.where(score == top, neighbour, torch.full_like(neighbour, torch.iinfo(torch.int64).max))
    return cand.argmin(dim=1)


def select_pairs(fwd_val, fwd_idx, bwd_val, bwd_idx, margin="ratio", min_score=0.0):
    """The tail of ``mine`` on the two neighbour lists (``knn_rows(src, tgt, k)`` and ``knn_rows(tgt, src, k)``; any device, the
    arithmetic is fp64): (src_idx, tgt_idx, score) as numpy arrays, by score descending, then (s, t) ascending.  A pair is kept
    iff t is s's best, s is t's best (indices only) and score >= min_score."""
    if margin not in MARGINS:
        raise ValueError("margin %r is not one of %s" % (margin, MARGINS))
    N, k = fwd_val.shape
    M = bwd_val.shape[0]
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64))
    if N == 0 or M == 0:
        return empty
    fv, bv = fwd_val.double(), bwd_val.double()
    fi, bi = fwd_idx.long(), bwd_idx.long()
    if margin == "none":
        s_best, s_score = fi[:, 0], fv[:, 0]
        t_best = bi[:, 0]
    else:
        a = fv[:, :min(k, M)].mean(dim=1)   # [N] a source's mean similarity to its neighbours
        b = bv[:, :min(k, N)].mean(dim=1)   # [M]
        ninf = torch.full_like(fv[:1, :1], float("-inf"))

        def scores(val, idx, mine, theirs):
            ok = idx >= 0
            den = (mine.unsqueeze(1) + theirs[idx.clamp(min=0)]) / 2
            ok = ok & (den > MIN_DENOMINATOR)
            return torch.where(ok, val / torch.where(ok, den, torch.ones_like(den)), ninf)

        fs, bs = scores(fv, fi, a, b), scores(bv, bi, b, a)
        fj, bj = _best_of(fs, fi), _best_of(bs, bi)
        rows_n, rows_m = torch.arange(N, device=fv.device), torch.arange(M, device=bv.device)
        s_best, s_score = fi[rows_n, fj], fs[rows_n, fj]
        s_best = torch.where(torch.isinf(s_score), torch.full_like(s_best, -1), s_best)   # no candidate at all
        t_best = bi[rows_m, bj]
        t_best = torch.where(torch.isinf(bs[rows_m, bj]), torch.full_like(t_best, -1), t_best)
    s = torch.arange(N, device=fv.device)
    keep = (s_best >= 0) & (t_best[s_best.clamp(min=0)] == s) & (s_score >= min_score)
    s, t, sc = s[keep].cpu().numpy(), s_best[keep].cpu().numpy(), s_score[keep].cpu().numpy()
    order = np.lexsort((t, s, -sc))
    return s[order], t[order], sc[order]


def mine(src_u, tgt_u, k=4, margin="ratio", min_score=0.0):
    """Mutual-best pairs of two sets of unit vectors (fp32 or bf16, on the GPU): (src_idx, tgt_idx, score) on the host."""
    fwd_val, fwd_idx = O.knn_rows(src_u, tgt_u, k)
    bwd_val, bwd_idx = O.knn_rows(tgt_u, src_u, k)
    return select_pairs(fwd_val, fwd_idx, bwd_val, bwd_idx, margin, min_score)


def _as_dir(path):
    return path + os.sep if os.path.isdir(path) and not path.endswith(os.sep) else path


def mine_pairs(options):
    """The entry point's work; returns the number of pairs written."""
    for flag, val in (("--model", options.model_path), ("--src", options.src_dir), ("--dst", options.dst_dir),
                      ("--output", options.output)):
        if not val:
            raise ValueError("%s is required" % flag)
    model, tp = SenSim.load(options.model_path, tok_dir=options.tokenizer_path)
    model = model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16).eval()
    load = lambda path: dataset.MassDataset(batch_pickle_dir=_as_dir(path), max_batch_capacity=options.total_capacity,
                                            max_batch=options.batch, pad_idx=tp.pad_token_id(), keep_pad_idx=False,
                                            max_seq_len=options.max_seq_len, keep_examples=False)
    src_u, src_ids = encode_corpus(model, load(options.src_dir))
    tgt_u, tgt_ids = encode_corpus(model, load(options.dst_dir))
    print("sentences", len(src_ids), len(tgt_ids), flush=True)
    if options.bf16_search:
        src_u, tgt_u = src_u.bfloat16(), tgt_u.bfloat16()
    s_idx, t_idx, score = mine(src_u, tgt_u, options.k, options.margin, options.min_score)
    decode = lambda ids: tp.tokenizer.decode(get_outputs_until_eos(tp.sep_token_id(), ids, remove_first_token=True)[0].numpy())
    with open(options.output, "w", encoding="utf-8") as w:
        for s, t, v in zip(s_idx, t_idx, score):
            w.write(decode(src_ids[int(s)]) + "\t" + decode(tgt_ids[int(t)]) + "\t" + str(float(v)) + "\n")
    return len(score)


def main(argv=None):
    options, _ = get_option_parser().parse_args(argv)
    n = mine_pairs(options)
    print("pairs", n)
    print("Finished!")


if __name__ == "__main__":
    main()
