"""Score given translation candidates and keep the best one per source -- counterpart of ``src/score_pairs.py``.

Same command line (``--tok --model --fp16 --capacity --data --sens --output --resume --end``, ``src/score_pairs.py:15-27``)
plus ``--fp32`` as in ``translate.py``; same files (``--sens``: a marshal of the sentence table, every sentence starting
with its language tag; ``--data``: a marshal of ``{source id: target ids}``); same tokenisation
(``tokenize_one_sentence(s)[:512]``); same ``--resume`` / ``--end`` window (1-based index over the sources: ``index <=
resume`` is skipped, the run stops at ``index >= end > 0``); same score (mean log-probability of the candidate's tokens
under the teacher-forced decoder, ``:116-127``) and the same output line ``source \\t best target \\t score`` with the score
printed as ``str(numpy.float32)``.

Differences from the reference, all deliberate:

* the model is loaded with this package's ``Seq2Seq.load`` (no apex); it computes in bf16 unless ``--fp32`` is given
  (``--fp16`` is accepted and means bf16, the default);
* consecutive sources are PACKED into one launch: one encoder batch for the sources of a pack, every candidate indexed
  to its source (``Seq2Seq.score(encoder_states=..., src_index=...)``).  A pack grows while the reference's own work
  estimate ``2 * max(S, T)^3 * candidates`` (``:84-85``), summed over its sources, stays within ``--capacity`` million; a
  single source over the cap is split over its candidates as the reference does (``:86-91``);
* the candidates of a pack are grouped by target language, one decoder call per language, so that the decoder and output
  layer a call uses (``batch_lang``) is the right one for each of its rows;
* a batch that raises ``RuntimeError`` is reported on stderr with its source ids and counted (the reference drops it
  silently, ``:137-138``).
"""
import marshal
import math
import sys
from optparse import OptionParser

import numpy as np
import torch


# (flag, dest, kind, default): names and values of src/score_pairs.py:15-27, then the build addition --fp32
OPTIONS = [
    ("--tok", "tokenizer_path", "str", None), ("--model", "model", "str", None), ("--fp16", "fp16", "flag", False),
    ("--capacity", "total_capacity", "int", 2000), ("--data", "data", "str", None), ("--sens", "sens", "str", None),
    ("--output", "output", "str", None), ("--resume", "resume_index", "int", 0), ("--end", "end_index", "int", -1),
    ("--fp32", "fp32", "flag", False),
]


def get_option_parser():
    from .option_parser import _add
    return _add(OptionParser(), OPTIONS)


def window(src2dst, resume=0, end=-1):
    """Source ids of the reference's ``--resume`` / ``--end`` window, in table order (``src/score_pairs.py:39-44``)."""
    index = 0
    for sid in src2dst.keys():
        index += 1
        if index >= end and end > 0:
            break
        if index <= resume:
            continue
        yield sid


def work_estimate(src_len, cand_width, n_cand):
    """The reference's capacity measure of one source with its candidates (``src/score_pairs.py:84-85``)."""
    return 2 * (max(int(src_len), int(cand_width)) ** 3) * int(n_cand)


def make_packs(entries, max_capacity):
    """Group sources into launches.  ``entries``: iterable of ``(sid, src_ids, src_lang, tids, cand_ids, cand_langs)``
    (token-id lists; one language id per candidate).  Yields packs = lists of such tuples.  Consecutive sources share a
    pack while the sum of their work estimates stays within ``max_capacity``; a source that exceeds it alone becomes packs
    of its own, its candidates split into equal runs exactly as ``src/score_pairs.py:86-91`` does."""
    pack, used = [], 0
    for sid, src_ids, src_lang, tids, cands, langs in entries:
        if not tids:
            continue
        est = work_estimate(len(src_ids), max(len(c) for c in cands), len(tids))
        if est > max_capacity:
            if pack:
                yield pack
                pack, used = [], 0
            n_split = int(math.ceil(est / max_capacity))
            size = max(1, int(math.floor(len(tids) / n_split)))
            for i in range(0, len(tids), size):
                yield [(sid, src_ids, src_lang, tids[i:i + size], cands[i:i + size], langs[i:i + size])]
            continue
        if pack and used + est > max_capacity:
            yield pack
            pack, used = [], 0
        pack.append((sid, src_ids, src_lang, tids, cands, langs))
        used += est
    if pack:
        yield pack


def decoder_calls(pack):
    """The decoder calls of a pack: ``{target language: [(index of the source in the pack, tid, candidate ids), ...]}`` in
    order of first appearance -- one language per call."""
    calls = {}
    for k, (_, _, _, tids, cands, langs) in enumerate(pack):
        for tid, ids, lang in zip(tids, cands, langs):
            calls.setdefault(int(lang), []).append((k, tid, ids))
    return calls


def _pad(rows, pad_idx):
    width = max(len(r) for r in rows)
    out = torch.full((len(rows), width), pad_idx, dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    return out


@torch.no_grad()
def score_pack(model, pack, pad_idx):
    """``{(source index in the pack, tid): score}`` of one pack: one encoder batch, one ``Seq2Seq.score`` per language."""
    device = model._device
    src = _pad([p[1] for p in pack], pad_idx).to(device)
    src_mask = src != pad_idx
    src_langs = model._lang_grid(torch.tensor([int(p[2]) for p in pack], dtype=torch.long), src.size(1), device)
    encoder_states = model.encode(src, src_mask, src_langs)[0]
    out = {}
    for lang, rows in decoder_calls(pack).items():
        tgt = _pad([r[2] for r in rows], pad_idx).to(device)
        scores = model.score(None, tgt, src_mask, tgt != pad_idx, None, torch.full((len(rows),), lang, dtype=torch.long),
                             normalize=True, encoder_states=encoder_states,
                             src_index=torch.tensor([r[0] for r in rows], dtype=torch.long))
        for (k, tid, _), s in zip(rows, scores.float().cpu().numpy()):
            out[(k, tid)] = s
    return out


def score_candidates(model, text_processor, sentences, src2dst, capacity, resume=0, end=-1, stats=None):
    """Yield ``(sid, best_tid, score, {tid: score})`` for every source of the window, in table order.  ``capacity`` in
    millions as ``--capacity``.  ``stats`` (optional dict): ``failed_batches`` / ``failed_sources`` are counted there."""
    tok = lambda s: text_processor.tokenize_one_sentence(s)[:512]  # noqa: E731  (src/score_pairs.py:30)
    lang_of = lambda s: text_processor.lang_id(s.strip().split(" ")[0])  # noqa: E731
    pad_idx = text_processor.pad_token_id()
    if stats is None:
        stats = {}
    stats.setdefault("failed_batches", 0)
    stats.setdefault("failed_sources", 0)

    def entries():
        for sid in window(src2dst, resume, end):
            tids = list(src2dst[sid])
            yield (sid, tok(sentences[sid]), lang_of(sentences[sid]), tids, [tok(sentences[t]) for t in tids],
                   [lang_of(sentences[t]) for t in tids])

    pending = {}  # sid -> [scores so far, candidates still missing]  (a split source spans several packs)
    failed = set()
    for pack in make_packs(entries(), int(capacity) * 1000000):
        if all(p[0] in failed for p in pack):
            continue  # a later part of a split source whose earlier part failed
        for sid, _, _, tids, _, _ in pack:
            pending.setdefault(sid, [{}, len(src2dst[sid])])
        try:
            got = score_pack(model, pack, pad_idx)
        except RuntimeError as e:
            sids = [p[0] for p in pack]
            stats["failed_batches"] += 1
            stats["failed_sources"] += len(sids)
            failed.update(sids)
            print("score_pairs: batch of sources %s failed: %s" % (sids, e), file=sys.stderr)
            for s in sids:
                pending.pop(s, None)
            continue
        for (k, tid), s in got.items():
            sid = pack[k][0]
            if sid in pending:
                pending[sid][0][tid] = s
        for sid, _, _, tids, _, _ in pack:
            if sid not in pending:
                continue
            pending[sid][1] -= len(tids)
            if pending[sid][1] <= 0:
                scores = pending.pop(sid)[0]
                best = None
                for tid in src2dst[sid]:  # the first of equal scores wins, as a stable descending sort (:131)
                    if tid in scores and (best is None or scores[tid] > scores[best]):
                        best = tid
                yield sid, best, scores[best], scores


def main(argv=None):
    options, _ = get_option_parser().parse_args(argv)
    from .seq2seq import Seq2Seq
    from .textprocessor import TextProcessor
    print("Loading text processor...")
    text_processor = TextProcessor(options.tokenizer_path)
    print("Loading model...")
    model = Seq2Seq.load(Seq2Seq, options.model, tok_dir=options.tokenizer_path)
    model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16)
    model = model.cuda().eval()
    print("Loading data...")
    with open(options.sens, "rb") as fp, open(options.data, "rb") as fp2:
        sentences = marshal.load(fp)
        src2dst = marshal.load(fp2)
    print(len(src2dst))
    print("Scoring candidates")
    stats = {}
    with open(options.output, "w") as writer:
        for i, (sid, tid, score, _) in enumerate(score_candidates(model, text_processor, sentences, src2dst, options.total_capacity,
                                                                 options.resume_index, options.end_index, stats)):
            writer.write(sentences[sid] + "\t" + sentences[tid] + "\t" + str(np.float32(score)))
            writer.write("\n")
            print(options.resume_index + i + 1, len(src2dst), end="\r")
    if stats.get("failed_batches"):
        print("\nscore_pairs: %d batches (%d sources) failed and were left out" % (stats["failed_batches"], stats["failed_sources"]),
              file=sys.stderr)
    print("\nDone!")
    return stats


if __name__ == "__main__":
    main()
