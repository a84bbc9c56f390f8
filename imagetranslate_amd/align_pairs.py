"""Word alignment of sentence pairs, and from it the ``--dict`` file of ``train_image_mt`` / ``train_captioning`` -- the step
the reference leaves to an external aligner (fast_align through src/scripts/align2fastalign.py / fastalign2align.py) followed by
src/build_alignment_dict.py, and the density filter of src/scripts/extract_dense_alignments.py.

The aligner here is the shared multilingual encoder: both sentences of a pair are encoded, ``imt_align_pairs`` takes the cosine
between their token states, the arg-max in both directions and keeps the mutual links ("argmax / intersection" of the
embedding-similarity aligners) without ever storing the similarities.  The language tag and ``</s>`` stay out through the
token ranges.  Words are the tokenizer's own (``Encoding.word_ids``); two words are linked iff any of their tokens are.

``--output`` receives one Pharaoh line (``i-j`` word links, sorted) per input pair, in input order; ``--token-output`` the same at
token level (positions in the tokenizer's encoding of the line); ``--dict-output`` the dictionary of the token links (key and
up to five translations per line, what ``dataset.get_lex_dict`` reads); ``--dense-output`` the ``src ||| dst`` lines whose word
links are at least ``--min-density`` of the longer side.  One process, one GPU."""
from collections import defaultdict
from optparse import OptionParser

import torch

from . import hip_ops as O
from .translate import build_batches

MODEL_TYPES = ("mt", "sensim", "lm")
MAX_LEN = 512


def get_option_parser():
    parser = OptionParser()
    parser.add_option("--tok", dest="tokenizer_path", type="string", default=None)
    parser.add_option("--model", dest="model_path", type="string", default=None)
    parser.add_option("--model-type", dest="model_type", type="choice", choices=list(MODEL_TYPES), default="mt")
    parser.add_option("--src", dest="src_path", type="string", default=None)
    parser.add_option("--dst", dest="dst_path", type="string", default=None)
    parser.add_option("--pairs", dest="pairs_path", type="string", default=None)
    parser.add_option("--src-lang", dest="src_lang", type="string", default=None)
    parser.add_option("--dst-lang", dest="dst_lang", type="string", default=None)
    parser.add_option("--output", dest="output", type="string", default=None)
    parser.add_option("--token-output", dest="token_output", type="string", default=None)
    parser.add_option("--dict-output", dest="dict_output", type="string", default=None)
    parser.add_option("--min-density", dest="min_density", type="float", default=None)
    parser.add_option("--dense-output", dest="dense_output", type="string", default=None)
    parser.add_option("--min-sim", dest="min_sim", type="float", default=0.0)
    parser.add_option("--batch", dest="batch", type="int", default=4000)
    parser.add_option("--fp32", dest="fp32", action="store_true", default=False)
    return parser


def check_options(options):
    """The combinations the entry point takes; ``ValueError`` otherwise."""
    for flag, val in (("--tok", options.tokenizer_path), ("--model", options.model_path), ("--src-lang", options.src_lang),
                      ("--dst-lang", options.dst_lang), ("--output", options.output)):
        if not val:
            raise ValueError("%s is required" % flag)
    if options.pairs_path:
        if options.src_path or options.dst_path:
            raise ValueError("--pairs replaces --src / --dst: give one or the other")
    elif not (options.src_path and options.dst_path):
        raise ValueError("--src and --dst (or --pairs) are required")
    if (options.min_density is None) != (options.dense_output is None):
        raise ValueError("--min-density and --dense-output go together")
    if options.batch < 1:
        raise ValueError("--batch must be positive")
    return options


# ---------------------------------------------------------------------------------------------- host rules
def word_links(token_links, src_word_ids, dst_word_ids):
    """Word links of one pair from its token links: (i, j) token positions -> sorted unique (word of i, word of j).  A token
    without a word (``None``: a special token) or beyond the word lists links nothing."""
    out = set()
    for i, j in token_links:
        if not (0 <= i < len(src_word_ids) and 0 <= j < len(dst_word_ids)):
            continue
        wi, wj = src_word_ids[i], dst_word_ids[j]
        if wi is not None and wj is not None:
            out.add((int(wi), int(wj)))
    return sorted(out)


def pharaoh_line(links):
    """``i-j`` pairs sorted by (i, j), blank-separated; the empty string for no links."""
    return " ".join("%d-%d" % (i, j) for i, j in sorted(set((int(i), int(j)) for i, j in links)))


def build_alignment_dict(src_seqs, dst_seqs, links):
    """src/build_alignment_dict.py:27-61 on sequences of ids: every link (i, j) of pair n counts ``src_seqs[n][i]`` as a
    translation of ``dst_seqs[n][j]`` and the reverse, in ONE table; a count is divided by its key's total; per key the five most
    probable translations, ties in the order they were first seen (a stable sort over insertion order).  Returns the rows
    ``[key, t1, ...]`` in the order the keys were first seen."""
    table = defaultdict(dict)
    total = defaultdict(int)
    for src, dst, pair_links in zip(src_seqs, dst_seqs, links):
        for i, j in pair_links:
            s, d = int(src[i]), int(dst[j])
            if d not in table[s]:    # (the reference tests one direction only and then sets both: a word linked to itself
                table[s][d] = 1      # is counted as the reference counts it)
                table[d][s] = 1
            else:
                table[s][d] += 1
                table[d][s] += 1
            total[s] += 1
            total[d] += 1
    rows = []
    for key in table.keys():
        denom = total[key]
        prob = [(t, c / denom) for t, c in table[key].items()]
        best = sorted(prob, key=lambda kv: kv[1], reverse=True)[:5]
        rows.append([key] + [t for t, _ in best])
    return rows


def write_alignment_dict(path, rows):
    with open(path, "w") as w:
        for row in rows:
            w.write(" ".join(str(v) for v in row) + "\n")


def len_condition(words1, words2):
    """src/scripts/extract_dense_alignments.py:4-5, with its operator precedence: the ratio test alone, OR all of the rest."""
    return bool(.9 <= len(words1) / len(words2) <= 1.1 or abs(len(words1) - len(words2)) <= 5 and len(words1) >= 5 and len(words2) >= 5)


def dense_pairs(src_words, dst_words, n_links, min_density):
    """src/scripts/extract_dense_alignments.py:21-23: links per word of the longer side at least ``min_density``, both sides
    of five words or more, and ``len_condition``.  ``n_links`` counts real links (the reference counts an empty alignment line
    as one link)."""
    density = n_links / max(len(src_words), len(dst_words))
    return bool(density >= min_density and len(src_words) >= 5 and len(dst_words) >= 5 and len_condition(src_words, dst_words))


# ---------------------------------------------------------------------------------------------- the model's part
def load_model(model_type, model_path, tok_dir):
    """(model, text_processor) of a saved ``ImageMassSeq2Seq`` (as translate.py loads it), ``SenSim`` or ``LM``."""
    from .textprocessor import TextProcessor
    tp = TextProcessor(tok_dir)
    if model_type == "mt":
        from .image_model import ImageMassSeq2Seq
        model = ImageMassSeq2Seq.load(ImageMassSeq2Seq, model_path, tok_dir=tok_dir, text_processor=tp)
    elif model_type == "sensim":
        from .sen_sim import SenSim
        model, _ = SenSim.load(model_path, tok_dir=tok_dir, text_processor=tp)
    elif model_type == "lm":
        from .lm import LM
        model = LM.load(model_path, text_processor=tp)
    else:
        raise ValueError("model type %r is not one of %s" % (model_type, MODEL_TYPES))
    return model, tp


def token_states(model, ids, mask, langs):
    """Encoder states [B, S, d] of the tokens.  A translation model gives them through ``encode(ids, mask, langs)``; ``SenSim``'s
    ``encode`` pools them away and ``LM`` has none, so those two are asked for their encoder stack's output, which is what
    ``Seq2Seq.encode`` returns too."""
    from .lm import LM
    from .sen_sim import SenSim
    if isinstance(model, (SenSim, LM)):
        device = model._device
        return model.encoder(ids.to(device), attention_mask=mask.to(device), token_type_ids=langs.to(device))
    return model.encode(ids, mask, langs)[0]


def _pad(ids_list, pad_idx):
    width = max(len(s) for s in ids_list)
    return torch.tensor([list(s) + [pad_idx] * (width - len(s)) for s in ids_list], dtype=torch.long)


@torch.no_grad()
def align_batch(model, src_ids, dst_ids, src_lang, dst_lang, pad_idx, min_sim=0.0, return_raw=False):
    """Token links of one batch of framed pairs (lists of ids: language tag first, ``</s>`` last unless the sentence was cut at
    512).  ``src_lang`` / ``dst_lang``: the language indices (token types).  Returns one sorted list of (i, j) per pair, positions
    counted WITHOUT the tag (position 0 is the first token of the tokenizer's encoding); with ``return_raw`` also the states,
    ranges and the op's outputs."""
    n = len(src_ids)
    assert n == len(dst_ids)
    if n == 0:
        return ([], None) if return_raw else []
    states, ranges = [], []
    for ids_list, lang in ((src_ids, src_lang), (dst_ids, dst_lang)):
        ids = _pad(ids_list, pad_idx)
        langs = torch.full(ids.shape, int(lang), dtype=torch.long)
        states.append(token_states(model, ids, ids != pad_idx, langs))
        # the tag is position 0; the last framed position is </s> unless the sentence filled all 512 places
        ranges.append(torch.tensor([[1, len(s) - 1 if len(s) < MAX_LEN else len(s)] for s in ids_list], dtype=torch.int32))
    dev = states[0].device
    xr, yr = ranges[0].to(dev), ranges[1].to(dev)
    out = O.align_pairs(states[0], states[1], xr, yr, min_sim)
    link = out[0].cpu()   # the one copy to the host; row-major nonzero order is (pair, source position) ascending
    rows, cols = torch.nonzero(link >= 0, as_tuple=True)
    links = [[] for _ in range(n)]
    for b, i, j in zip(rows.tolist(), cols.tolist(), link[rows, cols].tolist()):
        links[b].append((i - 1, j - 1))
    if return_raw:
        return links, dict(x=states[0], y=states[1], x_range=xr, y_range=yr, out=out)
    return links


def align_corpus(model, tp, src_lines, dst_lines, src_lang, dst_lang, batch=4000, min_sim=0.0):
    """Token links, token ids (without tag and ``</s>``) and word ids of every pair, in input order.  Pairs are sorted by length
    and packed to at most ``batch`` padded tokens per side."""
    src_tag, dst_tag = tp.token_id("<" + src_lang + ">"), tp.token_id("<" + dst_lang + ">")
    src_l, dst_l = tp.languages[tp.id2token(src_tag)], tp.languages[tp.id2token(dst_tag)]
    sep, pad = tp.token_id(tp.sep_token), tp.pad_token_id()
    enc = [(tp.tokenizer.encode(s.strip()), tp.tokenizer.encode(d.strip())) for s, d in zip(src_lines, dst_lines)]
    frame = lambda e, tag: ([tag] + list(e.ids) + [sep])[:MAX_LEN]   # tokenize_one_sentence_with_langid, keeping the Encoding
    framed = [(frame(es, src_tag), frame(ed, dst_tag)) for es, ed in enc]
    links = [None] * len(enc)
    # one length per pair (the longer side), so a batch holds at most `batch` padded tokens on either side
    longest = [[0] * max(len(fs), len(fd)) for fs, fd in framed]
    for idx, _, _, _ in build_batches(longest, batch, pad):
        res = align_batch(model, [framed[i][0] for i in idx], [framed[i][1] for i in idx], src_l, dst_l, pad, min_sim)
        for r, i in enumerate(idx):
            links[i] = res[r]
    tok_ids = [(list(es.ids)[:MAX_LEN - 1], list(ed.ids)[:MAX_LEN - 1]) for es, ed in enc]   # what the framed rows hold
    words = [(list(es.word_ids), list(ed.word_ids)) for es, ed in enc]
    return links, tok_ids, words


def read_pairs(options):
    """(source lines, target lines) from --src / --dst, or from the first two tab-separated fields of --pairs."""
    if options.pairs_path:
        src, dst = [], []
        with open(options.pairs_path, "r", encoding="utf-8") as fp:
            for ln in fp:
                if not ln.strip():
                    continue
                cols = ln.rstrip("\n").split("\t")
                if len(cols) < 2:
                    raise ValueError("--pairs: a line without a tab: %r" % ln)
                src.append(cols[0].strip())
                dst.append(cols[1].strip())
        return src, dst
    with open(options.src_path, "r", encoding="utf-8") as fs, open(options.dst_path, "r", encoding="utf-8") as fd:
        src, dst = [ln.strip() for ln in fs], [ln.strip() for ln in fd]
    if len(src) != len(dst):
        raise ValueError("--src has %d lines, --dst %d" % (len(src), len(dst)))
    return src, dst


def n_words(word_ids):
    ws = [w for w in word_ids if w is not None]
    return max(ws) + 1 if ws else 0


def write_outputs(options, src_lines, dst_lines, links, tok_ids, words):
    """Everything the entry point writes, from the token links; returns (pairs, word links, dense pairs)."""
    wl = [word_links(l, ws, wd) for l, (ws, wd) in zip(links, words)]
    with open(options.output, "w", encoding="utf-8") as w:
        for l in wl:
            w.write(pharaoh_line(l) + "\n")
    if options.token_output:
        with open(options.token_output, "w", encoding="utf-8") as w:
            for l in links:
                w.write(pharaoh_line(l) + "\n")
    if options.dict_output:
        write_alignment_dict(options.dict_output, build_alignment_dict([s for s, _ in tok_ids], [d for _, d in tok_ids], links))
    dense = 0
    if options.dense_output:
        with open(options.dense_output, "w", encoding="utf-8") as w:
            for s, d, l, (ws, wd) in zip(src_lines, dst_lines, wl, words):
                sw, dw = range(n_words(ws)), range(n_words(wd))   # the tokenizer's words, which the links index
                if len(sw) and len(dw) and dense_pairs(sw, dw, len(l), options.min_density):
                    w.write(s.strip() + " ||| " + d.strip() + "\n")
                    dense += 1
    return len(links), sum(len(l) for l in wl), dense


def align_pairs(options):
    check_options(options)
    model, tp = load_model(options.model_type, options.model_path, options.tokenizer_path)
    model.set_compute_dtype(torch.float32 if options.fp32 else torch.bfloat16)
    model = model.cuda().eval()
    src_lines, dst_lines = read_pairs(options)
    links, tok_ids, words = align_corpus(model, tp, src_lines, dst_lines, options.src_lang, options.dst_lang, options.batch,
                                         options.min_sim)
    return write_outputs(options, src_lines, dst_lines, links, tok_ids, words)


def main(argv=None):
    options, _ = get_option_parser().parse_args(argv)
    pairs, n_links, dense = align_pairs(options)
    print("pairs", pairs, "word links", n_links, "dense", dense)
    print("Finished!")


if __name__ == "__main__":
    main()
