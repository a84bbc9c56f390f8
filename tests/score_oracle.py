"""Checker for the scorer: ``src/score_pairs.py:96-127`` restated on ``oracle.reference_model.Seq2Seq`` (torch, CPU).

The reference scores the candidates of ONE source: it encodes the source, expands the encoder states over the candidates
(``:113-114``), runs the teacher-forced decoder on the full PADDED grid with ``future_mask`` (``:106, :116-118``), takes
``log_softmax`` of the output layer (``:119``), gathers the target ids (``:122-123``), masks the pad positions, sums per
sentence (``:126``) and divides by the number of non-pad positions (``:127``).  ``oracle_scores`` does exactly that for a
batch in which every target row has its own source row (the expanded form); ``oracle_rank`` runs it source by source over
a sentence table, as the reference's main loop does."""
import torch
import torch.nn.functional as F

from oracle import reference_model as R


@torch.no_grad()
def oracle_scores(ref, src_inputs, tgt_inputs, src_mask, tgt_mask, src_langs, tgt_langs, normalize=True, rows_per_block=16):
    """(scores [B], token log-probs [B, T-1] with zeros at pad positions).  The vocabulary projection runs in blocks of
    ``rows_per_block`` sentences so that a C1-size grid does not need one [B * (T-1), V] matrix; nothing else is chunked."""
    batch_lang = int(tgt_langs[0])
    src_langs_t = src_langs.unsqueeze(-1).expand(-1, src_inputs.size(-1))
    tgt_langs_t = tgt_langs.unsqueeze(-1).expand(-1, tgt_inputs.size(-1))
    encoder_states = ref.encode(src_inputs, src_mask, src_langs_t)[0]
    decoder = ref.decoder if not ref.lang_dec else ref.decoder[batch_lang]
    output_layer = ref.output_layer if (not ref.lang_dec) and ref.tie_embed else ref.output_layer[batch_lang]
    causal3d = R.future_mask(tgt_mask[:, :-1])
    hidden = decoder(encoder_states=encoder_states, input_ids=tgt_inputs[:, :-1], encoder_attention_mask=src_mask,
                             tgt_attention_mask=causal3d, token_type_ids=tgt_langs_t[:, :-1])
    B = tgt_inputs.size(0)
    tok_lp = torch.zeros(B, tgt_inputs.size(1) - 1, dtype=hidden.dtype)
    for b0 in range(0, B, rows_per_block):
        b1 = min(B, b0 + rows_per_block)
        logp = F.log_softmax(output_layer(hidden[b0:b1]), dim=-1)
        picked = logp.gather(2, tgt_inputs[b0:b1, 1:].unsqueeze(-1)).squeeze(-1)
        tok_lp[b0:b1] = picked * tgt_mask[b0:b1, 1:]
    total = tok_lp.sum(dim=1)
    if normalize:
        total = total / tgt_mask[:, 1:].sum(dim=-1)
    return total, tok_lp


@torch.no_grad()
def oracle_rank(ref, text_processor, sentences, src2dst, sids=None):
    """{sid: (best tid, best score, {tid: score})}: each source scored alone against its own candidates, the source row
    repeated per candidate (what ``expand`` does in the reference)."""
    pad = text_processor.pad_token_id()
    tok = lambda s: torch.tensor(text_processor.tokenize_one_sentence(s)[:512], dtype=torch.long)  # noqa: E731
    lang = lambda s: text_processor.lang_id(s.strip().split(" ")[0])  # noqa: E731
    out = {}
    for sid in (src2dst.keys() if sids is None else sids):
        tids = list(src2dst[sid])
        cands = torch.nn.utils.rnn.pad_sequence([tok(sentences[t]) for t in tids], batch_first=True, padding_value=pad)
        n = len(tids)
        src = tok(sentences[sid]).unsqueeze(0).expand(n, -1)
        scores, _ = oracle_scores(ref, src, cands, src != pad, cands != pad, torch.full((n,), lang(sentences[sid]), dtype=torch.long),
                                  torch.tensor([lang(sentences[t]) for t in tids], dtype=torch.long))
        table = {t: float(s) for t, s in zip(tids, scores)}
        best = max(tids, key=lambda t: table[t])  # the first of equal scores, as a stable descending sort
        out[sid] = (best, table[best], table)
    return out
