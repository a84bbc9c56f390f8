"""Plain-torch restatement of ImageMassSeq2Seq's image branches -- TEST INFRASTRUCTURE ONLY, written from the semantics of the
reference (src/image_model.py:185-230 gated text + image branch, :231-264 contrastive branch; src/seq_gen.py:105-106,180-188
text + image beam step) on top of oracle.reference_model and oracle.seq_gen.  Runs in whatever dtype the module is in
(``.double()`` for an fp64 truth).

  * The reference's ``encode`` keeps the (grid, objects) tuple its image head returns (:153 against :82) and the branch fails on
    it; the restatement takes element 0, the grid embeddings [B, 49, d], which is what :213 and :252 plainly mean.
  * Gated branch: the SAME decoder runs over the text encoder states (key mask src_pads) and over the image embeddings (no key
    mask), with tgt_mask = tgt_inputs != pad_idx, position_ids = tgt_positions[:, :-1], token types = the target language;
    out = s * text + (1 - s) * image, s = sigmoid(multimodal_attention_gate + 1e-7) (:217-219).
  * ``tgt_langs`` is read by both branches (:197, :235) but never passed by the reference trainer (src/train_image_mt.py:218-236):
    None means src_langs here, as in the product.
  * Contrastive branch: score = x . w + b, masked positions set to exactly -10000 (masked_fill, :241,246), softmax over
    positions, weighted sum, division by (|v|_2 + 1e-4) (:255-258); C = I [T_enc; T_neg]^T; loss = sum_i (log(sum_j exp C_ij +
    1e-4) - (C_ii + 1e-4)) / B (:260-263).  ``attn_pool_grads`` / ``contrastive_grads`` restate the closed forms the kernels
    compute; tests/test_multimodal.py holds them against autograd of the forwards in fp64.
  * Beam search: the image embeddings are repeated per beam like the encoder states (the reference omits that, :184, and can
    only run beam 1), src_langs is expanded over the source length as in the text route (:95).
"""
import torch
import torch.nn.functional as F

from oracle import reference_model as R
from oracle import seq_gen as OG


# ------------------------------------------------------------------------------------------------ contrastive tail
def attn_pool(x, w, b, mask=None):
    """(unit vector [rows, d], probabilities [rows, S], norm [rows]) of x [rows, S, d]; w [d], b scalar tensor, mask bool."""
    scores = x @ w + b
    if mask is not None:
        scores = scores.masked_fill(~mask, -10000.0)
    p = torch.softmax(scores, dim=1)
    v = torch.einsum("bfd,bf->bd", x, p)
    norm = torch.norm(v, dim=-1, p=2)
    return v / (norm.unsqueeze(-1) + 1e-4), p, norm


def attn_pool_grads(x, w, mask, u, p, norm, du):
    """(dx, dw, db) of attn_pool for an upstream du: dv = du / (r + eps) - u (du . u) / r; dp_s = dv . x_s;
    dscore = p (dp - sum p dp), zero at masked positions (their score is a constant); dx_s = p_s dv + dscore_s w."""
    r = norm.unsqueeze(-1)
    dv = du / (r + 1e-4) - u * (du * u).sum(-1, keepdim=True) / r
    dp = torch.einsum("bfd,bd->bf", x, dv)
    ds = p * (dp - (p * dp).sum(1, keepdim=True))
    if mask is not None:
        ds = ds.masked_fill(~mask, 0.0)
    dx = p.unsqueeze(-1) * dv.unsqueeze(1) + ds.unsqueeze(-1) * w
    return dx, torch.einsum("bf,bfd->d", ds, x), ds.sum()


def contrastive(img_u, txt_u):
    """:260-263; txt_u row i < B belongs to image i."""
    B = img_u.size(0)
    cross = img_u @ txt_u.t()
    denom = torch.log(torch.exp(cross).sum(-1) + 1e-4)
    nominator = torch.diagonal(cross[:, :B], 0) + 1e-4
    return (denom - nominator).sum() / B


def contrastive_grads(img_u, txt_u):
    """(d loss / d img_u, d loss / d txt_u) in closed form."""
    B = img_u.size(0)
    cross = img_u @ txt_u.t()
    e = torch.exp(cross)
    dc = e / (e.sum(-1, keepdim=True) + 1e-4)
    dc[:, :B] -= torch.eye(B, dtype=dc.dtype)
    dc = dc / B
    return dc @ txt_u, dc.t() @ img_u


# ------------------------------------------------------------------------------------------------ the model
class MultimodalSeq2Seq(R.ImageMassSeq2Seq):
    """R.ImageMassSeq2Seq plus the two image branches."""

    def mix(self, text_out, image_out):
        s = torch.sigmoid(self.multimodal_attention_gate + 1e-7)
        return s * text_out + (1 - s) * image_out

    def encode_both(self, src_inputs, src_pads, src_langs, images):
        src_langs_t = src_langs.unsqueeze(-1).expand(-1, src_inputs.size(-1))
        encoder_states = R.Seq2Seq.encode(self, src_inputs, src_pads, src_langs_t)[0]
        return encoder_states, self.image_model(images.to(encoder_states.dtype))[0]   # element 0 of (grid, objects)

    def forward(self, src_inputs=None, src_pads=None, tgt_inputs=None, src_langs=None, tgt_langs=None, pad_idx: int = 0,
                tgt_positions=None, batch=None, neg_samples=None, neg_mask=None, proposals=None, log_softmax: bool = False, **kw):
        if batch is None:
            return super().forward(src_inputs=src_inputs, src_pads=src_pads, tgt_inputs=tgt_inputs, src_langs=src_langs,
                                   tgt_langs=tgt_langs, pad_idx=pad_idx, tgt_positions=tgt_positions, log_softmax=log_softmax)
        encoder_states, image_embeddings = self.encode_both(src_inputs, src_pads, src_langs, batch["images"])
        langs = tgt_langs if tgt_langs is not None else src_langs
        lang = int(langs[0])
        if neg_samples is None:
            tgt_mask = tgt_inputs != pad_idx
            types = langs.unsqueeze(-1).expand(-1, tgt_inputs.size(-1))[:, :-1]
            pos = tgt_positions[:, :-1] if tgt_positions is not None else None
            args = dict(input_ids=tgt_inputs[:, :-1], tgt_attention_mask=R.future_mask(tgt_mask[:, :-1]), position_ids=pos,
                        token_type_ids=types)
            dec = self.decoder if not self.lang_dec else self.decoder[lang]
            out = self.mix(dec(encoder_states=encoder_states, encoder_attention_mask=src_pads, **args),
                           dec(encoder_states=image_embeddings, **args))
            if self.use_proposals:
                out = self.attend_proposal(out, proposals, pad_idx)
            sel = out.reshape(-1, out.size(-1))[tgt_mask[:, 1:].reshape(-1)]
            output_layer = self.output_layer if (not self.lang_dec) and self.tie_embed else self.output_layer[lang]
            logits = output_layer(sel)
            return F.log_softmax(logits, dim=-1) if log_softmax else logits
        neg_langs = langs[0].reshape(1, 1).expand(neg_samples.size(0), neg_samples.size(-1))
        neg_states = R.Seq2Seq.encode(self, neg_samples, neg_mask, neg_langs)[0]
        we, be = self.encoder_attention_w.weight[0], self.encoder_attention_w.bias[0]
        t_neg = attn_pool(neg_states, we, be, neg_mask)[0]
        t_enc = attn_pool(encoder_states, we, be, src_pads)[0]
        i_u = attn_pool(image_embeddings, self.image_attention_w.weight[0], self.image_attention_w.bias[0])[0]
        return contrastive(i_u, torch.cat([t_enc, t_neg]))


# ------------------------------------------------------------------------------------------------ beam search
class _Blended(torch.nn.Module):
    """The decoder over the text states and over the image states behind one decoder call: what oracle.seq_gen sees."""

    def __init__(self, model, dec, img_states):
        super().__init__()
        self.model, self.dec, self.img_states = model, dec, img_states

    def forward(self, encoder_states=None, **kw):
        out = self.dec(encoder_states=encoder_states, **kw)
        rep = encoder_states.size(0) // self.img_states.size(0)
        img = self.img_states if rep == 1 else torch.repeat_interleave(self.img_states, rep, 0)
        kw["encoder_attention_mask"] = None
        return self.model.mix(out, self.dec(encoder_states=img, **kw))


class _Proxy:
    def __init__(self, model, decoder):
        self._model, self.decoder = model, decoder

    def __getattr__(self, name):
        return getattr(self._model, name)


@torch.no_grad()
def beam_search(model, images, beam_width, max_len=None, **kw):
    """Text + image beam search (src/seq_gen.py:105-106,180-188) through oracle.seq_gen's text route with a blended decoder;
    ``max_len`` defaults to 512 as whenever images are given (:85-86)."""
    img = model.image_model(images)[0]
    if model.lang_dec:
        dec = [_Blended(model, d, img) for d in model.decoder]
    else:
        dec = _Blended(model, model.decoder, img)
    return OG.BeamDecoder(_Proxy(model, dec), beam_width=beam_width)(max_len=512 if max_len is None else max_len, **kw)
