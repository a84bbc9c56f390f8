"""Plain-torch restatement of ImageCaptioning's object stream -- TEST INFRASTRUCTURE ONLY, written from the semantics of the
reference (src/image_model.py:44-82 object rows, :279-296 obj_decoder / ties / gate, :357-366 second pass + gate;
src/seq_gen.py:164-180 beam search) on top of oracle.reference_model and oracle.seq_gen.

  * object row = [object_embedding[label] | box feature (1024) | locs (7)], locs = x1/800, x2/800, y1/800, y2/800, w, h, w*h
    (boxes x1, y1, x2, y2; :61-69); a label-0 row is zero whole (:75); object_fc = relu(object_feat_fc(row)) (:76), no bias;
    dropout in training (:78-81).
  * obj_decoder is built from the encoder's config (enc_layer layers, :281,287); no key mask over the object rows (captioning
    passes src_pads = None); out = s * dec + (1 - s) * obj with s = sigmoid(multistream_attention_gate + 1e-7) (:362-366).
  * beam search: the object rows are repeated per beam from step 2 on, exactly like the image states (:171-174).
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import reference_model as R
from oracle import seq_gen as OG

FEAT, LABELS = 1024, 91


def object_rows(emb_weight, labels, feats, boxes):
    x1, y1, x2, y2 = (boxes[..., i] / 800 for i in range(4))
    w, h = x2 - x1, y2 - y1
    locs = torch.stack([x1, x2, y1, y2, w, h, w * h], dim=-1).to(emb_weight.dtype)
    rows = torch.cat([emb_weight[labels], feats.to(emb_weight.dtype), locs], dim=-1)
    return torch.where((labels == 0).unsqueeze(-1), torch.zeros_like(rows), rows)


def object_fc(head, objects):
    rows = object_rows(head.object_embedding.weight, objects["labels"], objects["feats"], objects["boxes"])
    out = F.relu(F.linear(rows, head.object_feat_fc.weight))
    if head.dropout > 0 and head.training:
        out = F.dropout(out, p=head.dropout)
    return out


class ObjImageCaptioning(R.ImageCaptioning):
    """R.ImageCaptioning (use_obj=False form) plus the object stream."""

    def __init__(self, text_processor, **kw):
        kw.pop("use_obj", None)
        super().__init__(text_processor, **kw)
        d = self.config.hidden_size
        self.image_model.object_feat_fc = nn.Linear(d + FEAT + 7, d, bias=False)
        self.image_model.object_embedding = nn.Embedding(LABELS, d)
        tie = R._Pretrained._tie_or_clone_weights
        if not self.lang_dec:
            self.obj_decoder = R.BertDecoderModel(self.config)
            if self.tie_embed:
                tie(self.output_layer, self.decoder.embeddings.word_embeddings)
        else:
            dec = R.BertDecoderModel(self.config)
            self.obj_decoder = nn.ModuleList([copy.deepcopy(dec) for _ in text_processor.languages])
            for i, dec in enumerate(self.obj_decoder):
                if self.tie_embed:
                    dec.embeddings.position_embeddings = self.encoder.embeddings.position_embeddings
                tie(self.output_layer[i], dec.embeddings.word_embeddings)
                tie(self.encoder.embeddings.token_type_embeddings, dec.embeddings.token_type_embeddings)
        self.multistream_attention_gate = nn.Parameter(torch.full((1, d), 0.1))

    def encode(self, src_inputs=None, src_mask=None, src_langs=None, images=None, objects=None):
        if images is None:
            return super().encode(src_inputs, src_mask, src_langs)
        emb, _ = self.image_model(images)
        has = objects is not None and objects["labels"].numel() > 0 and bool((objects["labels"] != 0).any())
        return emb, (object_fc(self.image_model, objects) if has else None)

    def mix(self, dec_out, obj_out):
        s = torch.sigmoid(self.multistream_attention_gate + 1e-7)
        return s * dec_out + (1 - s) * obj_out

    def forward(self, tgt_inputs=None, tgt_langs=None, tgt_mask=None, batch=None, log_softmax=False, **kw):
        emb, obj = self.encode(images=batch["images"], objects=batch.get("objects"))
        lang = int(tgt_langs[0])
        types = tgt_langs.unsqueeze(-1).expand(-1, tgt_inputs.size(-1))[:, :-1]
        sub = R.future_mask(tgt_mask[:, :-1])
        args = dict(input_ids=tgt_inputs[:, :-1], encoder_attention_mask=None, tgt_attention_mask=sub, token_type_ids=types)
        dec = self.decoder if not self.lang_dec else self.decoder[lang]
        out = dec(encoder_states=emb, **args)
        if obj is not None:
            od = self.obj_decoder if not self.lang_dec else self.obj_decoder[lang]
            out = self.mix(out, od(encoder_states=obj, **args))
        sel = out.reshape(-1, out.size(-1))[tgt_mask[:, 1:].reshape(-1)]
        output_layer = self.output_layer if (not self.lang_dec) and self.tie_embed else self.output_layer[lang]
        logits = output_layer(sel)
        return F.log_softmax(logits, dim=-1) if log_softmax else logits


class _Blended(nn.Module):
    """The image decoder and the object decoder behind one decoder call: what oracle.seq_gen.BeamDecoder sees."""

    def __init__(self, model, dec, obj_dec, obj_states):
        super().__init__()
        self.model, self.dec, self.obj_dec, self.obj_states = model, dec, obj_dec, obj_states

    def forward(self, encoder_states=None, **kw):
        out = self.dec(encoder_states=encoder_states, **kw)
        rep = encoder_states.size(0) // self.obj_states.size(0)
        objs = self.obj_states if rep == 1 else torch.repeat_interleave(self.obj_states, rep, 0)
        kw["encoder_attention_mask"] = None
        return self.model.mix(out, self.obj_dec(encoder_states=objs, **kw))


class _Proxy:
    def __init__(self, model, decoder):
        self._model, self.decoder = model, decoder

    def __getattr__(self, name):
        return getattr(self._model, name)


@torch.no_grad()
def beam_search(model, images, objects, beam_width, **kw):
    emb, obj = model.encode(images=images, objects=objects)
    if obj is not None:
        if model.lang_dec:
            dec = [_Blended(model, d, od, obj) for d, od in zip(model.decoder, model.obj_decoder)]
        else:
            dec = _Blended(model, model.decoder, model.obj_decoder, obj)
        model = _Proxy(model, dec)
    return OG.BeamDecoder(model, beam_width=beam_width)(image_embed=emb, **kw)
