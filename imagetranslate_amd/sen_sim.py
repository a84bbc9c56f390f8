"""SenSim -- counterpart of src/sen_sim.py: the encoder stack, a one-vector attention pooling of its states to unit vectors
(``encode`` ``:36-47`` and the ``/ (norm + 1e-4)`` of ``:68-71``), and on the unit vectors of a batch of sentence pairs either
their dot products (``normalize=False``, ``:112``), the one-sided contrastive loss (``:105-108``) or, with a batch of negatives for
each side, the two-sided one (``:94-103``).  The tail is one autograd node per mode: ``imt_attn_pool_fwd`` pools every encoded
batch straight into its rows of the concatenated buffers, one kernel call gives the loss (or the dot products) together with the
gradients with respect to the unit vectors, and the backward is one ``imt_attn_pool_bwd`` per encoded batch."""
import json
import os
import pickle
import weakref

import torch
import torch.nn as nn

from . import hip_ops as O
from . import lm_config
from .bert_seq2seq import BertConfig, BertEncoderModel, dropout_seed_offset
from .param_store import store_of
from .seq2seq import FlatStoreModel


class _PooledTailFn(torch.autograd.Function):
    """The tail of SenSim over 2 (sources, targets) or 4 (source negatives, sources, target negatives, targets) encoded batches.
    Forward: ``imt_attn_pool_fwd`` writes the unit vectors of each batch into its slice of scat = [source negatives; sources] and
    tcat = [target negatives; targets] (the reference's cat([neg, pos]), :94-95), then ONE call:
      mode "dot":       ``imt_pair_dot``    -> [B] dot products;
      mode "one_sided": ``imt_contrastive`` with N = B -> the loss and its gradients;
      mode "two_sided": ``imt_sensim_loss`` -> the loss and its gradients.
    Backward: one ``imt_attn_pool_bwd`` per batch; the upstream loss gradient enters as a device scalar (``du_scale``), the
    gradient of the dot products through ``imt_pair_dot_bwd``; d(input_attention) accumulates into the flat gradient."""

    @staticmethod
    def forward(ctx, anchor, model, mode, n_neg_batches, *states_and_masks):
        store = store_of(model).ensure()
        states, masks = states_and_masks[0::2], states_and_masks[1::2]
        dtype, d = states[0].dtype, states[0].shape[-1]
        w, b = store.views(dtype, model.input_attention.weight, model.input_attention.bias)
        w = w.view(-1)  # nn.Linear(d, 1) weight is [1, d]
        states = [s.to(dtype).contiguous() for s in states]
        if n_neg_batches:
            sneg, src, tneg, tgt = states
            sides = ((sneg, src), (tneg, tgt))
        else:
            src, tgt = states
            sides = ((src,), (tgt,))
        B = src.shape[0]
        if tgt.shape[0] != B:
            raise ValueError("SenSim: %d sources for %d targets" % (B, tgt.shape[0]))
        bufs, saved, slices = [], [], []
        k = 0
        for side in sides:
            buf = torch.empty((sum(s.shape[0] for s in side), d), device=src.device, dtype=torch.float32)
            row = 0
            for s in side:
                _, probs, norm = O.attn_pool_fwd(s, w, b, masks[k], out=buf[row:row + s.shape[0]])
                saved += [probs, norm]
                slices.append((len(bufs), row, row + s.shape[0]))
                row += s.shape[0]
                k += 1
            bufs.append(buf)
        scat, tcat = bufs
        if mode == "dot":
            out, grads = O.pair_dot(scat, tcat), ()
        elif mode == "one_sided":
            loss, d_s, d_t = O.contrastive(scat, tcat)
            out, grads = loss.view(()), (d_s, d_t)
        else:
            loss, d_s, d_t = O.sensim_loss(scat, tcat, B)
            out, grads = loss.view(()), (d_s, d_t)
        ctx.store, ctx.model, ctx.layout_version = store, model, store.layout_version
        ctx.mode, ctx.masks, ctx.slices, ctx.n_states = mode, masks, slices, len(states)
        ctx.save_for_backward(w, scat, tcat, *grads, *states, *saved)
        return out

    @staticmethod
    def backward(ctx, g):
        t = ctx.saved_tensors
        w, scat, tcat = t[:3]
        n, k0 = ctx.n_states, 3 + (0 if ctx.mode == "dot" else 2)
        states, saved = t[k0:k0 + n], t[k0 + n:]
        store, att = ctx.store, ctx.model.input_attention
        store.check_layout(ctx.layout_version, "SenSim tail")
        bufs = (scat, tcat)
        if ctx.mode == "dot":
            dus, scale = O.pair_dot_bwd(scat, tcat, g.detach().to(torch.float32).contiguous()), None
        else:
            dus, scale = t[3:5], g.detach().to(torch.float32).reshape(1).contiguous()
        gw, gb = store.grad_view(att.weight).view(-1), store.grad_view(att.bias)
        out = []
        for k in range(n):
            side, lo, hi = ctx.slices[k]
            dx = O.attn_pool_bwd(states[k], w, ctx.masks[k], bufs[side][lo:hi], saved[2 * k], saved[2 * k + 1], dus[side][lo:hi], gw, gb,
                                 du_scale=scale)
            out += [dx, None]
        store.attach_grad_views()
        return (None, None, None, None) + tuple(out)


class SenSim(FlatStoreModel):
    def __init__(self, text_processor, enc_layer: int = 6, embed_dim: int = 768, intermediate_dim: int = 3072, *,
                 num_attention_heads: int = 12):
        super(SenSim, self).__init__()
        self.text_processor = text_processor
        self.config = lm_config.get_config(vocab_size=text_processor.tokenizer.get_vocab_size(),
                                           pad_token_id=text_processor.pad_token_id(),
                                           bos_token_id=text_processor.bos_token_id(),
                                           eos_token_id=text_processor.sep_token_id(),
                                           enc_layer=enc_layer, embed_dim=embed_dim, intermediate_dim=intermediate_dim,
                                           num_attention_heads=num_attention_heads)
        self.enc_layer = enc_layer
        self.embed_dim = embed_dim
        self.intermediate_dim = intermediate_dim
        self.config["type_vocab_size"] = len(text_processor.languages)
        self.config = BertConfig(**self.config)
        self.encoder = BertEncoderModel(self.config)
        self.encoder.init_weights()
        self.input_attention = nn.Linear(self.config.hidden_size, 1)
        self._imt_compute_dtype = torch.float32
        self._link_stacks()

    def _link_stacks(self):
        self.encoder.__dict__["_imt_owner"] = weakref.ref(self)

    def flat_param_order(self):
        """The order in which the gradients become final: the pooling vector, then the encoder from the top."""
        ps = [self.input_attention.weight, self.input_attention.bias]
        for lyr in reversed(list(self.encoder.encoder.layer)):
            ps += lyr.ordered_params()
        e = self.encoder.embeddings
        return ps + [e.LayerNorm.weight, e.LayerNorm.bias, e.position_embeddings.weight, e.token_type_embeddings.weight,
                     e.word_embeddings.weight]

    @property
    def _device(self):
        return self.encoder.embeddings.word_embeddings.weight.device

    def init_from_lm(self, model):
        """Adopt the encoder weights of a loaded ``LM`` or ``Seq2Seq`` (src/sen_sim.py:33-34, what ``train_txt_sim --pretrained``
        does): only ``model.encoder`` is read.  The values are copied into this model's flat store; the module is not rebound.  An encoder of another shape (layers, widths,
        vocabulary, positions, ``type_vocab_size``) or another head count is refused."""
        theirs, mine = model.encoder.state_dict(), self.encoder.state_dict()
        a = {k: tuple(v.shape) for k, v in theirs.items()}
        b = {k: tuple(v.shape) for k, v in mine.items()}
        if a != b:
            diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
            raise ValueError("SenSim.init_from_lm: the encoder does not match (%s: %s there, %s here)"
                             % (diff[0], a.get(diff[0]), b.get(diff[0])))
        heads = int(model.encoder.config.num_attention_heads)
        if heads != int(self.config.num_attention_heads):
            raise ValueError("SenSim.init_from_lm: the encoder has %d attention heads, this model %d"
                             % (heads, int(self.config.num_attention_heads)))
        res = self.load_state_dict({"encoder." + k: v for k, v in theirs.items()}, strict=False)
        assert not res.unexpected_keys and set(res.missing_keys) == {"input_attention.weight", "input_attention.bias"}, res
        return self

    def _states(self, inputs, mask, langs, pass_index: int = 0):
        """Encoder states of one batch; ``langs`` [rows] is expanded over the positions (:54).  In training mode every pass draws a
        dropout seed of its own; under a pinned seed (tests) pass k uses seed + k."""
        device = self._device
        inputs, mask = inputs.to(device), mask.to(device)
        langs = langs.to(device).unsqueeze(-1).expand(-1, inputs.size(-1))
        with dropout_seed_offset(self.encoder, pass_index):
            return self.encoder(inputs, attention_mask=mask, token_type_ids=langs), mask

    @torch.no_grad()
    def encode(self, src_inputs, src_mask, src_langs):
        """[rows, d] fp32: the reference's UNNORMALISED sentence vectors (src/sen_sim.py:36-47), recovered from the pooling
        kernel's outputs as u * (norm + 1e-4).  ``src_langs`` is per position, [rows, S], as in the reference.  An inference
        helper: it runs without autograd and returns a detached tensor (the reference's ``encode`` is differentiable; training
        goes through ``forward``)."""
        device = self._device
        src_inputs, src_mask, src_langs = src_inputs.to(device), src_mask.to(device), src_langs.to(device)
        states = self.encoder(src_inputs, attention_mask=src_mask, token_type_ids=src_langs)
        store = store_of(self).ensure()
        w, b = store.views(states.dtype, self.input_attention.weight, self.input_attention.bias)
        u, _, norm = O.attn_pool_fwd(states.contiguous(), w.view(-1), b, src_mask)
        return (u * (norm.unsqueeze(-1) + 1e-4)).detach()

    @torch.no_grad()
    def encode_unit(self, inputs, mask, langs):
        """[rows, d] fp32: the UNIT sentence vectors u = v / (|v| + 1e-4) as ``imt_attn_pool_fwd`` writes them -- what the
        similarity of ``forward`` and the neighbour search of ``mine_pairs`` work on.  ``langs`` is per sentence [rows] (as
        ``forward`` takes it) or per position [rows, S] (as ``encode`` does).  No autograd."""
        device = self._device
        inputs, mask, langs = inputs.to(device), mask.to(device), langs.to(device)
        if langs.dim() == 1:
            langs = langs.unsqueeze(-1).expand(-1, inputs.size(-1))
        states = self.encoder(inputs, attention_mask=mask, token_type_ids=langs)
        store = store_of(self).ensure()
        w, b = store.views(states.dtype, self.input_attention.weight, self.input_attention.bias)
        u, _, _ = O.attn_pool_fwd(states.contiguous(), w.view(-1), b, mask)
        return u.detach()

    def forward(self, src_inputs, src_mask, src_langs, tgt_inputs, tgt_mask, tgt_langs, src_neg_inputs=None, src_neg_mask=None,
                src_neg_langs=None, tgt_neg_inputs=None, tgt_neg_mask=None, tgt_neg_langs=None, normalize: bool = False):
        """``normalize=False``: [B] dot products of the pairs' unit vectors.  ``normalize=True``: the contrastive loss (0-d fp32),
        two-sided when ``src_neg_langs`` is given (the reference's test, :73), else one-sided."""
        with_neg = bool(normalize) and src_neg_langs is not None
        batches = []
        if with_neg:
            if tgt_neg_langs is None or src_neg_inputs is None or tgt_neg_inputs is None or src_neg_mask is None or tgt_neg_mask is None:
                raise ValueError("SenSim: negatives need inputs, masks and languages for both sides")
            batches = [(src_neg_inputs, src_neg_mask, src_neg_langs), (src_inputs, src_mask, src_langs),
                       (tgt_neg_inputs, tgt_neg_mask, tgt_neg_langs), (tgt_inputs, tgt_mask, tgt_langs)]
        else:
            batches = [(src_inputs, src_mask, src_langs), (tgt_inputs, tgt_mask, tgt_langs)]
        flat = []
        for k, (inputs, mask, langs) in enumerate(batches):
            flat += list(self._states(inputs, mask, langs, k))
        mode = "two_sided" if with_neg else ("one_sided" if normalize else "dot")
        anchor = store_of(self).ensure().anchor_if_grad()
        return _PooledTailFn.apply(anchor, self, mode, 2 if with_neg else 0, *flat)

    def loss_fused(self, src_inputs, src_mask, src_langs, tgt_inputs, tgt_mask, tgt_langs, **neg):
        """(loss, number of sentence pairs); ``neg``: the six negative-sample arguments of ``forward``, or none of them."""
        return self(src_inputs, src_mask, src_langs, tgt_inputs, tgt_mask, tgt_langs, normalize=True, **neg), int(src_inputs.size(0))

    def save(self, out_dir: str):
        if not os.path.exists(out_dir):
            os.makedirs(out_dir)
        with open(os.path.join(out_dir, "mt_config"), "wb") as fp:
            pickle.dump((self.enc_layer, self.embed_dim, self.intermediate_dim), fp)
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, os.path.join(out_dir, "mt_model.state_dict"))
        # build extension (the reference hard-codes 12 heads): beside the reference's files, as Caption2Image.save does
        with open(os.path.join(out_dir, "imt_config.json"), "w") as fp:
            json.dump({"num_attention_heads": int(self.config.num_attention_heads)}, fp)

    @staticmethod
    def load(out_dir: str, tok_dir: str, text_processor=None):
        """(model, text_processor), as the reference returns them (src/sen_sim.py:127-139)."""
        if text_processor is None:
            from .textprocessor import TextProcessor
            text_processor = TextProcessor(tok_model_path=tok_dir)
        from .safe_pickle import load_caption2image_config
        enc_layer, embed_dim, intermediate_dim = load_caption2image_config(os.path.join(out_dir, "mt_config"))
        kw = {}
        extra = os.path.join(out_dir, "imt_config.json")
        if os.path.exists(extra):  # absent in a directory the reference wrote: its 12 heads
            with open(extra, "r") as fp:
                kw["num_attention_heads"] = int(json.load(fp).get("num_attention_heads", 12))
        model = SenSim(text_processor=text_processor, enc_layer=enc_layer, embed_dim=embed_dim, intermediate_dim=intermediate_dim, **kw)
        sd = torch.load(os.path.join(out_dir, "mt_model.state_dict"), map_location="cpu", weights_only=True)
        model.load_state_dict(sd, strict=False)
        return model.to(torch.device("cuda" if torch.cuda.is_available() else "cpu")), text_processor
