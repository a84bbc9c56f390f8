"""Image branch of the path -- drop-in for the on-path parts of the reference's ``src/image_model.py``:
``ImageMassSeq2Seq`` (text branch ``:157-183``, gated text + image branch ``:185-230``, contrastive branch ``:231-264``),
``ImageCaptioning`` (``:267-377``) and ``Caption2Image`` (``:380-464``).

The frozen ResNet trunk (``:24-36``) is ``resnet.ResNetTrunk`` on the MFMA convolution kernels (csrc/conv.hip): attached to
the head with ``ImageHead.attach_trunk`` it turns 4-D pixel inputs into region features, and
``python -m imagetranslate_amd.extract_features`` writes them to the ``features.pt`` the trainers read.  It is never trained
(DESIGN.md section 1), so region features ``[B, 49, C]`` may as well enter pre-extracted at the ``fc`` layer:
``ImageHead`` = dropout -> fc (no bias) -> + location_embedding -> dropout (``:35-41,77-78``).  The Faster-RCNN detector
(``:42-124``) stays out of scope.
The detector's output (box features, boxes, labels) enters pre-extracted as ``batch["objects"]``: ``ImageCaptioning``
then runs its object stream (object rows ``:58-78``, ``obj_decoder`` and ``multistream_attention_gate`` ``:357-366``).
``ImageMassSeq2Seq`` with ``batch=`` runs its decoder over the text states and over the image regions and mixes the two with
``multimodal_attention_gate``, or, with negative samples, the contrastive loss on the fused pooling kernels (csrc/pool.hip).
``Caption2Image`` maps a sentence to the 49 x d region embedding of its image: encoder stack, sentence pooling
(``imt_sent_pool_fwd``, dropout included), one linear layer; its loss is the L2 distance to a captioner's embedding (``imt_l2_dist``).
"""
import json
import os
import pickle
import weakref

import torch
import torch.nn as nn

from . import hip_ops as O
from . import lm_config
from .bert_seq2seq import BertConfig, BertDecoderModel, BertEncoderModel, _LinearFn, _Pretrained, dropout_seed
from .mass_seq2seq import MassSeq2Seq
from .param_store import store_of
from .seq2seq import DecoderStream, FlatStoreModel, _GatedMixFn, future_mask, gated_mix, unwrap  # noqa: F401


class _ImageHeadFn(torch.autograd.Function):
    """dropout -> fc (no bias) -> + location_embedding -> dropout (src/image_model.py:35-41,77-78) on the HIP kernels:
    ``imt_add_rows_dropout`` (input dropout, fp32 features -> compute dtype), ``imt_gemm`` (fc), ``imt_add_rows_dropout``
    (+ location rows, output dropout).  Backward: the output dropout's mask is regenerated from its seed, the location
    gradient is a column sum over the batch (``imt_colsum``), the fc gradient one TN GEMM into the flat gradient buffer.
    The region features are frozen inputs: no gradient flows to them."""

    @staticmethod
    def forward(ctx, anchor, x, head, dtype, p, seed):
        store = store_of(head).ensure()
        w, loc = store.views(dtype, head.fc.weight, head.location_embedding.weight)
        (d, C), R, B = w.shape, loc.shape[0], x.shape[0]
        if x.shape[1] != R:
            raise ValueError("image head: %d regions given, location_embedding has %d" % (x.shape[1], R))
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        xd = O.add_rows_dropout(x.reshape(B * R, C).contiguous(), None, out_dtype=dtype, dropout_p=p, dropout_seed=seed)
        y = O.gemm(xd, w, O.IMT_NT, splitk_ws=O.splitk_workspace(xd.device))
        out = O.add_rows_dropout(y, loc, dropout_p=p, dropout_seed=seed + 1)
        ctx.store, ctx.head, ctx.layout_version = store, head, store.layout_version
        ctx.dims, ctx.p, ctx.seed = (B, R, d, C), p, seed
        ctx.save_for_backward(xd)
        return out.view(B, R, d)

    @staticmethod
    def backward(ctx, dout):
        (xd,) = ctx.saved_tensors
        store, head = ctx.store, ctx.head
        store.check_layout(ctx.layout_version, "image head")
        B, R, d, C = ctx.dims
        dy = O.add_rows_dropout(dout.to(xd.dtype).reshape(B * R, d).contiguous(), None, dropout_p=ctx.p, dropout_seed=ctx.seed + 1)
        # d(location_embedding) += sum over images; d(fc.weight) += dy^T x
        O.colsum(dy.view(B, R * d), store.grad_view(head.location_embedding.weight).view(-1))
        sk = O.dw_split_k(B * R, d, C, 256)
        O.gemm(dy, xd, O.IMT_TN, out=store.grad_view(head.fc.weight), accumulate=(sk == 1), split_k=sk)
        store.attach_grad_views()
        return None, None, None, None, None, None


def _objects_present(objects):
    """batch["objects"] = {"feats": [B,N,1024], "boxes": [B,N,4], "labels": [B,N] int64 (0 = padding)}; None, a missing key
    or N == 0 means the batch has no object stream (the reference's max_feature_nums == 0, src/image_model.py:53), and so
    does a batch whose labels are all 0 (padding only: no detection).  That last test is made for labels on the host only
    (the loader already leaves "objects" out of a batch without detections): device labels would cost a synchronisation."""
    if objects is None or objects.get("labels") is None:
        return False
    labels = objects["labels"]
    if labels.dim() != 2 or labels.size(1) == 0:
        return False
    return labels.is_cuda or bool((labels != 0).any())


class _ObjectHeadFn(torch.autograd.Function):
    """Object rows of src/image_model.py:58-78 on the HIP kernels: ``imt_obj_rows`` stages [object_embedding[label] |
    feature | locs] rows (label-0 rows zeroed whole) and the weight, both padded to Kp columns; ``imt_gemm`` NT is
    object_feat_fc (no bias); ``imt_relu_dropout`` the ReLU and the dropout (training only).  Backward: the mask is
    regenerated from the seed, dW is one TN GEMM into an fp32 [d, Kp] scratch folded into the flat gradient
    (``imt_obj_fold_w``), the embedding rows' gradient dz W_pad[:, :d] is scattered by label in a fixed order
    (``imt_obj_embed_grad``).  No gradient flows to the detector output (it runs under no_grad, :50-53)."""

    @staticmethod
    def forward(ctx, anchor, feats, boxes, labels, head, dtype, p, seed, status):
        store = store_of(head).ensure()
        w, emb = store.views(dtype, head.object_feat_fc.weight, head.object_embedding.weight)
        d, K = w.shape
        B, N = labels.shape
        x, w_pad = O.obj_rows(labels.reshape(-1).contiguous(), feats.reshape(B * N, -1).contiguous(),
                              boxes.reshape(B * N, 4).contiguous(), emb.view(-1), w.view(-1), d, dtype, status=status)
        y = O.relu_dropout_(O.gemm(x, w_pad, O.IMT_NT, splitk_ws=O.splitk_workspace(x.device)), p, seed)
        ctx.store, ctx.head, ctx.layout_version = store, head, store.layout_version
        ctx.dims, ctx.p, ctx.seed = (B, N, d, K), p, seed
        ctx.save_for_backward(x, w_pad, y, labels)
        return y.view(B, N, d)

    @staticmethod
    def backward(ctx, dout):
        x, w_pad, y, labels = ctx.saved_tensors
        store, head = ctx.store, ctx.head
        store.check_layout(ctx.layout_version, "object head")
        B, N, d, K = ctx.dims
        dz = O.relu_dropout_bwd(dout.to(y.dtype).reshape(B * N, d).contiguous(), y, ctx.p, ctx.seed)
        dw = torch.empty(w_pad.shape, device=x.device, dtype=torch.float32)
        O.gemm(dz, x, O.IMT_TN, out=dw)                                                   # dz^T X  [d, Kp]
        O.obj_fold_w(dw, store.grad_view(head.object_feat_fc.weight).view(-1), d)         # d(object_feat_fc.weight) +=
        dxe = O.gemm(dz, w_pad[:, :d], O.IMT_NN, splitk_ws=O.splitk_workspace(x.device))  # d(embedding rows) [R, d]
        O.obj_embed_grad(labels.reshape(-1).contiguous(), dxe, store.grad_view(head.object_embedding.weight).view(-1))
        store.attach_grad_views()
        return None, None, None, None, None, None, None, None, None


class _ContrastiveTailFn(torch.autograd.Function):
    """Contrastive tail (src/image_model.py:240-263) as one node: ``imt_attn_pool_fwd`` on the caption states (masked by
    src_pads), the negative-sample states (masked by neg_mask), both with encoder_attention_w, and on the image regions with
    image_attention_w (unmasked), the two text sets written into one [B + Nn, d] buffer (the reference's cat, :250); then
    ``imt_contrastive`` gives the loss and, in the same pass, its gradients with respect to the unit vectors.  Backward: three
    ``imt_attn_pool_bwd`` calls (the upstream loss gradient enters as a device scalar) return the gradients the encoder stack
    and the image head receive; d(encoder_attention_w), d(image_attention_w) accumulate into the flat gradient."""

    @staticmethod
    def forward(ctx, anchor, enc_states, src_mask, neg_states, neg_mask, img_states, model):
        store = store_of(model).ensure()
        dtype = enc_states.dtype
        d = enc_states.shape[-1]
        B, Nn = enc_states.shape[0], neg_states.shape[0]
        if img_states.shape[0] != B:
            raise ValueError("contrastive loss: %d images for %d captions" % (img_states.shape[0], B))
        we, be, wi, bi = store.views(dtype, model.encoder_attention_w.weight, model.encoder_attention_w.bias,
                                     model.image_attention_w.weight, model.image_attention_w.bias)
        we, wi = we.view(-1), wi.view(-1)  # nn.Linear(d, 1) weights are [1, d]
        enc, neg, img = enc_states.contiguous(), neg_states.to(dtype).contiguous(), img_states.to(dtype).contiguous()
        txt = torch.empty((B + Nn, d), device=enc.device, dtype=torch.float32)
        _, p_e, n_e = O.attn_pool_fwd(enc, we, be, src_mask, out=txt[:B])
        _, p_n, n_n = O.attn_pool_fwd(neg, we, be, neg_mask, out=txt[B:])
        img_u, p_i, n_i = O.attn_pool_fwd(img, wi, bi, None)
        loss, d_img, d_txt = O.contrastive(img_u, txt)
        ctx.store, ctx.model, ctx.layout_version, ctx.dims = store, model, store.layout_version, (B, Nn, d)
        ctx.masks = (src_mask, neg_mask)
        ctx.save_for_backward(enc, neg, img, we, wi, txt, img_u, p_e, n_e, p_n, n_n, p_i, n_i, d_img, d_txt)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        enc, neg, img, we, wi, txt, img_u, p_e, n_e, p_n, n_n, p_i, n_i, d_img, d_txt = ctx.saved_tensors
        B, Nn, d = ctx.dims
        store, model = ctx.store, ctx.model
        store.check_layout(ctx.layout_version, "contrastive tail")
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        gw_e, gb_e = store.grad_view(model.encoder_attention_w.weight).view(-1), store.grad_view(model.encoder_attention_w.bias)
        gw_i, gb_i = store.grad_view(model.image_attention_w.weight).view(-1), store.grad_view(model.image_attention_w.bias)
        d_enc = O.attn_pool_bwd(enc, we, ctx.masks[0], txt[:B], p_e, n_e, d_txt[:B], gw_e, gb_e, du_scale=g)
        d_neg = O.attn_pool_bwd(neg, we, ctx.masks[1], txt[B:], p_n, n_n, d_txt[B:], gw_e, gb_e, du_scale=g)
        d_im = O.attn_pool_bwd(img, wi, None, img_u, p_i, n_i, d_img, gw_i, gb_i, du_scale=g)
        store.attach_grad_views()
        return None, d_enc, None, d_neg, None, d_im, None


class ImageHead(nn.Module):
    """Stands in for ModifiedResnet's head; ``feat_dim`` = channels of the frozen trunk (2048 for depth >= 3)."""

    def __init__(self, feat_dim: int, embed_dim: int, dropout: float = 0.1, regions: int = 49):
        super().__init__()
        self.dropout = dropout
        self.fc = nn.Linear(in_features=feat_dim, out_features=embed_dim, bias=False)
        self.location_embedding = nn.Embedding(regions, embed_dim)
        self.layer_norm = nn.LayerNorm(embed_dim, eps=1e-12)  # present (unused) in the reference, :103
        self.fcnn = None

    def attach_trunk(self, trunk):
        """Keep a frozen ``resnet.ResNetTrunk`` for pixel inputs.  It is not a registered submodule: it has no gradients, so it
        stays out of the flat parameter store, of ``parameters()`` and of ``state_dict()`` (``save`` writes its tensors itself)."""
        if trunk is not None and trunk.out_channels != self.fc.in_features:
            raise ValueError("image head: the trunk gives %d channels, fc was built for %d" % (trunk.out_channels, self.fc.in_features))
        self.__dict__["_imt_trunk"] = trunk
        return self

    @property
    def trunk(self):
        return self.__dict__.get("_imt_trunk")

    def region_features(self, pixels, compute_dtype=torch.float32):
        """Pixels (4-D: ``[B, H, W, 8]`` from ``hip_ops.image_to_nhwc``, uint8 ``[B, H, W, 3]`` or normalised NCHW) through the
        attached trunk: ``[B, regions, feat_dim]`` (src/image_model.py:24-36)."""
        trunk = self.trunk
        if trunk is None:
            raise ValueError("image head: a 4-D input is pixels and needs the CNN trunk -- attach one with "
                             "image_model.attach_trunk(ResNetTrunk(depth).load_state_dict(weights)), or pass region features "
                             "[B, regions, %d] (python -m imagetranslate_amd.extract_features writes them)" % self.fc.in_features)
        dev = self.fc.weight.device
        if trunk.device != dev:
            trunk.to(dev)
        return trunk.set_compute_dtype(compute_dtype)(pixels)

    def forward(self, grid_hidden, compute_dtype=torch.float32):
        """grid_hidden: region features [B, regions, feat_dim] (the reference's x8.view().permute(), :35-36), or 4-D pixels,
        which run the attached trunk first."""
        if grid_hidden.dim() == 4:
            grid_hidden = self.region_features(grid_hidden, compute_dtype)
        x = grid_hidden.to(self.fc.weight.device)
        p = float(self.dropout) if self.training else 0.0
        seed = dropout_seed(self, p > 0)
        return _ImageHeadFn.apply(store_of(self).ensure().anchor_if_grad(), x, self, compute_dtype, p, seed), None

    def add_object_head(self, embed_dim: int):
        """object_feat_fc (Linear(d + 1031 -> d), no bias) and object_embedding (91 labels), src/image_model.py:110-116.
        Built under a forked RNG: every other parameter of the model initialises exactly as without them."""
        with torch.random.fork_rng(devices=[]):
            self.object_feat_fc = nn.Linear(in_features=O.OBJ_FEAT_DIM + 7 + embed_dim, out_features=embed_dim, bias=False)
            self.object_embedding = nn.Embedding(O.OBJ_LABELS, embed_dim)

    def objects_forward(self, objects, compute_dtype=torch.float32):
        """object_fc [B, N, d] (src/image_model.py:53-82) from pre-extracted detector output, or None when the batch has no
        detections.  Labels must lie in [0, 91).  Host labels are checked here; for device labels imt_obj_rows zeroes an
        out-of-range row and raises a status word that is read back without waiting (``check_object_labels``): the error
        surfaces at the next call once that step has run, or at once with ``wait=True``."""
        if not _objects_present(objects) or getattr(self, "object_feat_fc", None) is None:
            return None
        dev = self.object_feat_fc.weight.device
        labels = objects["labels"]
        status = None
        if not labels.is_cuda:
            if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= O.OBJ_LABELS):
                raise ValueError("objects: labels must lie in [0, %d)" % O.OBJ_LABELS)
        else:
            self.check_object_labels()
            status = self.__dict__.get("_imt_label_status_dev")
            if status is None or status.device != labels.device:
                status = torch.zeros(1, dtype=torch.int32, device=labels.device)
                self.__dict__["_imt_label_status_dev"] = status
        labels = labels.to(device=dev, dtype=torch.int64)
        feats = objects["feats"].to(dev)
        if feats.dtype not in (torch.float32, torch.bfloat16):
            feats = feats.float()
        boxes = objects["boxes"].to(device=dev, dtype=torch.float32)
        p = float(self.dropout) if self.training else 0.0
        seed = dropout_seed(self, p > 0, salt=2)
        anchor = store_of(self).ensure().anchor_if_grad()
        out = _ObjectHeadFn.apply(anchor, feats, boxes, labels, self, compute_dtype, p, seed, status)
        if status is not None:  # cumulative device word -> pinned host copy, read once its event has completed
            host = self.__dict__.get("_imt_label_status_host")
            if host is None:
                host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
                self.__dict__["_imt_label_status_host"] = host
            host.copy_(status, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.__dict__["_imt_label_status_event"] = ev
        return out

    def check_object_labels(self, wait: bool = False):
        """Raise if a device-resident label outside [0, 91) has reached the object head (its row was zeroed).  Without
        ``wait`` only a read-back that has already completed is looked at (no synchronisation)."""
        ev = self.__dict__.get("_imt_label_status_event")
        if ev is None or (not wait and not ev.query()):
            return
        ev.synchronize()
        self.__dict__["_imt_label_status_event"] = None
        if int(self.__dict__["_imt_label_status_host"][0]) != 0:
            self.__dict__["_imt_label_status_dev"].zero_()
            raise ValueError("objects: a label outside [0, %d) reached the object head (its row was zeroed)" % O.OBJ_LABELS)


class ImageMassSeq2Seq(MassSeq2Seq):
    def __init__(self, text_processor, freeze_image: bool = False, resnet_depth: int = 1, lang_dec: bool = False,
                 use_proposals: bool = False, tie_embed: bool = False, enc_layer: int = 6, dec_layer: int = 3,
                 embed_dim: int = 768, intermediate_dim: int = 3072, use_obj: bool = True, *,
                 num_attention_heads: int = 12, image_feat_dim: int = None):
        super(ImageMassSeq2Seq, self).__init__(text_processor=text_processor, tie_embed=tie_embed, lang_dec=lang_dec,
                                               use_proposals=use_proposals, enc_layer=enc_layer, dec_layer=dec_layer,
                                               embed_dim=embed_dim, intermediate_dim=intermediate_dim,
                                               freeze_image=freeze_image, resnet_depth=resnet_depth,
                                               num_attention_heads=num_attention_heads)
        if image_feat_dim is None:
            image_feat_dim = 512 if resnet_depth <= 2 else 2048  # fc.in_features of resnet18/34 vs 50+ (:87-97)
        # the reference builds a pretrained torchvision trunk here unconditionally (:136-138, network fetch); here the head is
        # built alone and a trunk (resnet.ResNetTrunk) is attached by `load` or by the caller when pixels are to be read.
        self.image_model = ImageHead(image_feat_dim, self.config.hidden_size, self.config.hidden_dropout_prob)
        self.multimodal_attention_gate = nn.Parameter(torch.zeros(1, self.config.hidden_size).fill_(0.1),
                                                      requires_grad=True)
        self.image_attention_w = nn.Linear(self.config.hidden_size, 1)
        self.encoder_attention_w = nn.Linear(self.config.hidden_size, 1)

    def encode(self, src_inputs, src_mask, src_langs, images=None):
        encoder_states = super().encode(src_inputs, src_mask, src_langs)
        if images is not None:
            image_embeddings = self.image_model(unwrap(images), self._imt_compute_dtype)
            return encoder_states[0], image_embeddings
        return encoder_states

    def _encode_text_and_image(self, src_inputs, src_pads, src_langs, batch):
        """(encoder states, image embeddings, src_pads on the device) of src/image_model.py:185-190.  The reference's head
        returns (grid, objects) and its ``encode`` keeps that tuple (:153 against :82), so the branch cannot run there; the
        build takes element 0, the grid embeddings, which is plainly what :213 and :252 mean."""
        if src_inputs is None:
            raise ValueError("ImageMassSeq2Seq with batch=: src_inputs is required (src/image_model.py:185)")
        device = self._device
        src_inputs = src_inputs.to(device)
        src_pads = (src_inputs != self.text_processor.pad_token_id()) if src_pads is None else src_pads.to(device)
        src_langs_t = self._lang_grid(src_langs, src_inputs.size(-1), device)
        encoder_states = MassSeq2Seq.encode(self, src_inputs, src_pads, src_langs_t)[0]
        image_embeddings = self.image_model(unwrap(batch["images"]), self._imt_compute_dtype)[0]
        return encoder_states, image_embeddings, src_pads

    def _multimodal_rows(self, src_inputs, src_pads, tgt_inputs, src_langs, tgt_langs, pad_idx, tgt_positions, batch, proposals):
        """Non-pad decoder rows of the gated text + image branch (src/image_model.py:192-226)."""
        assert tgt_inputs is not None
        encoder_states, image_embeddings, src_pads = self._encode_text_and_image(src_inputs, src_pads, src_langs, batch)
        langs = tgt_langs if tgt_langs is not None else src_langs
        batch_lang = int(langs[0])
        decoder = self._decoder_for(batch_lang)
        # the SAME decoder over the text states (key mask src_pads) and over the image regions, no key mask (:213-216)
        streams = [DecoderStream(decoder, encoder_states, src_pads, None),
                   DecoderStream(decoder, image_embeddings, None, self.multimodal_attention_gate)]
        return self._target_rows(streams, tgt_inputs, None, langs, pad_idx, tgt_positions, proposals) + (batch_lang,)

    def _contrastive_loss(self, src_inputs, src_pads, src_langs, tgt_langs, batch, neg_samples, neg_mask):
        """src/image_model.py:231-264: the captions, the negative samples and the image regions pooled to unit vectors, and the
        image-to-text contrastive loss (one fused tail, ``_ContrastiveTailFn``).  Scalar fp32 loss."""
        device = self._device
        encoder_states, image_embeddings, src_pads = self._encode_text_and_image(src_inputs, src_pads, src_langs, batch)
        langs = tgt_langs if tgt_langs is not None else src_langs
        neg_samples, neg_mask = neg_samples.to(device), neg_mask.to(device)
        neg_langs = self._uniform_grid(neg_samples.size(0), neg_samples.size(-1), int(langs[0]), device)  # :235
        neg_states = MassSeq2Seq.encode(self, neg_samples, neg_mask, neg_langs)[0]
        anchor = store_of(self).ensure().anchor_if_grad()
        return _ContrastiveTailFn.apply(anchor, encoder_states, src_pads, neg_states, neg_mask, image_embeddings, self)

    def forward(self, src_inputs=None, src_pads=None, tgt_inputs=None, src_langs=None, tgt_langs=None, pad_idx: int = 0,
                tgt_positions=None, batch=None, neg_samples=None, neg_mask=None, proposals=None,
                log_softmax: bool = False, **kwargs):
        """``batch`` given (src/image_model.py:185-264): with ``neg_samples`` / ``neg_mask`` the scalar contrastive loss, else the
        gated text + image branch -- the decoder runs over the text encoder states (key mask ``src_pads``) and again over the image
        regions (no key mask), the two outputs are mixed by ``sigmoid(multimodal_attention_gate + 1e-7)``.

        Deviations from the reference's text, both forced: the image embeddings are element 0 of what the image head returns (the
        reference keeps the (grid, objects) tuple, :153, and fails); and ``tgt_langs``, which both branches read (:197, :235) but
        the reference trainer never passes (src/train_image_mt.py:218-236), defaults to ``src_langs`` -- the masked caption is
        recovered, and the negatives are written, in the captions' own language, as in the MASS step."""
        u = unwrap
        batch, src_langs, tgt_langs, src_pads = u(batch), u(src_langs), u(tgt_langs), u(src_pads)
        src_inputs, tgt_positions, tgt_inputs, proposals = u(src_inputs), u(tgt_positions), u(tgt_inputs), u(proposals)
        if batch is None:
            return MassSeq2Seq.forward(self, src_inputs=src_inputs, tgt_inputs=tgt_inputs, src_langs=src_langs,
                                       tgt_langs=tgt_langs, pad_idx=pad_idx, tgt_positions=tgt_positions,
                                       proposals=proposals, log_softmax=log_softmax)
        if neg_samples is not None:
            return self._contrastive_loss(src_inputs, src_pads, src_langs, tgt_langs, batch, u(neg_samples), u(neg_mask))
        rows, _, _, batch_lang = self._multimodal_rows(src_inputs, src_pads, tgt_inputs, src_langs, tgt_langs, pad_idx,
                                                       tgt_positions, batch, proposals)
        return self._project(rows, batch_lang, log_softmax)

    def loss_fused(self, src_inputs=None, src_pads=None, tgt_inputs=None, src_langs=None, tgt_langs=None,
                   pad_idx: int = 0, tgt_positions=None, batch=None, proposals=None, epsilon: float = 0.1, neg_samples=None,
                   neg_mask=None, **kwargs):
        """(loss, ntokens).  With ``batch``: the gated text + image branch through the fused projection + loss, or, with
        ``neg_samples``, the contrastive loss and 0 tokens (nothing is predicted, src/train_image_mt.py:274-276)."""
        u = unwrap
        batch, src_langs, tgt_langs, src_pads = u(batch), u(src_langs), u(tgt_langs), u(src_pads)
        src_inputs, tgt_positions, tgt_inputs, proposals = u(src_inputs), u(tgt_positions), u(tgt_inputs), u(proposals)
        if batch is None:
            return MassSeq2Seq.loss_fused(self, src_inputs, tgt_inputs, src_langs, tgt_langs=tgt_langs, pad_idx=pad_idx,
                                          tgt_positions=tgt_positions, epsilon=epsilon, proposals=proposals)
        if neg_samples is not None:
            return self._contrastive_loss(src_inputs, src_pads, src_langs, tgt_langs, batch, u(neg_samples), u(neg_mask)), 0
        rows, tgt_inputs, tgt_mask, batch_lang = self._multimodal_rows(src_inputs, src_pads, tgt_inputs, src_langs, tgt_langs, pad_idx,
                                                                       tgt_positions, batch, proposals)
        return self._loss_from_rows(rows, tgt_inputs, tgt_mask, batch_lang, epsilon)


class ImageCaptioning(ImageMassSeq2Seq):
    def __init__(self, text_processor, freeze_image: bool = False, resnet_depth: int = 1, lang_dec: bool = False,
                 use_proposals: bool = False, tie_embed: bool = False, enc_layer: int = 6, dec_layer: int = 3,
                 embed_dim: int = 768, intermediate_dim: int = 3072, use_obj: bool = True, *,
                 num_attention_heads: int = 12, image_feat_dim: int = None):
        super(ImageCaptioning, self).__init__(text_processor=text_processor, tie_embed=tie_embed, lang_dec=lang_dec,
                                              use_proposals=use_proposals, enc_layer=enc_layer, dec_layer=dec_layer,
                                              embed_dim=embed_dim, intermediate_dim=intermediate_dim,
                                              freeze_image=freeze_image, resnet_depth=resnet_depth,
                                              num_attention_heads=num_attention_heads, image_feat_dim=image_feat_dim)
        if use_obj:
            # object stream (detector features, :279-296): the object head's parameters live in image_model, the second
            # decoder is built from self.config (enc_layer layers, :281,287), not from dec_config
            self.image_model.add_object_head(self.config.hidden_size)
            tie = _Pretrained._tie_or_clone_weights
            if not lang_dec:
                self.obj_decoder = BertDecoderModel(self.config)
                if tie_embed:  # :284-285: only re-registers output_layer.weight (already the decoder's word table)
                    tie(self.output_layer, self.decoder.embeddings.word_embeddings)
            else:
                import copy
                dec = BertDecoderModel(self.config)
                self.obj_decoder = nn.ModuleList([copy.deepcopy(dec) for _ in text_processor.languages])
                for i, dec in enumerate(self.obj_decoder):  # :288-294, in the reference's order and argument order
                    if tie_embed:
                        dec.embeddings.position_embeddings = self.encoder.embeddings.position_embeddings
                    tie(self.output_layer[i], dec.embeddings.word_embeddings)
                    tie(self.encoder.embeddings.token_type_embeddings, dec.embeddings.token_type_embeddings)
            self.multistream_attention_gate = nn.Parameter(torch.zeros(1, self.config.hidden_size).fill_(0.1),
                                                           requires_grad=True)
            self._link_stacks()

    def flat_param_order(self):
        """The object stream's parameters go last in the flat store: every other parameter keeps the offset it has in a
        model without them (and so does every gradient a batch without objects makes nonzero).  The object decoders are
        laid out like the decoders (q|k|v and the cross key|value projections contiguous, as the stack runtime needs)."""
        ps = super().flat_param_order()
        obj = self._modules.get("obj_decoder")
        if obj is None:
            return ps
        img = self.image_model
        objs = list(obj) if isinstance(obj, nn.ModuleList) else [obj]
        head = [img.object_feat_fc.weight, img.object_embedding.weight]
        late = {id(p) for od in objs for p in od.parameters()} | {id(self.multistream_attention_gate)} | {id(p) for p in head}
        seen = {id(p) for p in ps}
        for p in self.parameters():
            if id(p) not in seen and id(p) not in late:
                seen.add(id(p))
                ps.append(p)
        for od in objs:
            ps += self._decoder_param_order(od)
        return ps + [p for od in objs for p in od.parameters()] + [self.multistream_attention_gate] + head

    def encode(self, src_inputs=None, src_mask=None, src_langs=None, images=None, objects=None):
        """Images: (image_embeddings, object_fc or None) (src/image_model.py:298-308).  ``objects`` (build extension):
        pre-extracted detector output in place of the frozen Faster-RCNN (see ``_objects_present``)."""
        if images is not None:
            image_embeddings, _ = self.image_model(unwrap(images), self._imt_compute_dtype)
            object_fc = None
            if "obj_decoder" in self._modules:
                object_fc = self.image_model.objects_forward(unwrap(objects), self._imt_compute_dtype)
            return image_embeddings, object_fc
        return MassSeq2Seq.encode(self, src_inputs, src_mask, src_langs)

    def _obj_decoder_for(self, batch_lang):
        return self.obj_decoder[batch_lang] if self.lang_dec else self.obj_decoder

    def _caption_rows(self, batch, src_pads, tgt_inputs, tgt_langs, tgt_mask, pad_idx, tgt_positions, proposals):
        tgt_positions, tgt_inputs, tgt_mask, tgt_langs, src_pads = map(unwrap, (tgt_positions, tgt_inputs, tgt_mask, tgt_langs, src_pads))
        image_embeddings, object_fc = self.encode(images=batch["images"], objects=batch.get("objects"))
        assert tgt_inputs is not None
        batch_lang = int(tgt_langs[0])
        streams = [DecoderStream(self._decoder_for(batch_lang), image_embeddings, src_pads, None)]
        if object_fc is not None:  # second decoder over the object rows, same key mask (None for caption batches, :357-361)
            streams.append(DecoderStream(self._obj_decoder_for(batch_lang), object_fc, src_pads, self.multistream_attention_gate))
        return self._target_rows(streams, tgt_inputs, tgt_mask, tgt_langs, pad_idx, tgt_positions, proposals) + (batch_lang,)

    def forward(self, src_inputs=None, src_pads=None, tgt_inputs=None, src_langs=None, tgt_langs=None, tgt_mask=None,
                pad_idx: int = 0, tgt_positions=None, batch=None, proposals=None, log_softmax: bool = False,
                encode_only: bool = False, **kwargs):
        batch = unwrap(batch)
        if batch is None or src_inputs is not None:  # text-based input (:318-320)
            return ImageMassSeq2Seq.forward(self, src_inputs=src_inputs, src_mask=src_pads, tgt_inputs=tgt_inputs,
                                            src_langs=src_langs, tgt_langs=tgt_langs, proposals=proposals,
                                            log_softmax=log_softmax)
        if encode_only:
            return self.encode(images=batch["images"])[0]
        rows, _, _, batch_lang = self._caption_rows(batch, src_pads, tgt_inputs, tgt_langs, tgt_mask, pad_idx,
                                                    tgt_positions, proposals)
        return self._project(rows, batch_lang, log_softmax)

    def loss_fused(self, src_inputs=None, src_pads=None, tgt_inputs=None, src_langs=None, tgt_langs=None, tgt_mask=None,
                   pad_idx: int = 0, tgt_positions=None, batch=None, proposals=None, epsilon: float = 0.1, **kwargs):
        batch = unwrap(batch)
        if batch is None or src_inputs is not None:
            return ImageMassSeq2Seq.loss_fused(self, src_inputs=src_inputs, tgt_inputs=tgt_inputs, src_langs=src_langs,
                                               tgt_langs=tgt_langs, pad_idx=pad_idx, epsilon=epsilon,
                                               proposals=proposals)
        rows, tgt_inputs, tgt_mask, batch_lang = self._caption_rows(batch, src_pads, tgt_inputs, tgt_langs, tgt_mask,
                                                                    pad_idx, tgt_positions, proposals)
        return self._loss_from_rows(rows, tgt_inputs, tgt_mask, batch_lang, epsilon)

    def score(self, *args, **kwargs):
        raise NotImplementedError("ImageCaptioning.score: image-conditioned scoring is not implemented (score text pairs "
                                  "with Seq2Seq / ImageMassSeq2Seq)")


class _SentPoolFn(torch.autograd.Function):
    """dropout -> one-vector attention -> weighted sum (src/image_model.py:430-436) as one node: ``imt_sent_pool_fwd``; the
    backward (``imt_sent_pool_bwd``) regenerates the dropout mask from the seed, returns the gradient the encoder stack
    receives and accumulates d(input_attention) into the flat gradient."""

    @staticmethod
    def forward(ctx, anchor, states, mask, model, p, seed):
        store = store_of(model).ensure()
        w, b = store.views(states.dtype, model.input_attention.weight, model.input_attention.bias)
        w = w.view(-1)  # nn.Linear(d, 1) weight is [1, d]
        x = states.contiguous()
        v, probs = O.sent_pool_fwd(x, w, b, mask, dropout_p=p, dropout_seed=seed)
        ctx.store, ctx.model, ctx.layout_version = store, model, store.layout_version
        ctx.mask, ctx.p, ctx.seed = mask, p, seed
        ctx.save_for_backward(x, w, probs)
        return v

    @staticmethod
    def backward(ctx, dv):
        x, w, probs = ctx.saved_tensors
        store, att = ctx.store, ctx.model.input_attention
        store.check_layout(ctx.layout_version, "sentence pooling")
        dx = O.sent_pool_bwd(x, w, ctx.mask, probs, dv.to(x.dtype).contiguous(), store.grad_view(att.weight).view(-1),
                             store.grad_view(att.bias), dropout_p=ctx.p, dropout_seed=ctx.seed)
        store.attach_grad_views()
        return None, dx, None, None, None, None


class _L2DistFn(torch.autograd.Function):
    """torch.dist(pred, target, 2) / B (src/train_txt2image.py:67): ``imt_l2_dist`` gives the loss and d loss / d pred in one
    call; an upstream gradient multiplies the saved gradient on the device (it is never read on the host; a factor of 1, what
    ``loss.backward()`` passes, leaves a bf16 gradient bit for bit, any other factor rounds it a second time)."""

    @staticmethod
    def forward(ctx, pred, target):
        loss, dpred = O.l2_dist(pred.contiguous(), target)
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g.detach().to(torch.float32).reshape(()), None  # a 0-d fp32 factor: dpred's dtype is kept


class Caption2Image(FlatStoreModel):
    REGIONS = 49

    def __init__(self, text_processor, enc_layer: int = 6, embed_dim: int = 768, intermediate_dim: int = 3072, *,
                 num_attention_heads: int = 12):
        super(Caption2Image, self).__init__()
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
        self.decoder = nn.Linear(self.config.hidden_size, self.REGIONS * self.config.hidden_size)
        self._imt_compute_dtype = torch.float32
        self._link_stacks()

    def _link_stacks(self):
        self.encoder.__dict__["_imt_owner"] = weakref.ref(self)

    def flat_param_order(self):
        """The order in which the gradients become final: the linear layer, the pooling vector, the encoder from the top."""
        ps = [self.decoder.weight, self.decoder.bias, self.input_attention.weight, self.input_attention.bias]
        for lyr in reversed(list(self.encoder.encoder.layer)):
            ps += lyr.ordered_params()
        e = self.encoder.embeddings
        return ps + [e.LayerNorm.weight, e.LayerNorm.bias, e.position_embeddings.weight, e.token_type_embeddings.weight,
                     e.word_embeddings.weight]

    @property
    def _device(self):
        return self.encoder.embeddings.word_embeddings.weight.device

    def encode(self, src_inputs, src_mask, src_langs):
        device = self._device
        if src_inputs.device != device:
            src_inputs = src_inputs.to(device)
            src_mask = src_mask.to(device)
            src_langs = src_langs.to(device)
        encoder_states = self.encoder(src_inputs, attention_mask=src_mask, token_type_ids=src_langs)
        return (encoder_states, None)

    def forward(self, src_inputs, src_mask, src_langs):
        """[B, 49 * d] in the compute dtype: encoder stack -> dropout (training) + attention pooling, one kernel -> linear."""
        src_inputs, src_mask, src_langs = unwrap(src_inputs), unwrap(src_mask), unwrap(src_langs)
        device = self._device
        src_langs = src_langs.unsqueeze(-1).expand(-1, src_inputs.size(-1)).to(device)
        src_inputs, src_mask = src_inputs.to(device), src_mask.to(device)
        encoder_states = self.encode(src_inputs, src_mask, src_langs)[0]
        p = float(self.config.hidden_dropout_prob) if self.training else 0.0
        seed = dropout_seed(self, p > 0)
        anchor = store_of(self).ensure().anchor_if_grad()
        sentence_embeddings = _SentPoolFn.apply(anchor, encoder_states, src_mask, self, p, seed)
        return _LinearFn.apply(sentence_embeddings, self.decoder.weight, self.decoder.bias, self)

    def loss_fused(self, src_inputs, src_mask, src_langs, image_encoding):
        """(loss, number of images): |forward(...) - image_encoding|_2 / B (src/train_txt2image.py:62-67).  ``image_encoding``
        ([B, 49, d] or [B, 49 * d], e.g. ``ImageCaptioning(batch=..., encode_only=True)``) is a constant."""
        pred = self(src_inputs, src_mask, src_langs)
        target = unwrap(image_encoding).detach()
        if target.size(0) != pred.size(0) or target.numel() != pred.numel():
            raise ValueError("Caption2Image: image_encoding %s does not match the %d x %d predictions" % (tuple(target.shape), pred.size(0), pred.size(1)))
        target = target.reshape(pred.shape).to(device=pred.device, dtype=pred.dtype).contiguous()
        return _L2DistFn.apply(pred, target), int(pred.size(0))

    def save(self, out_dir: str):
        if not os.path.exists(out_dir):
            os.makedirs(out_dir)
        with open(os.path.join(out_dir, "mt_config"), "wb") as fp:
            pickle.dump((self.enc_layer, self.embed_dim, self.intermediate_dim), fp)
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, os.path.join(out_dir, "mt_model.state_dict"))
        # build extension (the reference hard-codes 12 heads): beside the reference's files, as Seq2Seq.save does
        with open(os.path.join(out_dir, "imt_config.json"), "w") as fp:
            json.dump({"num_attention_heads": int(self.config.num_attention_heads)}, fp)

    @staticmethod
    def load(out_dir: str, tok_dir: str, text_processor=None):
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
        mt_model = Caption2Image(text_processor=text_processor, enc_layer=enc_layer, embed_dim=embed_dim,
                                 intermediate_dim=intermediate_dim, **kw)
        sd = torch.load(os.path.join(out_dir, "mt_model.state_dict"), map_location="cpu", weights_only=True)
        mt_model.load_state_dict(sd, strict=False)
        return mt_model.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))
