"""Masked language model -- counterpart of src/lm.py: the encoder stack and a vocabulary projection whose weight IS the word
embedding table (``:40``; the reference names a ``.decoder`` that ``BertOutputLayer`` does not have -- its linear layer is
``.layer``, which is what is tied here).  ``forward`` gives the log-probs of the masked positions as the
reference does (``:42-55``); ``loss_fused`` is the training path: encoder stack -> rows at the masked positions -> fused
projection + log-softmax + NLL, the mean over the masked tokens (``nn.NLLLoss(ignore_index=pad)`` of src/train_lm.py:33,64).

The tied table has TWO gradient writers, the vocabulary projection's weight-gradient GEMM and the embedding backward's
scatter-add; both accumulate into the same span of the flat gradient (the store holds a tied parameter once), so after the
backward it holds their sum.  One process, one GPU: under data parallelism the output hook would release the projection's
bucket before the embedding backward has added to the table."""
import os
import weakref

import torch

from . import lm_config
from .bert_seq2seq import BertConfig, BertEncoderModel, BertOutputLayer
from .safe_pickle import load_lm_config, save_lm_config  # ``config``: a plain dict, nothing from the file is executed
from .seq2seq import FlatStoreModel, _FusedXentFn, _LogSoftmaxFn, _SelectRowsFn


class LM(FlatStoreModel):
    def __init__(self, text_processor, config=None, encoder=None, enc_layer: int = 6, embed_dim: int = 768,
                 intermediate_dim: int = 3072, *, num_attention_heads: int = 12):
        super(LM, self).__init__()
        self.text_processor = text_processor
        if config is None:
            config = lm_config.get_config(vocab_size=text_processor.tokenizer.get_vocab_size(),
                                          pad_token_id=text_processor.pad_token_id(),
                                          bos_token_id=text_processor.bos_token_id(),
                                          eos_token_id=text_processor.sep_token_id(),
                                          enc_layer=enc_layer, embed_dim=embed_dim, intermediate_dim=intermediate_dim,
                                          num_attention_heads=num_attention_heads)
            config["type_vocab_size"] = len(text_processor.languages)
        if isinstance(config, dict):
            config = BertConfig(**config)
        self.config = config
        self.masked_lm = BertOutputLayer(self.config)
        if encoder is None:
            self.encoder = BertEncoderModel(self.config)
            self.encoder.init_weights()
        else:
            self.encoder = encoder
        self.masked_lm.layer.weight = self.encoder.embeddings.word_embeddings.weight  # src/lm.py:40 (the bias stays its own)
        self._imt_compute_dtype = torch.float32
        self._link_stacks()

    def _link_stacks(self):
        ref = weakref.ref(self)
        for name in ("encoder", "masked_lm"):
            mod = self.__dict__.get("_modules", {}).get(name)
            if mod is not None:
                mod.__dict__["_imt_owner"] = ref

    def flat_param_order(self):
        """The order in which the gradients become final: the projection's bias, the encoder from the top, the embeddings -- the
        tied table last, because the embedding backward is its second writer."""
        ps = [self.masked_lm.layer.bias]
        for lyr in reversed(list(self.encoder.encoder.layer)):
            ps += lyr.ordered_params()
        e = self.encoder.embeddings
        return ps + [e.LayerNorm.weight, e.LayerNorm.bias, e.position_embeddings.weight, e.token_type_embeddings.weight,
                     e.word_embeddings.weight]

    @property
    def _device(self):
        return self.encoder.embeddings.word_embeddings.weight.device

    def _states(self, texts, pads, langs):
        """Encoder states [B, S, d]; ``langs`` [B] (or [B, 1]) is expanded over the positions (src/lm.py:47)."""
        device = self._device
        texts, pads = texts.to(device), pads.to(device)
        langs = langs.to(device).reshape(-1).unsqueeze(1).expand(-1, texts.size(1))
        return self.encoder(texts, attention_mask=pads, token_type_ids=langs)

    def forward(self, mask, texts, pads, langs=None):
        """fp32 log-probs [n_masked, V] of the positions where ``mask`` is set, in the order of ``texts[mask]``."""
        states = self._states(texts, pads, langs)
        idx = torch.nonzero(mask.to(self._device).reshape(-1), as_tuple=False).view(-1).to(torch.int32)
        if idx.numel() == 0:
            return torch.zeros((0, self.config.vocab_size), dtype=torch.float32, device=self._device)
        rows = _SelectRowsFn.apply(states.reshape(-1, states.size(-1)), idx)
        return _LogSoftmaxFn.apply(self.masked_lm(rows))

    def loss_fused(self, texts, pads, langs, idx, targets):
        """(loss, n) == ``nn.NLLLoss(ignore_index=pad)(self(mask, texts, pads, langs), targets)`` with ``idx`` the flat positions
        of the masked tokens (int32, row-major: ``mask_text_device``'s ``idx``) and ``targets`` their original ids, without the
        fp32 [n, V] matrix.  A pad is never masked, so the mean is over all ``n`` rows.  ``n == 0``: a zero loss that needs no
        backward."""
        n = int(targets.numel())
        device = self._device
        if n == 0:
            return torch.zeros((), dtype=torch.float32, device=device), 0
        if int(idx.numel()) != n:
            raise ValueError("LM.loss_fused: %d positions for %d targets" % (int(idx.numel()), n))
        states = self._states(texts, pads, langs)
        rows = _SelectRowsFn.apply(states.reshape(-1, states.size(-1)), idx.to(device=device, dtype=torch.int32))
        layer = self.masked_lm.layer
        loss = _FusedXentFn.apply(rows, layer.weight, layer.bias, targets.to(device).contiguous(), 0.0,
                                  int(self.text_processor.pad_token_id()))
        return loss, n

    def load_state_dict(self, state_dict, *args, **kwargs):
        """``encoder.pooler.*`` (the reference's encoder is a ``BertModel``; it never uses the pooled output) is ignored."""
        state_dict = {k: v for k, v in state_dict.items() if not k.startswith("encoder.pooler.")}
        return super().load_state_dict(state_dict, *args, **kwargs)

    def save(self, out_dir: str):
        """The reference's file names (src/lm.py:57-64): ``config`` -- here a pickle of a PLAIN DICT of the config fields,
        ``num_attention_heads`` among them --, ``model.state_dict`` and the tokenizer's files."""
        if not os.path.exists(out_dir):
            os.makedirs(out_dir)
        save_lm_config(self.config.to_dict(), os.path.join(out_dir, "config"))  # (a field that is no scalar is an error)
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, os.path.join(out_dir, "model.state_dict"))
        save_tokenizer = getattr(self.text_processor, "save", None)  # (the synthetic processors have no tokenizer to write)
        if save_tokenizer is not None:
            save_tokenizer(out_dir)

    @staticmethod
    def load(out_dir: str, text_processor=None):
        if text_processor is None:
            from .textprocessor import TextProcessor
            text_processor = TextProcessor(tok_model_path=out_dir)
        lm = LM(text_processor=text_processor, config=load_lm_config(os.path.join(out_dir, "config")))
        sd = torch.load(os.path.join(out_dir, "model.state_dict"), map_location="cpu", weights_only=True)
        lm.load_state_dict(sd)
        return lm.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

