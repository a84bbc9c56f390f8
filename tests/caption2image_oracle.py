"""Plain-torch restatement of Caption2Image -- TEST INFRASTRUCTURE ONLY, written from the semantics of the reference
(src/image_model.py:380-440 the model, src/train_txt2image.py:62-67 the loss) on top of oracle.reference_model.  Runs in whatever
dtype the module is in (``.double()`` for an fp64 truth) and takes the dropout as an explicit keep-mask, so that a test can hand
it the mask the kernels draw from their seed.

  * pooling: xd = x * keep / (1 - p) (keep None: no dropout); score = xd . w + b, masked positions set to exactly -10000
    (masked_fill, :434); p = softmax over positions; v = sum_s p_s xd_s.  No normalisation (unlike the contrastive tail).
  * loss: |pred - target|_2 over the WHOLE [B, 49 d] tensors, divided by B (torch.dist(..., 2) / predictions.size(0)).
  * ``sent_pool_grads`` / ``l2_dist_grad`` restate the closed forms the kernels compute; tests/test_caption2image.py holds them
    against autograd of the forwards in fp64.
"""
import torch
import torch.nn as nn

from oracle import reference_model as R

REGIONS = 49


def dropped(x, keep=None, p=0.0):
    return x if keep is None else x * keep.to(x.dtype) / (1.0 - p)


def sent_pool(x, w, b, mask=None, keep=None, p=0.0):
    """(v [rows, d], probabilities [rows, S]) of x [rows, S, d]; w [d], b scalar tensor, mask bool [rows, S], keep bool like x."""
    xd = dropped(x, keep, p)
    scores = xd @ w + b
    if mask is not None:
        scores = scores.masked_fill(~mask, -10000.0)
    probs = torch.softmax(scores, dim=1)
    return torch.einsum("bfd,bf->bd", xd, probs), probs


def sent_pool_grads(x, w, mask, probs, dv, keep=None, p=0.0):
    """(dx, dw, db) of sent_pool for an upstream dv: dp_s = dv . xd_s; dscore = p (dp - sum p dp), zero at masked positions
    (their score is a constant); d(xd_s) = p_s dv + dscore_s w; dx = the dropout's backward of that."""
    xd = dropped(x, keep, p)
    dp = torch.einsum("bfd,bd->bf", xd, dv)
    ds = probs * (dp - (probs * dp).sum(1, keepdim=True))
    if mask is not None:
        ds = ds.masked_fill(~mask, 0.0)
    dxd = probs.unsqueeze(-1) * dv.unsqueeze(1) + ds.unsqueeze(-1) * w
    return dropped(dxd, keep, p), torch.einsum("bf,bfd->d", ds, xd), ds.sum()


def l2_dist(pred, target):
    return torch.dist(pred, target, 2) / pred.size(0)


def l2_dist_grad(pred, target):
    """d l2_dist / d pred; zeros where the distance is 0 (torch's subgradient of the norm at 0)."""
    diff = pred - target
    r = diff.pow(2).sum().sqrt()
    return torch.zeros_like(diff) if float(r) == 0.0 else diff / (r * pred.size(0))


class Caption2Image(nn.Module):
    """Same attribute tree and state-dict keys as the reference's class (encoder.*, input_attention.*, decoder.*)."""

    def __init__(self, text_processor, enc_layer: int = 6, embed_dim: int = 768, intermediate_dim: int = 3072, *,
                 num_attention_heads: int = 12):
        super().__init__()
        cfg = R.bert_config(vocab_size=text_processor.tokenizer.get_vocab_size(), pad_token_id=text_processor.pad_token_id(),
                            bos_token_id=text_processor.bos_token_id(), eos_token_id=text_processor.sep_token_id(),
                            enc_layer=enc_layer, embed_dim=embed_dim, intermediate_dim=intermediate_dim,
                            num_attention_heads=num_attention_heads)
        cfg["type_vocab_size"] = len(text_processor.languages)
        self.config = R.BertConfig(**cfg)
        self.encoder = R.BertEncoderModel(self.config)
        self.input_attention = nn.Linear(self.config.hidden_size, 1)
        self.decoder = nn.Linear(self.config.hidden_size, REGIONS * self.config.hidden_size)

    def states(self, src_inputs, src_mask, src_langs):
        langs = src_langs.unsqueeze(-1).expand(-1, src_inputs.size(-1))
        return self.encoder(src_inputs, attention_mask=src_mask, token_type_ids=langs)

    def tail(self, states, src_mask, keep=None, p=0.0):
        v, _ = sent_pool(states, self.input_attention.weight[0], self.input_attention.bias[0], src_mask, keep, p)
        return self.decoder(v)

    def forward(self, src_inputs, src_mask, src_langs, keep=None, p=0.0):
        """[B, 49 d]; ``keep`` / ``p``: the dropout in front of the pooling (the encoder itself runs in the module's mode)."""
        return self.tail(self.states(src_inputs, src_mask, src_langs), src_mask, keep, p)

    def loss(self, src_inputs, src_mask, src_langs, image_encoding, keep=None, p=0.0):
        pred = self(src_inputs, src_mask, src_langs, keep, p)
        return l2_dist(pred, image_encoding.reshape(pred.shape).to(pred.dtype))
