"""Plain-torch restatement of SenSim -- TEST INFRASTRUCTURE ONLY, written from the semantics of the reference (src/sen_sim.py)
on top of oracle.reference_model.  Runs in whatever dtype the module is in (``.double()`` for an fp64 truth).

  * sentence vector: score = x . w + b, masked positions set to exactly -10000, softmax over positions, weighted sum (``encode``);
    the unit vector is that divided by (|v|_2 + 1e-4).
  * ``normalize=False``: the pairs' dot products.  ``normalize=True`` without negatives: C = S T^T,
    sum_i (log(sum_j exp C_ij + 1e-4) - (C_ii + 1e-4)) / B.  With negatives (used only when ``src_neg_langs`` is given):
    ``two_sided_loss`` below.
  * ``two_sided_grads`` / ``pair_dot_grads`` restate the closed forms the kernels compute; tests/test_sensim.py holds them against
    autograd in fp64.
"""
import torch
import torch.nn as nn

from oracle import reference_model as R
from tests.multimodal_oracle import attn_pool


def two_sided_loss(scat, tcat, B):
    """scat [Ns, d] = [source negatives; B sources], tcat [Nt, d] = [target negatives; B targets], unit vectors.  Every source is
    scored against all of tcat and every target against all of scat; the two score rows of a pair share one denominator."""
    src, tgt = scat[scat.size(0) - B:], tcat[tcat.size(0) - B:]
    scores = torch.cat([src @ tcat.t(), tgt @ scat.t()], dim=1)
    denom = torch.log(torch.exp(scores).sum(-1) + 1e-4)
    nominator = (src * tgt).sum(-1) + 1e-4
    return (denom - nominator).sum() / B


def two_sided_grads(scat, tcat, B):
    """(d loss / d scat, d loss / d tcat) in closed form."""
    Ns, Nt = scat.size(0), tcat.size(0)
    src, tgt = scat[Ns - B:], tcat[Nt - B:]
    ea, em = torch.exp(src @ tcat.t()), torch.exp(tgt @ scat.t())
    D = ea.sum(-1, keepdim=True) + em.sum(-1, keepdim=True) + 1e-4
    dA, dM = ea / (D * B), em / (D * B)
    d_scat, d_tcat = dM.t() @ tgt, dA.t() @ src
    d_scat[Ns - B:] += dA @ tcat - tgt / B
    d_tcat[Nt - B:] += dM @ scat - src / B
    return d_scat, d_tcat


def one_sided_loss(src, tgt):
    cross = src @ tgt.t()
    return (torch.log(torch.exp(cross).sum(-1) + 1e-4) - (torch.diagonal(cross, 0) + 1e-4)).sum() / src.size(0)


def pair_dot(a, b):
    return (a * b).sum(-1)


def pair_dot_grads(a, b, g):
    return g.unsqueeze(-1) * b, g.unsqueeze(-1) * a


class SenSim(nn.Module):
    """Same attribute tree and state-dict keys as the reference's class (encoder.*, input_attention.*)."""

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

    def states(self, inputs, mask, langs):
        return self.encoder(inputs, attention_mask=mask, token_type_ids=langs.unsqueeze(-1).expand(-1, inputs.size(-1)))

    def encode(self, inputs, mask, langs):
        """The unnormalised sentence vectors; ``langs`` [rows]."""
        u, _, norm = attn_pool(self.states(inputs, mask, langs), self.input_attention.weight[0], self.input_attention.bias[0], mask)
        return u * (norm.unsqueeze(-1) + 1e-4)

    def unit(self, inputs, mask, langs):
        return attn_pool(self.states(inputs, mask, langs), self.input_attention.weight[0], self.input_attention.bias[0], mask)[0]

    def forward(self, src_inputs, src_mask, src_langs, tgt_inputs, tgt_mask, tgt_langs, src_neg_inputs=None, src_neg_mask=None,
                src_neg_langs=None, tgt_neg_inputs=None, tgt_neg_mask=None, tgt_neg_langs=None, normalize: bool = False):
        src, tgt = self.unit(src_inputs, src_mask, src_langs), self.unit(tgt_inputs, tgt_mask, tgt_langs)
        if not normalize:
            return pair_dot(src, tgt)
        if src_neg_langs is None:
            return one_sided_loss(src, tgt)
        sneg = self.unit(src_neg_inputs, src_neg_mask, src_neg_langs)
        tneg = self.unit(tgt_neg_inputs, tgt_neg_mask, tgt_neg_langs)
        return two_sided_loss(torch.cat([sneg, src]), torch.cat([tneg, tgt]), src.size(0))
