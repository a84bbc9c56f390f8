"""fp64 restatement of the lexical-proposal tail (src/seq2seq.py:110-144) in the row / group form of
``imt_proposal_attn_fwd``: forward, and gradients by autograd in double precision (CPU), and the bf16 error measurement that
the accuracy test and tools/proposal_bench.py share."""
import torch
import torch.nn.functional as F


def proposal_forward(x, table, prop, gate, gamma, beta, rows_per_group, pad_idx, eps):
    """x [rows, d], table [V, d], gate / gamma / beta [d] (any float dtype; computed as given), prop [G, P] int64."""
    G, P = prop.shape
    d = x.shape[-1]
    e = F.embedding(prop, table, padding_idx=pad_idx)                # [G, P, d]; the pad row receives no gradient (:116)
    xg = x.view(G, rows_per_group, d)
    s = torch.einsum("grd,gpd->grp", xg, e)                          # pad entries take part: the fill at :132 is a no-op
    p = torch.softmax(s, dim=-1)
    c = torch.einsum("grp,gpd->grd", p, e)
    all_pad = (prop == pad_idx).all(-1)
    c = c.masked_fill(all_pad.view(G, 1, 1), 1e-8)                   # :137-138
    sg = torch.sigmoid(gate.view(-1) + 1e-8)
    z = sg * xg + (1 - sg) * c
    return F.layer_norm(z, (d,), gamma, beta, eps).view(-1, d)


def proposal_reference(x, table, prop, gate, gamma, beta, rows_per_group, pad_idx, eps, dy):
    """Everything in double: {"y", "dx", "dtable", "dgate", "dgamma", "dbeta"} for the upstream gradient dy."""
    leaves = [t.detach().double().cpu().clone().requires_grad_(True) for t in (x, table, gate.view(-1), gamma, beta)]
    y = proposal_forward(leaves[0], leaves[1], prop.cpu(), leaves[2], leaves[3], leaves[4], rows_per_group, pad_idx, eps)
    y.backward(dy.detach().double().cpu())
    out = {"y": y.detach()}
    for name, t in zip(("dx", "dtable", "dgate", "dgamma", "dbeta"), leaves):
        out[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    return out


def make_case(G, rows_per_group, P, d, seed=0, V=300, pad_idx=0):
    """Inputs of one kernel case.  Table rows are N(0, 0.02) times 20, so that with x ~ N(0, 1) the scores have a standard
    deviation of about 0.4 sqrt(d): the softmax is neither uniform nor one-hot.  Ids are drawn from [1, 200): rows 200 .. V - 1
    are never proposed.  With G >= 3 and P >= 4: group 1 is half pad, group 2 all pad, one id is repeated inside group 0 and
    again in group 1.  The pad row of the table is not zero (pad entries take part in the softmax)."""
    g = torch.Generator().manual_seed(1000 + seed)
    rows = G * rows_per_group
    x = torch.randn(rows, d, generator=g)
    table = torch.randn(V, d, generator=g) * 0.02 * 20
    prop = torch.randint(1, 200, (G, P), generator=g)
    if G >= 3 and P >= 4:
        prop[1, P // 2:] = pad_idx
        prop[2, :] = pad_idx
        prop[0, 1] = prop[0, 0]
        prop[1, 0] = prop[0, 0]
    gate = torch.randn(d, generator=g) * 0.5
    gamma = 1.0 + 0.1 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g)
    return dict(x=x, table=table, prop=prop, gate=gate, gamma=gamma, beta=beta, dy=dy, rows_per_group=rows_per_group,
                pad_idx=pad_idx, eps=1e-12)


def bf16_errors(G, rows_per_group, P, d):
    """{"fused" | "torch": {tensor: max-norm relative error}} of Seq2Seq.attend_proposal (the kernel pair) and
    Seq2Seq._attend_proposal_torch in bf16 compute, each against the fp64 restatement evaluated on the bf16-rounded states,
    table and upstream gradient of make_case(G, rows_per_group, P, d).  Needs the GPU."""
    from imagetranslate_amd.seq2seq import Seq2Seq
    from oracle.reference_model import SyntheticTextProcessor
    from tests.util import rel_err
    c = make_case(G, rows_per_group, P, d, seed=P, V=1000)
    for k in ("x", "table", "dy"):
        c[k] = c[k].bfloat16().float()
    torch.manual_seed(3)
    m = Seq2Seq(SyntheticTextProcessor(1000), lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=d, intermediate_dim=2 * d,
                num_attention_heads=4, use_proposals=True).cuda().eval()
    table_p, ln = m.proposal_embedding.weight, m.lexical_layer_norm
    with torch.no_grad():
        table_p.copy_(c["table"])
        m.lexical_gate.copy_(c["gate"].view(1, -1))
        ln.weight.copy_(c["gamma"])
        ln.bias.copy_(c["beta"])
    c["eps"] = ln.eps
    m.set_compute_dtype(torch.bfloat16)
    want = proposal_reference(**c)
    prop = c["prop"].cuda()
    errs = {}
    for name, fn in (("fused", m.attend_proposal), ("torch", m._attend_proposal_torch)):
        m.zero_grad()
        x = c["x"].cuda().bfloat16().view(G, rows_per_group, d).requires_grad_(True)
        y = fn(x, prop, c["pad_idx"])
        assert y.dtype == torch.bfloat16
        y.backward(c["dy"].cuda().bfloat16().view(G, rows_per_group, d))
        got = dict(y=y.view(-1, d), dx=x.grad.view(-1, d), dtable=table_p.grad, dgate=m.lexical_gate.grad.view(-1),
                   dgamma=ln.weight.grad, dbeta=ln.bias.grad)
        errs[name] = {k: rel_err(v.float(), want[k]) for k, v in got.items()}
    return errs
