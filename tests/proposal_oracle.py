"""fp64 restatement of the lexical-proposal tail (src/seq2seq.py:110-144) in the row / group form of
``imt_proposal_attn_fwd``: forward, and gradients by autograd in double precision (CPU), and the bf16 error measurement that
the accuracy test and tools/proposal_bench.py share; then the edge cases of tests/test_gpu_proposal_edges.py with host
restatements of the backward's chain and scatter and of the contract for ids outside the table."""
import torch
import torch.nn.functional as F


def proposal_forward(x, table, prop, gate, gamma, beta, rows_per_group, pad_idx, eps, keep_e=None):
    """x [rows, d], table [V, d], gate / gamma / beta [d] (any float dtype; computed as given), prop [G, P] int64.  ``keep_e``:
    a list that receives the gathered rows e [G, P, d] with their gradient retained (proposal_reference, entry_grads)."""
    G, P = prop.shape
    d = x.shape[-1]
    e = F.embedding(prop, table, padding_idx=pad_idx)                # [G, P, d]; the pad row receives no gradient (:116)
    if keep_e is not None:
        e.retain_grad()
        keep_e.append(e)
    xg = x.view(G, rows_per_group, d)
    s = torch.einsum("grd,gpd->grp", xg, e)                          # pad entries take part: the fill at :132 is a no-op
    p = torch.softmax(s, dim=-1)
    c = torch.einsum("grp,gpd->grd", p, e)
    all_pad = (prop == pad_idx).all(-1)
    c = c.masked_fill(all_pad.view(G, 1, 1), 1e-8)                   # :137-138
    sg = torch.sigmoid(gate.view(-1) + 1e-8)
    z = sg * xg + (1 - sg) * c
    return F.layer_norm(z, (d,), gamma, beta, eps).view(-1, d)


def proposal_reference(x, table, prop, gate, gamma, beta, rows_per_group, pad_idx, eps, dy, entry_grads=False):
    """Everything in double: {"y", "dx", "dtable", "dgate", "dgamma", "dbeta"} for the upstream gradient dy; with
    ``entry_grads`` also "de" [G, P, d], the gradient of every gathered row before the rows of one id are summed (what the
    kernel's group launch writes; the rows of pad entries are not zero there, they are dropped by the sum)."""
    leaves = [t.detach().double().cpu().clone().requires_grad_(True) for t in (x, table, gate.view(-1), gamma, beta)]
    keep = [] if entry_grads else None
    y = proposal_forward(leaves[0], leaves[1], prop.cpu(), leaves[2], leaves[3], leaves[4], rows_per_group, pad_idx, eps, keep)
    y.backward(dy.detach().double().cpu())
    out = {"y": y.detach()}
    for name, t in zip(("dx", "dtable", "dgate", "dgamma", "dbeta"), leaves):
        out[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    if entry_grads:
        out["de"] = keep[0].grad
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


# ------------------------------------------------------------------------------------------- edge cases of csrc/proposal.hip
# (G, rows_per_group, P, d) -> the E-tile splits of P the case is there for, per dtype (tests/test_gpu_proposal_edges.py runs
# them, tests/test_proposal_host.py checks that the inputs have the properties)
EDGE_CASES = {
    (20, 3, 130, 64): {"fp32": [64, 64, 2], "bf16": [64, 64, 2]},      # n = 2600: 3 chain chunks, 11 chain workgroups
    (9, 1, 257, 128): {"fp32": [64] * 4 + [1], "bf16": [64] * 4 + [1]},  # n = 2313, one row per group
    (3, 17, 9, 1024): {"fp32": [8, 1], "bf16": [9]},                   # KD = 4, the smallest PT, rpg = 16 + 1 = 2 x 8 + 1
    (3, 8, 64, 260): {"fp32": [31, 31, 2], "bf16": [63, 1]},           # KD = 2 with one live lane in the second slice
    (4, 9, 33, 516): {"fp32": [15, 15, 3], "bf16": [31, 2]},           # KD = 3, partial
    (3, 16, 65, 12): {"fp32": [64, 1], "bf16": [64, 1]},               # d / 4 = 3 does not divide 256
    (1, 1, 4, 4): {"fp32": [4], "bf16": [4]},                          # the smallest d
    (3, 5, 64, 128): {"fp32": [64], "bf16": [64]},                     # P == PT
    (3, 5, 128, 128): {"fp32": [64, 64], "bf16": [64, 64]},            # P == 2 PT
}
CHAIN_CASES = [(20, 3, 130, 64), (9, 1, 257, 128)]
CHAIN_CHUNK, CHAIN_THREADS = 1024, 256  # PROP_CHAIN_CHUNK and the workgroup of prop_chain_kernel
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def tile_splits(dtype_bytes, d, P):
    """The E-tile lengths of csrc/proposal.hip: PT = min(64, 32768 / (d * bytes), P), then P in steps of PT."""
    pt = max(1, min(64, 32768 // (d * dtype_bytes), P))
    return [min(pt, P - j0) for j0 in range(0, P, pt)]


def round_inputs(c, dtype):
    """The case with x, table and dy rounded to ``dtype`` (kept as fp32 values): what the kernel is given in that dtype, and
    what the oracle is given, bit for bit."""
    c = dict(c)
    for k in ("x", "table", "dy"):
        c[k] = c[k].to(dtype).float()
    return c


_edge_cache = {}


def edge_case(shape, dtype_name, pad_idx=0):
    """(case, fp64 reference) of one edge shape with its inputs rounded to the dtype; computed once per process and shared
    (nobody writes into either)."""
    key = (shape, dtype_name, pad_idx)
    if key not in _edge_cache:
        G, rpg, P, d = shape
        c = round_inputs(make_case(G, rpg, P, d, seed=P, pad_idx=pad_idx), DTYPES[dtype_name])
        _edge_cache[key] = (c, proposal_reference(**c))
    return _edge_cache[key]


def live_entries(prop, V, pad_idx):
    """[G, P] bool: the entries that receive a gradient -- not pad, and inside [0, V)."""
    return (prop != pad_idx) & (prop >= 0) & (prop < V)


def untouched_rows(prop, V, pad_idx):
    """[V] bool: the table rows whose gradient the backward must leave alone: the pad row and every row no live entry names."""
    rows = torch.ones(V, dtype=torch.bool)
    rows[prop[live_entries(prop, V, pad_idx)]] = False
    return rows


def one_row_per_entry(c):
    """The same problem with every entry (g, j) naming a table row of its own: prop2 = 1 + the flat entry index (pad entries stay
    pad), table2[1 + i] = table[prop.flatten()[i]], row 0 the pad row.  States, parameters and dy are shared, so y, dx and the
    gathered gradients are the same numbers and dtable2[1 + i] holds entry i's alone."""
    assert c["pad_idx"] == 0
    prop = c["prop"]
    n = prop.numel()
    prop2 = torch.arange(1, n + 1).view_as(prop).clone()
    prop2[prop == 0] = 0
    c2 = dict(c)
    c2["prop"] = prop2
    c2["table"] = torch.cat([c["table"][:1], c["table"][prop.flatten()]])
    return c2


def sum_in_entry_order(prop, dtable2, V):
    """dtable [V, d] from the per-entry rows of one_row_per_entry's problem: per id the rows of its entries added one after the
    other in entry order, each add in dtable2's dtype (no sum(): its order is not ours to choose)."""
    flat = prop.flatten()
    out = torch.zeros(V, dtable2.shape[1], dtype=dtable2.dtype)
    live = (flat != 0).nonzero().flatten()
    order = live[torch.sort(flat[live], stable=True).indices]        # by id, entries of one id in entry order
    ids = flat[order]
    start = torch.cat([torch.ones(1, dtype=torch.bool), ids[1:] != ids[:-1]])
    pos = torch.arange(ids.numel())
    rank = pos - torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 0).values  # 0 for an id's first entry, 1, 2, ...
    for r in range(int(rank.max()) + 1):
        sel = rank == r                                              # at most one entry per id: a plain indexed add
        rows = dtable2[1 + order[sel]]
        out[ids[sel]] = rows if r == 0 else out[ids[sel]] + rows    # starts from the first entry's value
    return out


def chain_links(prop, V, pad_idx, forget_across_chunks=False):
    """(next, first) per flat entry as prop_chain_kernel forms them: next[i] the next entry with the same id or -1, first[i]
    whether no earlier entry has it; pad and out-of-range entries get (-1, False).  The ids are scanned in chunks of CHAIN_CHUNK.
    ``forget_across_chunks`` restates a kernel that restarts its two results with every chunk, so that only the last chunk's
    survive: the mistake the multi-chunk cases are there to catch."""
    flat = prop.flatten()
    n = flat.numel()
    live = live_entries(flat, V, pad_idx)
    nxt, first = torch.full((n,), -1, dtype=torch.long), torch.zeros(n, dtype=torch.bool)
    for i in live.nonzero().flatten().tolist():
        nx, has_prev = -1, False
        for k0 in range(0, n, CHAIN_CHUNK):
            if forget_across_chunks:
                nx, has_prev = -1, False
            kk = k0 + (flat[k0:k0 + CHAIN_CHUNK] == flat[i]).nonzero().flatten()
            has_prev = has_prev or bool((kk < i).any())
            later = kk[kk > i]
            if nx < 0 and later.numel():
                nx = int(later[0])
        nxt[i], first[i] = nx, not has_prev
    return nxt, first


def scatter_chains(prop, de, nxt, first, V):
    """prop_scatter_kernel on the host: every first entry adds the rows of ``de`` [n, d] along its chain and adds the sum to its
    id's row of a zero [V, d]."""
    flat = prop.flatten()
    out = torch.zeros(V, de.shape[1], dtype=de.dtype)
    for i in first.nonzero().flatten().tolist():
        acc, k = torch.zeros(de.shape[1], dtype=de.dtype), i
        while k >= 0:
            acc = acc + de[k]
            k = int(nxt[k])
        out[flat[i]] += acc
    return out


OUT_OF_RANGE = (-1, 0, 7, 2 ** 40)  # ids written as (-1, V, V + 7, 2^40): below, just past, past and far past the table


def with_out_of_range_ids(c):
    """The case (G >= 2, P >= 7) with four live entries of groups 0 and 1 overwritten by ids outside [0, V); both groups keep
    live ids (the repeated one among them), so neither turns all-pad."""
    V = c["table"].shape[0]
    prop = c["prop"].clone()
    ids = [OUT_OF_RANGE[0], V + OUT_OF_RANGE[1], V + OUT_OF_RANGE[2], OUT_OF_RANGE[3]]
    for (g, j), v in zip(((0, 2), (0, 4), (1, 1), (0, 6)), ids):
        assert int(prop[g, j]) != c["pad_idx"]
        prop[g, j] = v
    c = dict(c)
    c["prop"] = prop
    return c


def out_of_range_reference(c):
    """proposal_reference under the contract of include/imt_hip.h for ids outside [0, V): they read row 0 and get no gradient.
    A copy of table[0] is appended as row V, the ids are pointed at it, and that row's gradient is dropped -- which also holds
    when row 0 is not the pad row, and changes nothing when every id is in range."""
    V = c["table"].shape[0]
    c2 = dict(c)
    c2["table"] = torch.cat([c["table"], c["table"][:1]])
    c2["prop"] = torch.where((c["prop"] < 0) | (c["prop"] >= V), torch.full_like(c["prop"], V), c["prop"])
    want = proposal_reference(**c2)
    want["dtable"] = want["dtable"][:V].clone()
    return want
