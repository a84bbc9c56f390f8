"""csrc/proposal.hip (imt_proposal_attn_fwd / imt_proposal_attn_bwd) where its loops wrap and its tails begin, against the fp64
restatement of tests/proposal_oracle.py.  tests/test_gpu_proposal.py stops at G * P = 260 entries, d in {64, 128, 512, 768},
zero gradient buffers and pad_idx 0; the cases here (proposal_oracle.EDGE_CASES, (G, rows_per_group, P, d)) reach

  * the chain kernel's second and third chunk of 1024 ids and its eleventh workgroup (n = 2600 and 2313 entries, ids repeated
    on both sides of every boundary);
  * KD = 4 (d = 1024), a last 256-column slice with one live lane (d = 260) or a few (d = 516), d = 4, and d / 4 = 3 threads per
    proposal in the group kernel;
  * E tiles of 8, 15, 16, 31 and 63 proposals, P == PT, P == 2 PT and a tail of one proposal;
  * 1, 8, 16 and 17 rows per group (the forward's row tile is 16, the backward's 8), all-pad groups under a multi-tile P.

tests/test_proposal_host.py shows without a GPU that the inputs have these properties.  Per case and dtype: y and the five
gradients against fp64, two calls bit for bit, untouched table rows exactly zero.  bf16 runs on bf16-rounded x, table and dy,
which the oracle receives bit for bit: y and dx are rounded once on the way out (2^-8 of the tensor's maximum, the bound
tests/test_gpu_multimodal.py derives for DX_TOL), while dtable, dgate, dgamma and dbeta are fp32 sums of fp32 products of those
inputs and are held to the fp32 contract.  Every test prints ``PROPEDGE ...`` lines with the measured errors before it asserts.

Measured on an MI355X when the module was written (max-norm relative error; fp32: the worst of the six tensors, bf16: y, dx, and
the worst of the four parameter gradients); no case needed a change to the kernels:

  case                          fp32 worst        bf16 y    bf16 dx   bf16 parameter gradients
  (20, 3, 130, 64)              2.0e-6 (dx)       1.7e-3    1.8e-3    2.4e-6 (dtable)
  (9, 1, 257, 128)              4.8e-6 (dx)       1.7e-3    2.6e-3    8.6e-7 (dtable)
  (3, 17, 9, 1024)              8.9e-7 (dtable)   2.7e-3    2.0e-3    6.7e-7 (dtable)
  (3, 8, 64, 260)               4.9e-6 (dtable)   2.5e-3    3.0e-3    2.9e-6 (dtable)
  (4, 9, 33, 516)               2.2e-6 (dtable)   3.1e-3    2.7e-3    2.7e-6 (dtable)
  (3, 16, 65, 12)               1.4e-6 (dx)       2.4e-3    1.9e-3    5.6e-7 (dtable)
  (1, 1, 4, 4)                  8.7e-8 (dgate)    2.9e-3    1.5e-3    2.6e-7 (dtable)
  (3, 5, 64, 128)               2.0e-6 (dtable)   2.0e-3    1.7e-3    2.3e-6 (dtable)
  (3, 5, 128, 128)              3.1e-6 (dtable)   2.8e-3    1.7e-3    2.1e-6 (dtable)
  (3, 5, 7, 128) pad 5          3.7e-7 (dtable)   1.9e-3    2.2e-3    3.2e-7 (dtable)
  (3, 5, 7, 128) ids out, pad 0 3.7e-7 (dtable)   1.9e-3    3.4e-3    4.2e-7 (dtable)
  (3, 5, 7, 128) ids out, pad 5 2.3e-7 (dx)       1.9e-3    2.9e-3    2.6e-7 (dtable)

Bounds: 1e-4 (fp32, and the bf16 parameter gradients: held as derived everywhere), 2^-8 = 3.9e-3 (bf16 y and dx).  Entry-order
check: 0 of 300 table rows differ in both chain cases.  Accumulation: 3.8e-8 .. 4.6e-8 of the tensor's scale (bound 1e-6)."""
import pytest
import torch

from imagetranslate_amd import hip_ops as O
from tests import proposal_oracle as PO
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

proposal_attn, proposal_attn_bwd = O.proposal_attn, O.proposal_attn_bwd  # without the feature the module fails here

GRADS = ("dx", "dtable", "dgate", "dgamma", "dbeta")
PARAM_GRADS = ("dtable", "dgate", "dgamma", "dbeta")
FP32_TOL = 1e-4      # the project's fp32 contract (tests/test_gpu_proposal.py)
BF16_OUT_TOL = 2.0 ** -8  # one rounding of an output to bf16
SHAPE_ID = lambda s: "G%d_r%d_P%d_d%d" % s


def _tol(name, dtype_name):
    return BF16_OUT_TOL if dtype_name == "bf16" and name in ("y", "dx") else FP32_TOL


def _run(c, dtype_name, init=None):
    """One forward + backward through hip_ops on the case's tensors in the dtype; the parameter gradients accumulate into zero
    buffers, or into copies of ``init`` ({name: fp32 tensor})."""
    dev, dtype = "cuda", PO.DTYPES[dtype_name]
    x, table, dy = (c[k].to(dev, dtype).contiguous() for k in ("x", "table", "dy"))
    prop = c["prop"].to(dev)
    gate, gamma, beta = (c[k].to(dev).contiguous() for k in ("gate", "gamma", "beta"))
    y, scores, stats = proposal_attn(x, table, prop, gate, gamma, beta, c["rows_per_group"], c["pad_idx"], c["eps"])
    d = x.shape[1]
    shapes = dict(dtable=tuple(table.shape), dgate=(d,), dgamma=(d,), dbeta=(d,))
    g = {k: torch.zeros(s, device=dev) if init is None else init[k].to(dev).clone() for k, s in shapes.items()}
    dx = proposal_attn_bwd(dy, x, table, prop, gate, gamma, scores, stats, g["dtable"], g["dgate"], g["dgamma"], g["dbeta"],
                           c["rows_per_group"], c["pad_idx"])
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, **g)


def _check(c, want, dtype_name, what):
    """Accuracy of the six tensors, repeatability, untouched table rows; returns the first run."""
    got, again = _run(c, dtype_name), _run(c, dtype_name)
    errs = {k: rel_err(got[k].float(), want[k]) for k in ("y",) + GRADS}
    print("PROPEDGE %s %s %s" % (what, dtype_name, " ".join("%s=%.2e" % kv for kv in errs.items())))
    for k in ("y",) + GRADS:
        assert_close(got[k].float(), want[k], _tol(k, dtype_name), "%s %s %s" % (k, what, dtype_name))
    for k in ("y",) + GRADS:
        assert torch.equal(got[k], again[k]), "%s differs between two calls" % k
    dt = got["dtable"].cpu()
    rows = PO.untouched_rows(c["prop"], dt.shape[0], c["pad_idx"])
    assert bool(rows[c["pad_idx"]])
    assert float(dt[rows].abs().max()) == 0.0, "the pad row or a table row that no live proposal names got a gradient"
    return got


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(PO.EDGE_CASES), ids=SHAPE_ID)
def test_edge_case_against_fp64(cuda, shape, dtype_name):
    """fp32: 1e-4 max-norm relative on all six tensors (a plain fp32 restatement of the op is within 3e-6 of fp64 on these cases,
    so a miss is not round-off).  bf16: 2^-8 on y and dx, 1e-4 on the four parameter gradients.  Two calls give the same bits;
    the pad row of dtable and every row no live entry names are exactly zero."""
    c, want = PO.edge_case(shape, dtype_name)
    _check(c, want, dtype_name, SHAPE_ID(shape))


@pytest.mark.parametrize("shape", PO.CHAIN_CASES, ids=SHAPE_ID)
def test_every_entry_once_in_entry_order(cuda, shape):
    """One writer, every entry once, in entry order -- exactly.  The same problem with a table row per entry
    (proposal_oracle.one_row_per_entry) leaves each entry's gathered gradient on a row of its own; adding those rows per
    original id one after the other in entry order, in fp32 on the host, must give the original dtable bit for bit: a lost, a
    doubled or a reordered link at any chunk or workgroup boundary changes bits whatever the tolerance."""
    c, _ = PO.edge_case(shape, "fp32")
    c2 = PO.one_row_per_entry(c)
    got, got2 = _run(c, "fp32"), _run(c2, "fp32")
    for k in ("y", "dx", "dgate", "dgamma", "dbeta"):
        assert torch.equal(got[k], got2[k]), k  # the ids only choose where the gradient lands
    want = PO.sum_in_entry_order(c["prop"], got2["dtable"].cpu(), c["table"].shape[0])
    dt = got["dtable"].cpu()
    differ = int((dt != want).any(1).sum())
    print("PROPEDGE %s entry order: %d of %d table rows differ, rel err %.2e" % (SHAPE_ID(shape), differ, dt.shape[0], rel_err(dt, want)))
    assert torch.equal(dt, want), "%d table rows are not the sum of their entries in entry order" % differ


def test_parameter_gradients_accumulate(cuda):
    """dtable, dgate, dgamma and dbeta are ACCUMULATED: a run into buffers of small integers (|v| <= 4) gives init + the run
    into zero buffers, to 1e-6 of the tensor's scale (one fp32 addition of values of 1 .. 30 rounds by at most 6e-8 of
    them), and table rows that no entry names keep their bits."""
    shape = (4, 9, 33, 516)
    c, _ = PO.edge_case(shape, "fp32")
    g = torch.Generator().manual_seed(17)
    d, V = shape[3], c["table"].shape[0]
    init = {k: torch.randint(-4, 5, s, generator=g).float() for k, s in (("dtable", (V, d)), ("dgate", (d,)), ("dgamma", (d,)), ("dbeta", (d,)))}
    first, second = _run(c, "fp32"), _run(c, "fp32", init=init)
    for k in ("y", "dx"):
        assert torch.equal(first[k], second[k]), k
    for k in PARAM_GRADS:
        want = init[k].double() + first[k].cpu().double()
        e = assert_close(second[k], want, 1e-6, "accumulated " + k)
        print("PROPEDGE accumulate %s rel err %.2e (max |first| %.3g)" % (k, e, float(first[k].abs().max())))
    rows = PO.untouched_rows(c["prop"], V, c["pad_idx"])
    assert int(rows.sum()) > 100 and torch.equal(second["dtable"].cpu()[rows], init["dtable"][rows])


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_non_zero_pad(cuda, dtype_name):
    """pad_idx = 5: row 5 of the table takes part in the softmax of the half-pad group and gets no gradient, row 0 is an
    ordinary unproposed row, group 2 is all 5."""
    shape = (3, 5, 7, 128)
    c, want = PO.edge_case(shape, dtype_name, pad_idx=5)
    assert c["pad_idx"] == 5 and bool((c["prop"][2] == 5).all()) and float(c["table"][5].abs().max()) > 0
    _check(c, want, dtype_name, SHAPE_ID(shape) + " pad 5")


@pytest.mark.parametrize("pad_idx", [0, 5], ids=["pad0", "pad5"])
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_ids_outside_the_table(cuda, dtype_name, pad_idx):
    """include/imt_hip.h: an id outside [0, vocab) reads row 0 and gets no gradient.  Ids -1, V, V + 7 and 2^40 replace live
    entries of groups 0 and 1 (proposal_oracle.with_out_of_range_ids); the oracle reads a copy of table[0] appended as row V
    and drops that row's gradient (out_of_range_reference).  Row 0 is the pad row under pad_idx 0 and an ordinary row that
    nobody proposes under pad_idx 5: it gets nothing either way.

    Every use of an id in csrc/proposal.hip is guarded, which was read before this ran: stage_tile, the only reader of the
    table (forward and both passes of the rows kernel), replaces an id outside [0, V) by 0 before it forms the address;
    prop_chain_kernel compares ids but forms no address from one, and marks such entries not live (first 0, next -1);
    prop_scatter_kernel reads prop[i] for an address only where first[i] is set, so only for a live id; group_all_pad compares
    with pad_idx only; the group and fold kernels take no ids."""
    shape = (3, 5, 7, 128)
    c, _ = PO.edge_case(shape, dtype_name, pad_idx=pad_idx)
    c = PO.with_out_of_range_ids(c)
    got = _check(c, PO.out_of_range_reference(c), dtype_name, "%s out of range, pad %d" % (SHAPE_ID(shape), pad_idx))
    assert float(got["dtable"][0].abs().max()) == 0.0
