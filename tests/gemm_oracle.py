"""fp64 restatement of imt_gemm as include/imt_hip.h defines it, and the guarded buffers its edge tests launch into
(tests/test_gpu_gemm_edges.py; checked on the CPU by tests/test_gemm_oracle.py).

    v = alpha * alpha_dev * op(A) op(B)          NT: A[M,K] B[N,K]^T   NN: A[M,K] B[K,N]   TN: A[K,M]^T B[K,N]
    v += bias[n]
    IMT_AUX_GELU_FWD: aux[m,n] = v rounded to T ; v = gelu(v)  (exact erf)      IMT_AUX_DGELU: v *= gelu'(aux[m,n])
    dropout: v = keep[m,n] ? v / (1 - p) : 0     (the keep mask is an ARGUMENT: recovered from a kernel, never restated here)
    v += resid[m,n] ; v += C0[m,n] (accumulate)
    TN: a_colsum[m] += alpha * alpha_dev * sum_k A[k,m]

The operands arrive already rounded to the compute type T; everything here is fp64."""
import math

import torch

NT, NN, TN = 0, 1, 2
AUX_NONE, AUX_GELU_FWD, AUX_DGELU = 0, 1, 2
NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}
BF16_ULP = 2.0 ** -7   # an upper bound of ulp(x) / |x| in bf16 (tests/test_gpu_row_edges.py)
ERF_ABS = 1.5e-7       # csrc/common.hpp, erf_and_gauss: |error| of the rational erf
U32 = 2.0 ** -24


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def op_views(layout, A, B):
    """(A as [M,K], B as [K,N]) in fp64."""
    A, B = A.double(), B.double()
    if layout == NT:
        return A, B.t()
    if layout == NN:
        return A, B
    assert layout == TN
    return A.t(), B


def product(layout, A, B):
    """(sum_k a b, sum_k |a||b|) in fp64, [M,N] each: the part of a case that does not depend on the epilogue."""
    a, b = op_views(layout, A, B)
    return a @ b, a.abs() @ b.abs()


def reference(layout, A, B, dtype, *, alpha=1.0, alpha_dev=None, bias=None, aux_mode=AUX_NONE, aux=None, keep=None, dropout_p=0.0,
              resid=None, C0=None, colsum0=None, prod=None):
    """dict(out, mag [, aux] [, colsum], pre): ``out`` the fp64 value of every C element, ``mag`` the magnitude of its terms
    |alpha| sum_k |a||b| + |bias| + |resid| + |C0|, ``pre`` the value after the bias (the GELU argument), ``aux`` what
    IMT_AUX_GELU_FWD stores (``pre`` rounded to ``dtype``), ``colsum`` the TN column sums on top of ``colsum0``.
    ``prod``: product(layout, A, B), when the caller shares it among epilogues."""
    ab, abmag = prod if prod is not None else product(layout, A, B)
    s = float(alpha) * (1.0 if alpha_dev is None else float(alpha_dev))
    v = s * ab
    mag = abs(s) * abmag
    if bias is not None:
        v = v + bias.double()[None, :]
        mag = mag + bias.double().abs()[None, :]
    res = {"pre": v, "accmag": mag}
    if aux_mode == AUX_GELU_FWD:
        res["aux"] = v.to(dtype)
        v = gelu(v)
    elif aux_mode == AUX_DGELU:
        res["z"] = aux.double()
        v = v * gelu_grad(aux.double())
    if dropout_p > 0.0:
        assert keep is not None and keep.dtype == torch.bool and keep.shape == v.shape
        v = torch.where(keep, v / (1.0 - dropout_p), torch.zeros_like(v))
    if resid is not None:
        v = v + resid.double()
        mag = mag + resid.double().abs()
    if C0 is not None:
        v = v + C0.double()
        mag = mag + C0.double().abs()
    res["out"], res["mag"] = v, mag
    if colsum0 is not None:
        assert layout == TN
        res["colsum"] = colsum0.double() + s * A.double().sum(0)
    return res


def bound(res, aux_mode, out_dtype):
    """Element-wise bound of |got - out| for the real-valued (GELU / GELU') epilogues: twice the stated absolute error of the
    rational erf (the 1-ulp rcp / exp2 beside it) times the factor by which erf enters -- 0.5 |z| in z (1 + erf) / 2, and
    0.5 + 0.4 |z| (the erf term and the Gaussian z exp(-z^2 / 2) / sqrt(2 pi) that shares its exponential) times the accumulator
    magnitude in v gelu'(z) -- plus 4 fp32 roundings of the terms' magnitude and one rounding of the output."""
    if aux_mode == AUX_GELU_FWD:
        b = 2.0 * ERF_ABS * 0.5 * res["pre"].abs()
    elif aux_mode == AUX_DGELU:
        b = 2.0 * ERF_ABS * (0.5 + 0.4 * res["z"].abs()) * res["accmag"]
    else:
        b = torch.zeros_like(res["out"])
    b = b + 4.0 * U32 * res["mag"]
    return b + (BF16_ULP if out_dtype == torch.bfloat16 else U32) * res["out"].abs()


# ------------------------------------------------------------------------------------------------ guarded buffers
def _round_up(n, m):
    return (n + m - 1) // m * m


class Guard:
    """A [rows, cols] ``view`` inside a [2 + rows + 2, ld] buffer filled with a NaN bit pattern.  ld defaults to cols rounded up
    to a 16-byte chunk plus 8 (bf16) / 4 (fp32) pad columns, so the view's first column stays 16-byte aligned and the leading
    dimension is wider than the inner extent.  ``check`` asserts that everything outside the view still holds the pattern, bit
    for bit; ``check_all`` (inputs) that the whole buffer is what it was after ``put``."""

    def __init__(self, rows, cols, dtype, dev, ld=None):
        al = 8 if dtype == torch.bfloat16 else 4
        self.rows, self.cols = rows, cols
        self.ld = ld if ld is not None else _round_up(cols, al) + al
        assert self.ld >= cols and self.ld % al == 0
        self.itype, self.pattern = NAN_BITS[dtype]
        self.full = torch.empty(rows + 4, self.ld, dtype=dtype, device=dev)
        self.bits = self.full.view(self.itype)
        self.bits.fill_(self.pattern)
        self.view = self.full[2:2 + rows, :cols]
        self.snapshot = None

    def put(self, t):
        """Copy ``t`` ([rows, cols]) into the view; returns self."""
        assert tuple(t.shape) == (self.rows, self.cols), (tuple(t.shape), self.rows, self.cols)
        self.view.copy_(t.to(self.full.dtype))
        self.snapshot = self.bits.clone()
        return self

    def check(self, what):
        b = self.bits.cpu()
        assert bool((b[:2] == self.pattern).all()), "%s: wrote in front of the first row" % what
        assert bool((b[2 + self.rows:] == self.pattern).all()), "%s: wrote past the last row" % what
        assert bool((b[:, self.cols:] == self.pattern).all()), "%s: wrote into the pad columns" % what

    def check_all(self, what):
        assert torch.equal(self.bits, self.snapshot), "%s: an input came back changed" % what


class GuardVec:
    """A contiguous [n] ``view`` (bias, a_colsum) with 8 guard elements of the NaN pattern on either side."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.itype, self.pattern = NAN_BITS[dtype]
        self.full = torch.empty(n + 16, dtype=dtype, device=dev)
        self.bits = self.full.view(self.itype)
        self.bits.fill_(self.pattern)
        self.view = self.full[8:8 + n]
        self.snapshot = None

    def put(self, t):
        assert tuple(t.shape) == (self.n,)
        self.view.copy_(t.to(self.full.dtype))
        self.snapshot = self.bits.clone()
        return self

    def check(self, what):
        b = self.bits.cpu()
        assert bool((b[:8] == self.pattern).all()) and bool((b[8 + self.n:] == self.pattern).all()), "%s: wrote outside the vector" % what

    def check_all(self, what):
        assert torch.equal(self.bits, self.snapshot), "%s: an input came back changed" % what


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ exact data
def integer_operands(layout, M, N, K, seed):
    """Operands whose every fp32 partial sum is exact: integers in -3..3 plus an asymmetric ramp (a swapped row / column / k
    mapping shows), as tests/test_gpu_ops.py::test_gemm_exact_integer_layout.  Returns fp32 CPU tensors in the layout's shapes."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    B = torch.randint(-3, 4, (N, K), generator=g).float()
    A[:, 0] += torch.arange(M).float() % 5
    B[0, :] += torch.arange(K).float() % 3
    if layout == NT:
        return A, B
    if layout == NN:
        return A, B.t().contiguous()
    return A.t().contiguous(), B.t().contiguous()
