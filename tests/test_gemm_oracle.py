"""tests/gemm_oracle.py against torch (F.gelu, autograd for GELU', fp64 matmul) and against one hand-written 2 x 3 x 2 case
per layout; the guarded buffers against stray writes of every kind.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_oracle as GO

F64 = torch.float64


def test_gelu_and_gradient_against_torch():
    z = torch.linspace(-9.0, 9.0, 3601, dtype=F64, requires_grad=True)
    y = F.gelu(z)
    (g,) = torch.autograd.grad(y.sum(), z)
    assert float((GO.gelu(z.detach()) - y.detach()).abs().max()) < 1e-15
    assert float((GO.gelu_grad(z.detach()) - g).abs().max()) < 1e-15


# A (as [M,K]) = [[1, 2], [3, 4]], B (as [K,N]) = [[1, 0, -1], [2, 1, 0]]:  A B = [[5, 2, -1], [11, 4, -3]]
A_MK = [[1.0, 2.0], [3.0, 4.0]]
B_KN = [[1.0, 0.0, -1.0], [2.0, 1.0, 0.0]]
AB = [[5.0, 2.0, -1.0], [11.0, 4.0, -3.0]]
ABMAG = [[5.0, 2.0, 1.0], [11.0, 4.0, 3.0]]


def _hand(layout):
    a, b = torch.tensor(A_MK), torch.tensor(B_KN)
    if layout == GO.NT:
        return a, b.t().contiguous()
    if layout == GO.NN:
        return a, b
    return a.t().contiguous(), b


@pytest.mark.parametrize("layout", [GO.NT, GO.NN, GO.TN])
def test_hand_written_case(layout):
    A, B = _hand(layout)
    ab, mag = GO.product(layout, A, B)
    assert torch.equal(ab, torch.tensor(AB, dtype=F64)) and torch.equal(mag, torch.tensor(ABMAG, dtype=F64))
    bias = torch.tensor([1.0, -2.0, 0.5])
    resid = torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])
    C0 = torch.tensor([[10.0, 20.0, 30.0], [40.0, 50.0, 60.0]])
    keep = torch.tensor([[True, False, True], [False, True, True]])
    r = GO.reference(layout, A, B, torch.float32, alpha=0.5, alpha_dev=2.0 ** -1, bias=bias, keep=keep, dropout_p=0.5, resid=resid, C0=C0,
                     colsum0=torch.tensor([100.0, 200.0]) if layout == GO.TN else None)
    # v = AB / 4 + bias = [[2.25, -1.5, 0.25], [3.75, -1, -0.25]]; kept ones doubled; + resid + C0
    want = [[2 * 2.25 + 1 + 10, 0 + 1 + 20, 2 * 0.25 + 1 + 30], [0 - 1 + 40, 2 * -1.0 - 1 + 50, 2 * -0.25 - 1 + 60]]
    assert torch.equal(r["out"], torch.tensor(want, dtype=F64))
    wmag = [[5 / 4 + 1 + 1 + 10, 2 / 4 + 2 + 1 + 20, 1 / 4 + 0.5 + 1 + 30], [11 / 4 + 1 + 1 + 40, 4 / 4 + 2 + 1 + 50, 3 / 4 + 0.5 + 1 + 60]]
    assert torch.equal(r["mag"], torch.tensor(wmag, dtype=F64))
    if layout == GO.TN:  # column sums of A[K,M]: sum_k A[k,m] = [1 + 2, 3 + 4], times alpha * alpha_dev = 1/4
        assert torch.equal(r["colsum"], torch.tensor([100.75, 201.75], dtype=F64))


@pytest.mark.parametrize("layout", [GO.NT, GO.NN, GO.TN])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_against_torch(layout, dtype):
    M, N, K = 7, 10, 9
    g = torch.Generator().manual_seed(3)
    A, B = GO.integer_operands(layout, M, N, K, 4)
    A, B = A.to(dtype), B.to(dtype)
    a, b = (A.double(), B.double().t()) if layout == GO.NT else (A.double(), B.double()) if layout == GO.NN else (A.double().t(), B.double())
    bias = torch.randint(-4, 5, (N,), generator=g).to(dtype)
    z0 = 0.125 * (a @ b) + bias.double()
    # GELU forward: aux is the rounded pre-activation, out = F.gelu of the UNROUNDED one
    r = GO.reference(layout, A, B, dtype, alpha=0.125, bias=bias, aux_mode=GO.AUX_GELU_FWD)
    assert torch.equal(r["aux"], z0.to(dtype)) and r["aux"].dtype == dtype
    assert float((r["out"] - F.gelu(z0)).abs().max()) < 1e-13
    assert torch.equal(r["pre"], z0)
    # GELU': autograd of F.gelu at aux, times the upstream value
    aux = (torch.randn(M, N, generator=g) * 1.5).to(dtype)
    zz = aux.double().requires_grad_(True)
    (gz,) = torch.autograd.grad(F.gelu(zz).sum(), zz)
    resid = torch.randint(-3, 4, (M, N), generator=g).to(dtype)
    r = GO.reference(layout, A, B, dtype, alpha=0.125, bias=bias, aux_mode=GO.AUX_DGELU, aux=aux, resid=resid)
    assert float((r["out"] - (z0 * gz + resid.double())).abs().max()) < 1e-12
    want_mag = 0.125 * (a.abs() @ b.abs()) + bias.double().abs() + resid.double().abs()
    assert torch.equal(r["mag"], want_mag) and torch.equal(r["accmag"], 0.125 * (a.abs() @ b.abs()) + bias.double().abs())
    # the bound is positive everywhere and grows with the output rounding of bf16
    assert bool((GO.bound(r, GO.AUX_DGELU, dtype) > 0).all())
    assert bool((GO.bound(r, GO.AUX_DGELU, torch.bfloat16) >= GO.bound(r, GO.AUX_DGELU, torch.float32)).all())


def test_integer_operands_are_exact_in_bf16():
    for layout in (GO.NT, GO.NN, GO.TN):
        A, B = GO.integer_operands(layout, 300, 392, 193, 1)
        assert torch.equal(A.to(torch.bfloat16).float(), A) and torch.equal(B.to(torch.bfloat16).float(), B)
        ab, mag = GO.product(layout, A, B)
        assert tuple(ab.shape) == (300, 392) and float(mag.max()) < 2 ** 24  # every fp32 partial sum is an exact integer
    a_nt, b_nt = GO.integer_operands(GO.NT, 5, 6, 8, 1)
    a_tn, b_tn = GO.integer_operands(GO.TN, 5, 6, 8, 1)
    assert torch.equal(a_nt.t(), a_tn) and torch.equal(b_nt.t(), b_tn)   # one product in every layout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guard_sees_every_stray_write(dtype):
    dev = torch.device("cpu")
    al = 8 if dtype == torch.bfloat16 else 4
    g = GO.Guard(5, 13, dtype, dev)
    assert g.ld == 16 + al and g.view.data_ptr() % 16 == 0 and g.view.stride(0) == g.ld and g.ld > 13
    g.put(torch.ones(5, 13))
    g.check("clean")
    g.check_all("clean")
    for (r, c, msg) in [(1, 0, "in front"), (7, 3, "past the last"), (3, 13, "pad"), (2, g.ld - 1, "pad")]:
        h = GO.Guard(5, 13, dtype, dev).put(torch.ones(5, 13))
        h.full[r, c] = 1.0
        with pytest.raises(AssertionError, match=msg):
            h.check("x")
        with pytest.raises(AssertionError, match="changed"):
            h.check_all("x")
    h = GO.Guard(5, 13, dtype, dev).put(torch.ones(5, 13))
    h.view[4, 12] = 2.0
    h.check("x")   # inside the view: not the guard's business ...
    with pytest.raises(AssertionError, match="changed"):
        h.check_all("x")   # ... but an input must come back whole
    # a NaN written over the NaN pattern with other bits is a write too
    h = GO.Guard(5, 13, dtype, dev)
    h.full[0, 0] = float("nan")
    assert int(h.bits[0, 0]) != h.pattern
    with pytest.raises(AssertionError):
        h.check("x")
    assert GO.Guard(300, 390, dtype, dev, ld=392).view.stride(0) == 392
    v = GO.GuardVec(10, dtype, dev).put(torch.arange(10.0))
    assert v.view.data_ptr() % 16 == 0
    v.check("v")
    v.full[7] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        v.check("v")
    v = GO.GuardVec(10, dtype, dev)
    v.full[18] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        v.check("v")


def test_bits_equal_tells_zero_signs_apart():
    a = torch.tensor([0.0, 1.0])
    assert GO.bits_equal(a, a.clone()) and not GO.bits_equal(a, torch.tensor([-0.0, 1.0]))
    assert not GO.bits_equal(a, a.double())


def test_bound_terms():
    """The bound is the stated sum: erf term + 4 fp32 roundings of the magnitude + one output rounding."""
    r = {"pre": torch.tensor([[4.0]], dtype=F64), "accmag": torch.tensor([[6.0]], dtype=F64), "mag": torch.tensor([[8.0]], dtype=F64),
         "out": torch.tensor([[2.0]], dtype=F64), "z": torch.tensor([[-3.0]], dtype=F64)}
    assert math.isclose(float(GO.bound(r, GO.AUX_GELU_FWD, torch.float32)), 3e-7 * 0.5 * 4 + 4 * 2.0 ** -24 * 8 + 2.0 ** -24 * 2, rel_tol=1e-12)
    assert math.isclose(float(GO.bound(r, GO.AUX_DGELU, torch.bfloat16)), 3e-7 * (0.5 + 1.2) * 6 + 4 * 2.0 ** -24 * 8 + 2.0 ** -7 * 2, rel_tol=1e-12)
