"""The 256 x 128-tile instance of the grouped weight-gradient kernel (imt_gemm_grouped_tn, csrc/gemm.hip grouped_tall_tile)
against the 128 x 128 instance and against fp64.

Both instances give every output element one writer that sums the whole K in ascending 32-element (bf16) / 4-element (fp32)
MFMA steps into fp32, and the bias gradient rides on the same fragments, so dW and db must carry the SAME BITS; that is what
is asserted.  Against fp64 (dy^T x, column sums of dy) the 256 x 128 instance may be off by at most 1.5 times the error of the
128 x 128 instance on the same inputs.

Shapes, the smallest at which the new code can go wrong: token counts 64, 65, 192, 193, 448 = 1, 2 (ragged), 3, 4 (ragged), 7 K
tiles of 64, i.e. 2 .. 14 (bf16) or 4 .. 28 (fp32) K slabs in the six-slab ring, which wraps from six slabs on (bf16 groups
with one K tile, 64 tokens, are not groupable and take imt_gemm per product with either setting); rows 256 and 512, columns
128 and 384; groups of 1, 2 and 11 problems (4 + 7, a pair of layers' worth) with 3, 7 and 28 tiles, so that the XCDs' shares
end inside problems; accumulation onto a non-zero C with and without the fused bias gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = {
    1: [(256, 384)],
    2: [(512, 384), (256, 128)],
    11: [(256, 128), (512, 128), (256, 384), (512, 384), (256, 128), (512, 384), (256, 384), (512, 128), (256, 128), (256, 128), (512, 128)],
}


def _problems(shapes, tokens, dtype, colsum, dev, gen):
    pr = []
    for (m, n) in shapes:
        pr.append(dict(A=torch.randn(tokens, m, generator=gen).to(dtype).to(dev), B=torch.randn(tokens, n, generator=gen).to(dtype).to(dev),
                       out=torch.randn(m, n, generator=gen).to(dev), a_colsum=torch.randn(m, generator=gen).to(dev) if colsum else None))
    return pr


def _copy(pr):
    return [dict(A=p["A"], B=p["B"], out=p["out"].clone(), a_colsum=None if p["a_colsum"] is None else p["a_colsum"].clone()) for p in pr]


def _check(pr0, old, new, what):
    for i, (p0, a, b) in enumerate(zip(pr0, old, new)):
        assert torch.equal(a["out"], b["out"]), "%s: dW of problem %d differs from the 128 x 128 instance by %g" % (
            what, i, float((a["out"] - b["out"]).abs().max()))
        ref = p0["out"].double() + p0["A"].double().t() @ p0["B"].double()
        e_old, e_new = float((a["out"].double() - ref).abs().max()), float((b["out"].double() - ref).abs().max())
        assert e_new <= 1.5 * e_old, (what, i, e_old, e_new)
        if p0["a_colsum"] is not None:
            assert torch.equal(a["a_colsum"], b["a_colsum"]), "%s: db of problem %d differs by %g" % (
                what, i, float((a["a_colsum"] - b["a_colsum"]).abs().max()))
            ref = p0["a_colsum"].double() + p0["A"].double().sum(0)
            e_old, e_new = float((a["a_colsum"].double() - ref).abs().max()), float((b["a_colsum"].double() - ref).abs().max())
            assert e_new <= 1.5 * e_old, (what, i, e_old, e_new)
            scale = float(ref.abs().max())
            assert e_old <= (1e-4 if p0["A"].dtype == torch.float32 else 2e-2) * scale, (what, i, e_old, scale)  # the yardstick itself is sane


@pytest.mark.parametrize("tokens", [64, 65, 192, 193, 448])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_tall_tiles_carry_the_bits_of_square_tiles(cuda, dtype, tokens):
    from imagetranslate_amd import hip_ops as O
    gen = torch.Generator().manual_seed(1000 + tokens)
    torch.full((1 << 22,), 7.0, device=cuda)  # poison recycled allocator blocks: a read past an operand would not see zeros
    for count, shapes in GROUPS.items():
        for colsum in (True, False):
            pr0 = _problems(shapes, tokens, dtype, colsum, cuda, gen)
            old, new = _copy(pr0), _copy(pr0)
            O.gemm_grouped_tn(old, tile_rows=128)
            O.gemm_grouped_tn(new, tile_rows=256)
            _check(pr0, old, new, "%d problems, %d tokens, %s, colsum=%s" % (count, tokens, dtype, colsum))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rows_not_a_multiple_of_256_keep_square_tiles(cuda, dtype):
    """A row count of 384 in the group: the policy refuses 256 x 128 tiles whatever is asked for, and the bits are those of
    the 128 x 128 instance; the same for what the policy picks itself for so few tiles."""
    from imagetranslate_amd import hip_ops as O
    gen = torch.Generator().manual_seed(77)
    pr0 = _problems([(512, 128), (384, 384), (256, 128)], 193, dtype, True, cuda, gen)
    old, asked, auto = _copy(pr0), _copy(pr0), _copy(pr0)
    O.gemm_grouped_tn(old, tile_rows=128)
    O.gemm_grouped_tn(asked, tile_rows=256)
    O.gemm_grouped_tn(auto)
    _check(pr0, old, asked, "row count 384, 256-row tiles asked for")
    _check(pr0, old, auto, "row count 384, policy")
    pr1 = _problems(GROUPS[2], 193, dtype, True, cuda, gen)  # 7 tall tiles: far below three quarters of a tile per CU
    old, auto = _copy(pr1), _copy(pr1)
    O.gemm_grouped_tn(old, tile_rows=128)
    O.gemm_grouped_tn(auto)
    _check(pr1, old, auto, "7 tiles, policy")
