"""imt_stack_backward over a whole stack, with the weight gradients of two layers per grouped launch on 256 x 128 tiles
(csrc/model.hip: DeferredDW::hold_for_pair says which layers may pair, DwPlan where each launch goes), against the per-layer
segment calls (layer_lo, layer_hi) of a data-parallel run, which keep one launch of 128 x 128 tiles per layer.

A 2-layer encoder (one pair) and a 3-layer decoder with cross-attention (one pair and an odd layer), d = 256, ff = 512 -- every
row count (256, 512, 768) a multiple of 256 -- on 192 tokens (3 K tiles) and 193 (a ragged fourth), bf16.  So few tiles never
reach the policy's three quarters of a tile per CU: the test lowers that bar for the whole-stack run
(imt_set_gemm_grouped_tall_min_tiles), the segment run keeps the default.

A 6-layer encoder and a 5-layer decoder (unequal depths: the decoder does not share the encoder's attention) on 2 x 64 tokens run
past the four scratch sets of the backward: layers 1 and 0 wait for the side-stream launches that read the sets of layers 5 and 4
before they overwrite them, and the decoder ends on an odd layer.

The two instances of the kernel carry the same bits (tests/test_gpu_grouped_dw_tiles.py), and everything upstream of a weight
gradient is the same launches in the same order, so every weight and bias gradient of the layers must be EQUAL bit for bit.
LayerNorm and embedding gradients are summed with float atomics in both runs and are compared to 1e-3 of their largest
magnitude."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _grads(m, args, segments):
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd.param_store import store_of
    store = store_of(m)
    m.zero_grad()
    if segments:
        store.segment_hook = lambda mod, l: None
    try:
        with O.grouped_tall_min_tiles(0 if segments else 1):
            loss, _ = m.loss_fused(*args)
            loss.backward()
            torch.cuda.synchronize()
    finally:
        if segments:
            del store.segment_hook
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _check(batch, length, enc_layer, dec_layer):
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    g = torch.Generator().manual_seed(3)
    src = torch.randint(6, 1000, (batch, length), generator=g)
    tgt = torch.randint(6, 1000, (batch, length), generator=g)
    args = (src, tgt, src != 0, tgt != 0, torch.zeros(batch, dtype=torch.long), torch.ones(batch, dtype=torch.long))
    torch.manual_seed(0)
    m = Seq2Seq(SyntheticTextProcessor(1000), lang_dec=False, enc_layer=enc_layer, dec_layer=dec_layer, embed_dim=256, intermediate_dim=512,
                num_attention_heads=4).cuda().eval()
    m.set_compute_dtype(torch.bfloat16)
    loss_seg, seg = _grads(m, args, segments=True)
    loss_all, whole = _grads(m, args, segments=False)
    assert loss_seg == loss_all
    assert seg.keys() == whole.keys()
    exact = [n for n in seg if (".encoder.layer." in n or ".decoder.layer." in n) and "LayerNorm" not in n]
    assert len(exact) == enc_layer * 12 + dec_layer * 20, sorted(seg)  # 6 (encoder) / 10 (decoder) linear maps per layer, weight and bias
    for n in sorted(seg):
        a, b = seg[n], whole[n]
        if n in exact:
            assert float(a.abs().max()) > 0, n
            assert torch.equal(a, b), "%s: differs from the segment calls by %g (largest %g)" % (n, float((a - b).abs().max()), float(a.abs().max()))
        else:
            assert float((a - b).abs().max()) <= 1e-3 * float(a.abs().max()), n


@pytest.mark.parametrize("batch,length", [(3, 64), (1, 193)])
def test_layer_pairs_give_the_gradients_of_per_layer_segments(cuda, batch, length):
    _check(batch, length, enc_layer=2, dec_layer=3)


def test_stacks_deeper_than_the_scratch_sets_give_the_gradients_of_per_layer_segments(cuda):
    _check(2, 64, enc_layer=6, dec_layer=5)
