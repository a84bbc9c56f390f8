"""The launches of the stack runtime (csrc/model.hip), by kernel kind and count (imt_prof_report), against dictionaries recorded
with this test body from the commit before the runtime was reshaped (operands by name, one scratch copy, the weight-gradient
schedule as an object): the same kernels, on the same shapes, the same number of times.

  * one loss_fused + backward of the 2-encoder / 3-decoder model of tests/test_gpu_stack_dw_pairs.py (d = 256, ff = 512, 4 heads,
    bf16, 3 x 64 tokens): embeddings, batched cross key|value projection, every block forward and backward, the LayerNorm fold;
  * a beam search of three steps on the same model in fp32, which never takes the one-launch step: imt_decode_begin and three
    times the per-operator chain of imt_decode_step.

With the profiler on, the side stream and the layer pairs are off by design (one grouped launch per layer on the main stream):
this test pins the arithmetic chain; tests/test_stack_dw_schedule_host.py and tests/test_gpu_stack_dw_pairs.py pin the schedule.
Each case prints ``STACKLAUNCHES <case> <dictionary>`` before it asserts (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TRAIN = {'attn_bwd_fused_bf16': 8, 'attn_fwd_bf16': 8, 'embed_bwd': 2, 'embed_ln_fwd': 2, 'gemm_bf16_tn_grouped': 5, 'gemm_ln_bf16': 13,
         'gemm_sbuf_bf16_nn': 1, 'gemm_splitk_epilogue': 1, 'gemm_ws_bf16_nn': 19, 'gemm_ws_bf16_nt': 15, 'gemm_ws_bf16_tn': 1,
         'layernorm_bwd': 15, 'ln_partial_reduce': 2, 'xent_fused': 1}

DECODE = {'attn_decode': 18, 'attn_fwd_f32': 2, 'beam_merge': 3, 'beam_row_topk': 3, 'embed_ln_fwd': 4, 'gemm_ln_f32': 31,
          'gemm_ws_f32_nt': 37}


def _kinds_of(fn):
    """Kernel kinds (imt_prof_report rows) launched by fn(), as {kind: launches}."""
    from imagetranslate_amd import _lib as L
    lib = L.load()
    torch.cuda.synchronize()
    lib.imt_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        rows = (L.ProfRow * 256)()
        n = lib.imt_prof_report(rows, 256)
    finally:
        lib.imt_prof_enable(0)
    assert n < 256
    return {rows[i].kind.decode(): int(rows[i].launches) for i in range(n)}


@pytest.fixture(scope="module")
def model(cuda):
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    torch.manual_seed(0)
    return Seq2Seq(SyntheticTextProcessor(1000), lang_dec=False, enc_layer=2, dec_layer=3, embed_dim=256, intermediate_dim=512,
                   num_attention_heads=4).cuda().eval()


def _batch(batch, length):
    g = torch.Generator().manual_seed(3)
    src = torch.randint(6, 1000, (batch, length), generator=g)
    tgt = torch.randint(6, 1000, (batch, length), generator=g)
    return src, tgt


def test_train_step_launches(model):
    src, tgt = _batch(3, 64)
    args = (src, tgt, src != 0, tgt != 0, torch.zeros(3, dtype=torch.long), torch.ones(3, dtype=torch.long))
    model.set_compute_dtype(torch.bfloat16)
    model.zero_grad()

    def step():
        loss, _ = model.loss_fused(*args)
        loss.backward()

    step()  # buffers, streams and workspaces exist before the launches are counted
    model.zero_grad()
    got = _kinds_of(step)
    print("STACKLAUNCHES train", dict(sorted(got.items())))
    assert got == TRAIN


def test_decode_chain_launches(model):
    from imagetranslate_amd.seq_gen import BeamDecoder
    src, _ = _batch(3, 24)
    model.set_compute_dtype(torch.float32)
    kw = dict(src_inputs=src, src_sizes=(src != 0).sum(1), first_tokens=torch.full((3,), 6), src_mask=src != 0,
              src_langs=torch.zeros(3, dtype=torch.long), tgt_langs=torch.ones(3, dtype=torch.long), pad_idx=0, max_len=4)
    search = BeamDecoder(model, beam_width=3)
    search(**kw)
    got = _kinds_of(lambda: search(**kw))
    print("STACKLAUNCHES decode", dict(sorted(got.items())))
    assert got == DECODE
