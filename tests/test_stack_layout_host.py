"""Workspace sizes of the stack runtime (csrc/model.hip: carve, carve_decode), pinned as literal numbers, WITHOUT a GPU.

imt_stack_workspace_bytes / imt_decode_workspace_bytes return the end of the last carved buffer, so a buffer that is added,
dropped, resized or moved in front of another changes them.  The numbers were recorded by running this table against a library
built from the commit before the runtime's scratch pointers lost their mirrored copies; the forward and the backward carve the
workspace with the same function, so equal sizes here mean every saved activation is still where the other pass looks for it.

Cases: an encoder and a decoder whose cross key|value weights are contiguous in layer order (one batched projection: kv_all and
d_kv_all), 0 / 1 / 2 / 6 layers, fp32 and bf16; a decoder with cross_kv_* = -1 and one whose layer 1 has no cross block (both
unbatched); 16 tokens (ceil(N/128) * ceil(d/128) <= 128: the split-K slabs are carved) and 5120 tokens at d = 512 (160 tiles: no
slabs); the decode workspace at d = 512 in bf16 (hand-off buffers of the one-launch step) and in fp32 (none)."""
import ctypes

import pytest

from imagetranslate_amd import _lib as L

F32, BF16 = L.IMT_F32, L.IMT_BF16


def _desc(n_layers, d, heads, ff, decoder, dtype, cross_kv="contiguous", no_cross=()):
    """A stack descriptor over a flat store laid out by a bump allocator (offsets in elements, nothing is dereferenced)."""
    arr = (L.LayerDesc * max(1, n_layers))()
    off = [4096]

    def take(n):
        off[0] += n
        return off[0] - n

    kv_w0, kv_b0 = take(n_layers * 2 * d * d), take(n_layers * 2 * d)
    for i in range(n_layers):
        for blk in (arr[i].self_attn, arr[i].cross_attn):
            blk.qkv_w, blk.qkv_b, blk.o_w, blk.o_b, blk.ln_g, blk.ln_b = take(3 * d * d), take(3 * d), take(d * d), take(d), take(d), take(d)
        if not decoder or i in no_cross:
            arr[i].cross_attn.qkv_w = -1
        arr[i].ff1_w, arr[i].ff1_b, arr[i].ff2_w, arr[i].ff2_b = take(d * ff), take(ff), take(d * ff), take(d)
        arr[i].ln2_g, arr[i].ln2_b = take(d), take(d)
        contiguous = decoder and cross_kv == "contiguous"
        arr[i].cross_kv_w = kv_w0 + i * 2 * d * d if contiguous else -1
        arr[i].cross_kv_b = kv_b0 + i * 2 * d if contiguous else -1
    s = L.StackDesc()
    s.dtype, s.d, s.heads, s.ff, s.vocab, s.max_pos, s.n_types, s.n_layers = dtype, d, heads, ff, 1000, 128, 2, n_layers
    s.is_decoder, s.pad_id, s.ln_eps = int(decoder), 0, 1e-12
    s.emb_word, s.emb_pos, s.emb_type, s.emb_ln_g, s.emb_ln_b = 0, 1024, 2048, 3072, 3584
    s.layers = ctypes.cast(arr, ctypes.POINTER(L.LayerDesc))
    s.params = 0x1000
    s._keep = arr
    return s


SMALL = dict(d=128, heads=4, ff=512)      # B x T = 2 x 8 (Tk 12): one output tile, the split-K slabs are carved
WIDE = dict(d=512, heads=8, ff=2048)      # B x T = 64 x 80 (Tk 40): 40 x 4 = 160 tiles, no slabs

# (kind, n_layers, dtype, size) -> bytes
STACK = {
    ("enc", 0, F32, "small"): 17343232, ("enc", 0, BF16, "small"): 17079040,
    ("enc", 1, F32, "small"): 17573888, ("enc", 1, BF16, "small"): 17244160,
    ("enc", 2, F32, "small"): 17804544, ("enc", 2, BF16, "small"): 17409280,
    ("enc", 6, F32, "small"): 18727168, ("enc", 6, BF16, "small"): 18069760,
    ("dec", 0, F32, "small"): 17437440, ("dec", 0, BF16, "small"): 17126144,
    ("dec", 1, F32, "small"): 17726208, ("dec", 1, BF16, "small"): 17320704,
    ("dec", 2, F32, "small"): 18064128, ("dec", 2, BF16, "small"): 17539840,
    ("dec", 6, F32, "small"): 19317504, ("dec", 6, BF16, "small"): 18367232,
    ("dec_kv_absent", 2, BF16, "small"): 17515264, ("dec_kv_absent", 6, F32, "small"): 19170048,
    ("dec_layer1_no_cross", 2, BF16, "small"): 17485824, ("dec_layer1_no_cross", 6, F32, "small"): 19111936,
    ("enc", 2, F32, "wide"): 1008263168, ("enc", 6, BF16, "wide"): 843038720,
    ("dec", 2, F32, "wide"): 1176428544, ("dec", 6, BF16, "wide"): 1053974528,
    ("dec_kv_absent", 6, BF16, "wide"): 1022517248,
}

# (d, n_layers, dtype, r_max) -> bytes
DECODE = {
    (512, 2, BF16, 320): 32187392, (512, 6, BF16, 320): 53158912, (512, 2, F32, 320): 26614272, (512, 6, F32, 320): 26614272,
    (128, 2, BF16, 8): 16812544, (128, 2, F32, 8): 16843264,
}


def stack_bytes(lib, kind, n_layers, dtype, size):
    shape, (B, T, Tk) = (SMALL, (2, 8, 12)) if size == "small" else (WIDE, (64, 80, 40))
    kw = {"enc": dict(decoder=False), "dec": dict(decoder=True), "dec_kv_absent": dict(decoder=True, cross_kv="absent"),
          "dec_layer1_no_cross": dict(decoder=True, no_cross=(1,))}[kind]
    return lib.imt_stack_workspace_bytes(ctypes.byref(_desc(n_layers, dtype=dtype, **shape, **kw)), B, T, Tk)


def decode_bytes(lib, d, n_layers, dtype, r_max):
    return lib.imt_decode_workspace_bytes(ctypes.byref(_desc(n_layers, d, d // 64, 4 * d, True, dtype)), r_max)


@pytest.mark.parametrize("case", sorted(STACK), ids=lambda c: "%s-%d-%s-%s" % (c[0], c[1], "bf16" if c[2] == BF16 else "fp32", c[3]))
def test_stack_workspace_bytes(case):
    assert stack_bytes(L.load(), *case) == STACK[case]


@pytest.mark.parametrize("case", sorted(DECODE), ids=lambda c: "d%d-%d-%s-r%d" % (c[0], c[1], "bf16" if c[2] == BF16 else "fp32", c[3]))
def test_decode_workspace_bytes(case):
    assert decode_bytes(L.load(), *case) == DECODE[case]


def test_the_table_covers_what_it_says():
    """The cases really differ where the list above says so: batched key|value buffers, split-K slabs, hand-off buffers."""
    slabs = L.load().imt_gemm_splitk_ws_bytes()
    # batched: kv_all and d_kv_all [Nk, n * 2d] instead of n buffers [Nk, 2d] -> n * Nk * 2d elements more (Nk = 2 * 12, d = 128)
    assert STACK[("dec", 2, BF16, "small")] - STACK[("dec_kv_absent", 2, BF16, "small")] == 2 * 24 * 256 * 2
    assert STACK[("dec", 6, F32, "small")] - STACK[("dec_kv_absent", 6, F32, "small")] == 6 * 24 * 256 * 4
    # 16 tokens: the slabs are most of the workspace; 5120 tokens: the activations alone (the slabs are 16 MiB)
    assert slabs < STACK[("enc", 0, BF16, "small")] < slabs + (1 << 20)
    assert DECODE[(512, 6, F32, 320)] == DECODE[(512, 2, F32, 320)]                     # the chain: nothing per layer
    assert DECODE[(512, 6, BF16, 320)] - DECODE[(512, 2, BF16, 320)] == 4 * 320 * (6 * 512 * 2 + 2048 * 2 + 3 * 512 * 4)
