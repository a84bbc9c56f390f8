"""ImageCaptioning's object stream on the GPU: the object head and gated-mix kernels against torch, whole-model parity with
the plain-torch restatement (tests/object_stream_oracle.py), beam search with objects, and the CLIs."""
import os

import pytest
import torch

from oracle import reference_model as R
from tests.object_stream_oracle import ObjImageCaptioning, beam_search, object_rows
from tests.util import assert_close, beam_state_dict

pytestmark = pytest.mark.gpu


def _objects(B, N, counts=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    labels = torch.zeros(B, N, dtype=torch.long)
    counts = counts if counts is not None else torch.randint(0, N + 1, (B,), generator=g).tolist()
    for b, c in enumerate(counts):
        labels[b, :c] = torch.randint(1, 91, (c,), generator=g)
    xy = torch.rand(B, N, 2, generator=g) * 600
    wh = torch.rand(B, N, 2, generator=g) * 200
    return {"feats": torch.randn(B, N, 1024, generator=g), "boxes": torch.cat([xy, xy + wh], -1), "labels": labels}


def _head(d, p=0.0):
    from imagetranslate_amd.image_model import ImageHead
    torch.manual_seed(d)
    head = ImageHead(64, d, dropout=p)
    head.add_object_head(d)
    return head.cuda()


def _keep_mask(seed, n, p):
    """Restatement of csrc/common.hpp dropout_keep (lowbias32 finaliser, two 16-bit draws per word, four per block)."""
    M = 0xFFFFFFFF

    def mix32(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & M
        x ^= x >> 15
        x = (x * 0x846ca68b) & M
        return x ^ (x >> 16)
    thresh = max(1, min(65535, int(p * 65536.0 + 0.5)))
    key = (seed & M) ^ (((seed >> 32) * 0x9e3779b9) & M)
    idx = torch.arange(n, dtype=torch.int64)
    idx4 = idx >> 2
    lo = mix32((((idx4 & M) ^ key) + (((idx4 >> 32) * 0x85ebca6b) & M)) & M)
    hi = mix32((lo + 0x9e3779b9) & M)
    e = idx & 3
    w = torch.where((e & 2) != 0, hi, lo)
    draw = torch.where((e & 1) != 0, w >> 16, w & 0xFFFF)
    return draw >= thresh


# ------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_object_head_forward_backward(cuda, d, dtype):
    head = _head(d)
    objs = _objects(3, 37, counts=[37, 5, 0], seed=d)
    out = head.objects_forward(objs, dtype)
    dy = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(out.device)
    out.backward(dy.to(out.dtype))
    W = head.object_feat_fc.weight.detach().cpu().double().requires_grad_()
    E = head.object_embedding.weight.detach().cpu().double().requires_grad_()
    z = object_rows(E, objs["labels"], objs["feats"].double(), objs["boxes"].double()) @ W.t()
    ref = torch.relu(z)
    tol = 1e-5 if dtype == torch.float32 else 2.5e-2
    assert_close(out.float(), ref, tol, "object_fc")
    if dtype == torch.bfloat16:
        # bf16 rounding flips the sign of pre-activations near 0, and each flip moves an O(1) term in or out of dW:
        # the backward is checked against the forward's own ReLU mask
        ref = z * (out.detach().cpu() > 0)
    (ref * dy.to(dtype).double().cpu()).sum().backward()
    assert_close(head.object_feat_fc.weight.grad, W.grad, tol, "d object_feat_fc")
    assert_close(head.object_embedding.weight.grad, E.grad, tol, "d object_embedding")
    assert float(head.object_embedding.weight.grad[0].abs().max()) == 0.0  # label 0: zeroed rows get nothing
    assert float(head.object_feat_fc.weight.grad.abs().max()) > 0


def test_object_head_dropout_mask_regenerated(cuda):
    d, p = 128, 0.25
    head = _head(d, p).train()
    head._imt_dropout_seed = 7
    objs = _objects(2, 29, counts=[29, 11], seed=3)
    out = head.objects_forward(objs, torch.float32)
    dy = torch.randn(out.shape, device=out.device)
    out.backward(dy)
    W = head.object_feat_fc.weight.detach().cpu().double().requires_grad_()
    E = head.object_embedding.weight.detach().cpu().double()
    z = object_rows(E, objs["labels"], objs["feats"].double(), objs["boxes"].double()) @ W.t()
    keep = (out.detach().cpu() != 0)
    active = z > 0
    drop_rate = 1.0 - float((keep & active).sum()) / float(active.sum())
    assert abs(drop_rate - p) < 0.03, drop_rate
    # the mask is the shared counter-based one: keep(seed, r * d + c) of csrc/common.hpp, here with seed 7 + 2
    want = _keep_mask(9, out.numel(), p).view(out.shape)
    clear = z.abs() > 1e-3 * float(z.detach().abs().max())            # no sign decided by rounding
    assert torch.equal(keep[active & clear], want[active & clear])
    assert_close(out.cpu(), torch.relu(z) * keep / (1 - p), 1e-5, "dropout(relu(z)) with the kernel's mask")
    ((torch.relu(z) * keep / (1 - p)) * dy.cpu().double()).sum().backward()
    assert_close(head.object_feat_fc.weight.grad, W.grad, 1e-5, "d object_feat_fc under dropout (mask from the seed)")
    head.object_feat_fc.weight.grad.zero_()
    out2 = head.objects_forward(objs, torch.float32)
    assert torch.equal(out2, out), "same seed, same mask"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gated_mix_backward_against_autograd(cuda, dtype):
    from imagetranslate_amd import hip_ops as O
    g = torch.Generator().manual_seed(4)
    rows, d = 301, 512
    a, b, dy = (torch.randn(rows, d, generator=g) for _ in range(3))
    gate = torch.randn(d, generator=g) * 0.5
    dgate = torch.zeros(d, device="cuda")
    da, db = O.gated_mix_bwd(dy.to("cuda", dtype), a.to("cuda", dtype), b.to("cuda", dtype), gate.to("cuda", dtype), dgate)
    ad, bd, gd = (t.to(dtype).double().requires_grad_() for t in (a, b, gate))
    s = torch.sigmoid(gd + 1e-7)
    ((s * ad + (1 - s) * bd) * dy.to(dtype).double()).sum().backward()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert_close(da.float(), ad.grad, tol, "da")
    assert_close(db.float(), bd.grad, tol, "db")
    assert_close(dgate, gd.grad, 1e-5 if dtype == torch.float32 else 1e-2, "dgate")


def test_gradients_are_bit_identical_across_runs(cuda):
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd.param_store import store_of
    head = _head(512)
    objs = _objects(8, 100, seed=11)
    grads = []
    for _ in range(2):
        store_of(head).zero_grad()
        out = head.objects_forward(objs, torch.bfloat16)
        out.backward(torch.ones_like(out))
        grads.append(head.object_embedding.weight.grad.clone())
    assert torch.equal(grads[0], grads[1])
    g = torch.Generator().manual_seed(2)
    a, b, dy = (torch.randn(3200, 512, generator=g).cuda() for _ in range(3))
    gate = torch.randn(512, generator=g).cuda()
    outs = []
    for _ in range(2):
        dg = torch.zeros(512, device="cuda")
        O.gated_mix_bwd(dy, a, b, gate, dg)
        outs.append(dg)
    assert torch.equal(outs[0], outs[1])


def test_out_of_range_device_label_is_reported(cuda):
    """A device-resident label outside [0, 91): its row is zeroed on the device and the status word turns into an error
    (at once with wait=True, otherwise at a later call once the read-back has landed)."""
    head = _head(128).eval()
    objs = _objects(2, 9, counts=[9, 4], seed=5)
    good = head.objects_forward({k: v.cuda() for k, v in objs.items()}, torch.float32)
    head.check_object_labels(wait=True)                       # nothing to report
    bad = {k: v.clone().cuda() for k, v in objs.items()}
    bad["labels"][0, 3] = 95
    with torch.no_grad():
        out = head.objects_forward(bad, torch.float32)
    with pytest.raises(ValueError):
        head.check_object_labels(wait=True)
    assert float(out[0, 3].abs().max()) == 0.0 and torch.equal(out[1], good[1].detach())
    head.check_object_labels(wait=True)                       # reported once, word cleared


# ------------------------------------------------------------------------------------------------ model parity
def _pair(lang_dec=False, d=128, enc=2, dec=2, seed=0, V=1000, **kw):
    from imagetranslate_amd.image_model import ImageCaptioning
    torch.manual_seed(seed)
    tp = R.SyntheticTextProcessor(V)
    args = dict(lang_dec=lang_dec, enc_layer=enc, dec_layer=dec, embed_dim=d, intermediate_dim=4 * d, num_attention_heads=4,
                image_feat_dim=64, **kw)
    ref = ObjImageCaptioning(tp, **args).eval()
    with torch.no_grad():
        ref.multistream_attention_gate.normal_(0.0, 1.0)  # a gate away from its 0.1 fill: both streams matter per column
    ours = ImageCaptioning(tp, use_obj=True, **args)
    res = ours.load_state_dict(ref.state_dict(), strict=False)
    assert not res.unexpected_keys and all("layer_norm" in k for k in res.missing_keys), res
    return ref, ours.cuda().eval()


def _caption_batch(B=5, T=13, N=23, seed=6, counts=None):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randint(6, 1000, (B, T), generator=g)
    lt = torch.randint(T // 2, T + 1, (B,), generator=g)
    tgt[torch.arange(T)[None] >= lt[:, None]] = 0
    return dict(images=torch.randn(B, 49, 64, generator=g), objects=_objects(B, N, counts=counts, seed=seed), tgt=tgt,
                langs=torch.ones(B, dtype=torch.long))


@pytest.mark.parametrize("lang_dec", [False, True])
def test_model_parity_fp32(cuda, lang_dec):
    ref, ours = _pair(lang_dec)
    b = _caption_batch(counts=[23, 4, 0, 17, 9])
    batch = {"images": b["images"], "objects": b["objects"]}
    lp_ref = ref(tgt_inputs=b["tgt"], tgt_langs=b["langs"], tgt_mask=b["tgt"] != 0, batch=batch, log_softmax=True)
    lp = ours(tgt_inputs=b["tgt"], tgt_langs=b["langs"], tgt_mask=b["tgt"] != 0, batch=batch, log_softmax=True, pad_idx=0)
    assert_close(lp, lp_ref, 1e-4, "log-probs")
    targets = b["tgt"][:, 1:][b["tgt"][:, 1:] != 0]
    loss_ref = R.SmoothedNLLLoss(ignore_index=0)(lp_ref, targets).mean()
    loss_ref.backward()
    loss, n = ours.loss_fused(tgt_inputs=b["tgt"], tgt_mask=b["tgt"] != 0, tgt_langs=b["langs"], batch=batch, pad_idx=0)
    assert n == targets.numel()
    assert_close(loss.view(1), loss_ref.view(1), 1e-5, "loss")
    loss.backward()
    ref_params = dict(ref.named_parameters())
    checked = set()
    for k, p in ours.named_parameters():
        rp = ref_params.get(k)
        if rp is None or rp.grad is None:
            continue
        if k.endswith("self.key.bias"):  # exactly 0 in exact arithmetic (softmax shift invariance): rounding noise only
            assert float(p.grad.abs().max()) < 1e-6 and float(rp.grad.abs().max()) < 1e-6
            checked.add(k)
            continue
        assert_close(p.grad, rp.grad, 2e-4, "grad " + k)
        checked.add(k)
    must = ["image_model.object_feat_fc.weight", "image_model.object_embedding.weight", "multistream_attention_gate"]
    obj_keys = [k for k in ref_params if k.startswith("obj_decoder") and ref_params[k].grad is not None]
    assert len(obj_keys) > 20 and set(must + obj_keys) <= checked, set(must + obj_keys) - checked
    for k in must:
        assert float(dict(ours.named_parameters())[k].grad.abs().max()) > 0, k


def test_all_padding_labels_give_the_image_only_result(cuda):
    ref, ours = _pair()
    b = _caption_batch(counts=[0, 0, 0, 0, 0])
    kw = dict(tgt_inputs=b["tgt"], tgt_langs=b["langs"], tgt_mask=b["tgt"] != 0, log_softmax=True, pad_idx=0)
    with_objs = ours(batch={"images": b["images"], "objects": b["objects"]}, **kw)
    without = ours(batch={"images": b["images"]}, **kw)
    assert torch.equal(with_objs, without)


def test_c3_size_with_objects_bf16_against_oracle(cuda):
    """C3 (feats [32,49,2048], captions [32,32], 6L/6L d=512, V=30000) plus objects [32, <=100, 1024] with seeded per-image
    detection counts, bf16 compute: log-probs, loss and every gradient against the fp32 oracle under the C3 bf16 rule of
    tests/test_gpu_c34.py (log-probs 4e-2, loss 2e-2, gradients 1e-1 with the attention-projection exception)."""
    from imagetranslate_amd.image_model import ImageCaptioning
    from tests.test_gpu_c34 import DIMS, V, _check_bf16_argmax, _check_grads
    torch.manual_seed(33)
    tp = R.SyntheticTextProcessor(V)
    ref = ObjImageCaptioning(tp, lang_dec=False, image_feat_dim=2048, **DIMS).eval()
    with torch.no_grad():  # as tests/test_gpu_c34.py: N(0, 0.02) matrices give degenerate (uniform) softmaxes
        for k, p in ref.named_parameters():
            if p.dim() > 1:
                p.mul_(2.0)
            elif k.endswith("bias"):
                p.normal_(0.0, 0.02)
        ref.multistream_attention_gate.normal_(0.0, 1.0)
    ours = ImageCaptioning(tp, lang_dec=False, image_feat_dim=2048, use_obj=True, **DIMS)
    res = ours.load_state_dict(ref.state_dict(), strict=False)
    assert not res.unexpected_keys and all("layer_norm" in k for k in res.missing_keys), res
    ours = ours.cuda().eval()
    g = torch.Generator().manual_seed(303)
    B, T = 32, 32
    feats = torch.randn(B, 49, 2048, generator=g)
    cap = torch.randint(6, V, (B, T), generator=g)
    cap[:, 0] = 6
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    for i in range(B):
        cap[i, lens[i] - 1] = 4
        cap[i, lens[i]:] = 0
    counts = torch.randint(0, 101, (B,), generator=g).tolist()
    objs = _objects(B, 100, counts=counts, seed=304)
    n = max(counts)
    objs = {k: v[:, :n].contiguous() for k, v in objs.items()}  # trimmed to the batch maximum, as the loader does
    kw = dict(tgt_inputs=cap, tgt_mask=cap != 0, tgt_langs=torch.ones(B, dtype=torch.long), batch={"images": feats, "objects": objs})
    lp_ref = ref(**kw, log_softmax=True)
    loss_ref = R.SmoothedNLLLoss(ignore_index=0)(lp_ref, cap[:, 1:][(cap != 0)[:, 1:]]).mean()
    loss_ref.backward()
    ours.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        lp = ours(**kw, log_softmax=True, pad_idx=0)
    assert_close(lp, lp_ref.detach(), 4e-2, "C3obj bf16 log-probs")
    _check_bf16_argmax(lp, lp_ref.detach(), "C3obj")
    ours.zero_grad()
    loss, _ = ours.loss_fused(**kw, pad_idx=0)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_ref)) <= 2e-2 * abs(float(loss_ref))
    _check_grads(ours, ref, 1e-1, 200, "C3obj bf16", worst_tol=2.5e-1)
    params = dict(ours.named_parameters())
    for k in ("image_model.object_feat_fc.weight", "image_model.object_embedding.weight", "multistream_attention_gate",
              "obj_decoder.decoder.layer.5.crossattention.self.value.weight", "obj_decoder.decoder.layer.0.intermediate.dense.weight"):
        assert dict(ref.named_parameters())[k].grad is not None and float(params[k].grad.abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------ beam search
# (beam, lang_dec, B, objects per image, detections): the first two rows are the long-standing cases; the lang_dec rows are the
# toy size of an object-stream search through per-language decoders (decoder[1] and obj_decoder[1] must be the ones that run)
BEAM_CASES = [(1, False, 4, 19, [19, 3, 0, 11]), (3, False, 4, 19, [19, 3, 0, 11]),
              (1, True, 3, 5, [5, 2, 0]), (3, True, 3, 5, [5, 2, 0])]


@pytest.mark.parametrize("beam,lang_dec,B,N,counts", BEAM_CASES, ids=["1", "3", "1-lang_dec", "3-lang_dec"])
def test_beam_search_fp32_matches_oracle(cuda, beam, lang_dec, B, N, counts):
    from imagetranslate_amd.seq_gen import BeamDecoder
    ref, ours = _pair(lang_dec, seed=3)
    if lang_dec:  # the per-language stacks start as copies of one another: language 0's must differ, so that running them shows
        with torch.no_grad():
            for stack in (ref.decoder[0], ref.obj_decoder[0]):
                for lyr in stack.decoder.layer:
                    lyr.output.dense.weight.neg_()
    sd = beam_state_dict(ref.state_dict())
    ref.load_state_dict(sd)
    ours.load_state_dict(sd, strict=False)
    b = _caption_batch(B=B, N=N, seed=8, counts=counts)
    kw = dict(first_tokens=torch.full((B,), 5, dtype=torch.long), tgt_langs=torch.ones(B, dtype=torch.long), pad_idx=0, max_len=14)
    want = beam_search(ref, b["images"], b["objects"], beam, **kw)
    no_obj = beam_search(ref, b["images"], None, beam, **kw)
    assert [w.tolist() for w in want] != [w.tolist() for w in no_obj], "the object stream must change the search"
    for kv in (True, False):
        got = BeamDecoder(ours, beam_width=beam, kv_cache=kv)(images=b["images"], objects=b["objects"], **kw)
        assert [g.tolist() for g in got] == [w.tolist() for w in want], "kv_cache=%s" % kv
        # precomputed image embeddings together with objects= (the object head still runs): the same search
        with torch.no_grad():
            emb = ours.image_model(b["images"].cuda(), torch.float32)[0]
        got = BeamDecoder(ours, beam_width=beam, kv_cache=kv)(image_embed=emb, objects=b["objects"], **kw)
        assert [g.tolist() for g in got] == [w.tolist() for w in want], "image_embed=, kv_cache=%s" % kv


def test_one_launch_step_with_objects_against_chain(cuda, monkeypatch):
    """bf16, d = 512: every step's blended state of the one-launch decoder steps within bf16 tolerance of the chain's, on the
    same teacher-forced tokens (both stacks step through imt_decode_step, the slot table is shared)."""
    import ctypes
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd.param_store import store_of
    from imagetranslate_amd.seq_gen import _Incremental
    from imagetranslate_amd.image_model import ImageCaptioning
    torch.manual_seed(0)
    m = ImageCaptioning(R.SyntheticTextProcessor(3000), lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=512, intermediate_dim=2048,
                        num_attention_heads=8, image_feat_dim=64, use_obj=True)
    with torch.no_grad():
        m.multistream_attention_gate.normal_()
    m = m.cuda().eval()
    B, T = 4, 10
    b = _caption_batch(B=B, N=30, seed=12)
    ids = torch.randint(6, 3000, (T, B)).cuda()
    types = torch.ones(B, dtype=torch.long, device="cuda")
    slots = torch.arange(B, dtype=torch.int32, device="cuda").unsqueeze(1).expand(B, T).contiguous()
    store = store_of(m.decoder).ensure()
    lib = L.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    states = {}
    for mode, dtype in (("1", torch.bfloat16), ("0", torch.bfloat16), ("0", torch.float32)):
        monkeypatch.setenv("IMT_DECODE_FUSED", mode)
        m.set_compute_dtype(dtype)
        with torch.no_grad():
            emb, obj = m.encode(images=b["images"].cuda(), objects=b["objects"])
        flat = store.params_for(dtype)
        gate = store.views(dtype, m.multistream_attention_gate)[0].view(-1)
        inc = _Incremental(lib, m.decoder, store, dtype, flat, emb.contiguous(), None, B, 1, T, stream)
        inc_obj = _Incremental(lib, m.obj_decoder, store, dtype, flat, obj.contiguous(), None, B, 1, T, stream)
        h, ho = (torch.empty(B, 512, dtype=dtype, device="cuda") for _ in range(2))
        out = []
        for t in range(T):
            inc.step(t, B, 1, ids[t].contiguous(), types, slots, h)
            inc_obj.step(t, B, 1, ids[t].contiguous(), types, slots, ho)
            out.append(O.gated_mix(h, ho, gate).float())
        inc_obj.check()
        inc.check()
        states[(mode, dtype)] = out
    # the rule of tests/test_gpu_decode.py for the one-launch step: bf16 rounds pre-LayerNorm sums at other places than the
    # chain, so both bf16 paths are measured against the fp32 chain and the one-launch path may not be much further from it
    from tests.util import rel_err
    for t in range(T):
        one, chain, f32 = states[("1", torch.bfloat16)][t], states[("0", torch.bfloat16)][t], states[("0", torch.float32)][t]
        e_one, e_chain = rel_err(one, f32), rel_err(chain, f32)
        assert e_one <= max(1e-2, 1.5 * e_chain), "step %d: one launch %.2e from the fp32 chain, the bf16 chain %.2e" % (t, e_one, e_chain)
        assert_close(one, chain, 6e-2, "blended state, step %d" % t)


@pytest.mark.parametrize("beam", [1, 3])
def test_beam_search_with_objects_one_launch_against_chain(cuda, monkeypatch, beam):
    """A whole BeamDecoder search with objects= at the size where both stacks take the one-launch step (bf16, d = 512), against
    the chain: the rule of tests/test_gpu_decode.py::test_beam_search_with_the_one_launch_step (the first tokens agree on nearly
    every sentence; later positions may part where bf16 rounding flips a near-tie), and the objects change the search."""
    from imagetranslate_amd.image_model import ImageCaptioning
    from imagetranslate_amd.seq_gen import BeamDecoder
    torch.manual_seed(11)
    m = ImageCaptioning(R.SyntheticTextProcessor(1000), lang_dec=False, enc_layer=2, dec_layer=3, embed_dim=512, intermediate_dim=2048,
                        num_attention_heads=8, image_feat_dim=64, use_obj=True)
    with torch.no_grad():
        m.multistream_attention_gate.normal_()
    m.set_compute_dtype(torch.bfloat16)
    m = m.cuda().eval()
    B = 12
    b = _caption_batch(B=B, N=40, seed=21)
    args = dict(images=b["images"], first_tokens=torch.full((B,), 5, dtype=torch.long), tgt_langs=torch.ones(B, dtype=torch.long),
                pad_idx=0, max_len=12)
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("IMT_DECODE_FUSED", fused)
        outs[fused] = BeamDecoder(m, beam_width=beam, kv_cache=True)(objects=b["objects"], **args)
    head = sum(int(x[:4].tolist() == y[:4].tolist()) for x, y in zip(outs["1"], outs["0"]))
    assert head >= B - 2, "the first tokens of %d of %d sentences differ between the one-launch step and the chain" % (B - head, B)
    for o in outs["1"]:
        assert int(o[0]) == 5 and 2 <= len(o) <= 12 and bool(((o >= 0) & (o < 1000)).all())
    monkeypatch.setenv("IMT_DECODE_FUSED", "1")
    plain = BeamDecoder(m, beam_width=beam, kv_cache=True)(**args)
    assert [o.tolist() for o in plain] != [o.tolist() for o in outs["1"]], "the object stream must change the search"


# ------------------------------------------------------------------------------------------------ CLIs
def test_train_and_caption_cli_with_objects(cuda, tmp_path, capsys):
    import marshal
    from imagetranslate_amd import caption, train_captioning
    from imagetranslate_amd.dataset import ImageDataset
    from imagetranslate_amd.image_model import ImageCaptioning
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.seq_gen import BeamDecoder
    from tests.test_gpu_cli import _corpus
    from imagetranslate_amd import train_tokenizer
    from imagetranslate_amd.textprocessor import TextProcessor
    d = str(tmp_path)
    src, _ = _corpus(100, 4)
    with open(os.path.join(d, "all.txt"), "w") as fw:
        fw.write("\n".join(["<xa> " + s + " </s>" for s in src]) + "\n")
    tok = os.path.join(d, "tok")
    train_tokenizer.main(["--data", os.path.join(d, "all.txt"), "--vocab_size", "200", "--model", tok])
    tp = TextProcessor(tok)
    n_img = 24
    torch.manual_seed(0)
    objs = _objects(n_img, 12, seed=5)
    paths = ["img%02d.jpg" % i for i in range(n_img)]
    img_dir = os.path.join(d, "images")
    os.makedirs(img_dir)
    torch.save({"paths": paths, "feats": torch.randn(n_img, 49, 64), "obj_feats": objs["feats"], "obj_boxes": objs["boxes"],
                "obj_labels": objs["labels"]}, os.path.join(img_dir, "features.pt"))
    caps = sorted([(i, tp.tokenize_one_sentence_with_langid(src[i % 8], tp.token_id("<xa>"))) for i in range(n_img)], key=lambda c: len(c[1]))
    with open(os.path.join(d, "train.cap"), "wb") as fw:
        marshal.dump(({i: paths[i] for i in range(n_img)}, caps), fw)
    model_dir = os.path.join(d, "cap_model")
    torch.manual_seed(1)
    init = ImageCaptioning(tp, lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4,
                           image_feat_dim=64, use_obj=True)
    before = {k: v.clone() for k, v in init.state_dict().items() if "object" in k or "obj_decoder" in k or "multistream" in k}
    init.save(os.path.join(d, "init"))
    train_captioning.main(["--train", os.path.join(d, "train.cap"), "--image", img_dir, "--tok", tok, "--model", model_dir,
                           "--pretrained", os.path.join(d, "init"), "--max-image", "8", "--batch", "1200", "--lr", "0.003",
                           "--warmup", "5", "--step", "6", "--log-steps", "2", "--eval-steps", "1000", "--fp32"])
    log = capsys.readouterr().out
    losses = [float(ln.split("Loss: ")[1].split()[0]) for ln in log.splitlines() if "Epoch Step" in ln]
    assert losses and all(torch.isfinite(torch.tensor(losses))), log
    trained = Seq2Seq.load(ImageCaptioning, model_dir, tok_dir=tok, use_obj=True)
    after = trained.state_dict()
    for k in ("image_model.object_feat_fc.weight", "image_model.object_embedding.weight", "multistream_attention_gate",
              "obj_decoder.decoder.layer.0.crossattention.self.key.weight"):
        assert not torch.equal(after[k].cpu(), before[k]), "%s did not move" % k
    out_file = os.path.join(d, "captions.txt")
    caption.main(["--input", img_dir, "--target", "xa", "--output", out_file, "--tok", tok, "--model", model_dir, "--beam", "2",
                  "--batch", "8", "--max-len", "16", "--fp32", "--obj"])
    lines = dict(ln.split("\t", 1) for ln in open(out_file).read().rstrip("\n").split("\n"))  # a caption may be empty
    trained = trained.cuda().eval()
    gen = BeamDecoder(trained, beam_width=2, max_len_a=1.3, max_len_b=5, len_penalty_ratio=0.8)
    data = ImageDataset(img_dir, 8, target_lang=tp.languages["<xa>"], first_token=tp.token_id("<xa>"))
    for i in range(len(data)):
        bt = data[i]
        assert "objects" in bt
        hyps = gen(first_tokens=bt["first_tokens"], images=bt["images"], tgt_langs=bt["tgt_langs"], pad_idx=tp.pad_token_id(),
                   max_len=16, objects=bt["objects"])
        for p, h in zip(bt["paths"], hyps):
            assert lines[p] == tp.decode(h[1:].tolist())


# ------------------------------------------------------------------------------------------------ stale layout
@pytest.mark.parametrize("node", ["linear", "fused_loss", "image_head", "object_head", "gated_mix", "contrastive_tail"])
def test_backward_after_a_rebuilt_layout_is_refused(cuda, node):
    """Every node that addresses the flat buffers records the layout version in forward; after a rebuild its backward
    raises instead of writing gradients at the offsets of the old layout (nothing reaches the new gradient buffer)."""
    from imagetranslate_amd._lib import ImtError
    from imagetranslate_amd.image_model import ImageCaptioning, _ContrastiveTailFn, gated_mix
    from imagetranslate_amd.param_store import store_of
    from imagetranslate_amd.seq2seq import _FusedXentFn
    torch.manual_seed(0)
    m = ImageCaptioning(R.SyntheticTextProcessor(1000), lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256,
                        num_attention_heads=4, image_feat_dim=64, use_obj=True).cuda().eval()
    store = store_of(m.encoder).ensure()
    g = torch.Generator().manual_seed(1)
    rows = lambda *shape: torch.randn(*shape, generator=g).cuda().requires_grad_()
    if node == "linear":
        out = m.output_layer[1](rows(5, 128))
    elif node == "fused_loss":
        lin = m.output_layer[1].layer
        out = _FusedXentFn.apply(rows(5, 128), lin.weight, lin.bias, torch.randint(6, 1000, (5,), generator=g).cuda(), 0.1, 0)
    elif node == "image_head":
        out = m.image_model(torch.randn(2, 49, 64, generator=g))[0]
    elif node == "object_head":
        out = m.image_model.objects_forward(_objects(2, 5, counts=[5, 2], seed=3))
    elif node == "gated_mix":
        out = gated_mix(m, m.multistream_attention_gate, rows(2, 3, 128), rows(2, 3, 128))
    else:
        mask = torch.ones(2, 6, dtype=torch.bool, device="cuda")
        out = _ContrastiveTailFn.apply(store.anchor_if_grad(), rows(2, 6, 128), mask, rows(2, 6, 128), mask, rows(2, 49, 128), m)
    assert out.requires_grad
    store.rebuild()
    with pytest.raises(ImtError, match="parameter layout changed between forward and backward"):
        out.float().sum().backward()
    torch.cuda.synchronize()
    assert float(store.grad.abs().sum()) == 0.0
