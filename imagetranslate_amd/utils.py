"""Trainer-side pieces of the path -- drop-in for the parts of the reference's ``src/utils.py`` that sit inside the
timed train step: ``build_optimizer`` (:14-16), ``AdamInverseSqrtWithWarmup`` (:105-156), gradient clipping
(``train_image_mt.py:291``), plus ``mass_mask`` / ``mass_unmask`` (:41-82, host-side batch construction, kept on the
host exactly as the reference), ``mask_text`` / ``unmask_text`` (:19-38, BERT masking for the masked LM; on the device
``mask_text_device`` = ``imt_mlm_mask``) and ``backward`` (:85-90).

The optimizer works on the model's FLAT buffers: global grad-norm = one reduction kernel, clip + Adam + bf16 shadow
write + grad zeroing = one elementwise kernel (``imt_sumsq`` / ``imt_clip_adam``).
"""
import math
import random
from typing import Dict

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from . import hip_ops as O


def build_optimizer(model, learning_rate, warump_steps):
    return AdamInverseSqrtWithWarmup(model.parameters(), lr=learning_rate, betas=(0.9, 0.98),
                                     warmup_updates=warump_steps)


def backward(loss, optimizer=None, fp16: bool = False):
    # bf16 keeps fp32's exponent range: no loss scaling (the reference needs apex amp.scale_loss for fp16, :85-90)
    loss.backward()


class AdamInverseSqrtWithWarmup(torch.optim.Optimizer):
    """Adam whose lr follows linear warm-up then inverse-sqrt decay, updated AFTER each step (src/utils.py:105-156).

    ``step(max_grad_norm=..., grad_scale=...)`` additionally fuses ``clip_grad_norm_`` (and the 1/world_size of
    data-parallel averaging) into the same kernel; plain ``step()`` after an external
    ``torch.nn.utils.clip_grad_norm_`` (the reference's call sequence) gives the same result.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_updates=4000,
                 warmup_init_lr=1e-7):
        if weight_decay != 0:
            raise ValueError("weight_decay is not used by the reference (src/utils.py:14-16) and not supported")
        defaults = dict(lr=warmup_init_lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.warmup_updates = warmup_updates
        self.warmup_init_lr = warmup_init_lr
        warmup_end_lr = lr
        self.lr_step = (warmup_end_lr - warmup_init_lr) / warmup_updates
        self.decay_factor = warmup_end_lr * warmup_updates ** 0.5
        for param_group in self.param_groups:
            param_group['num_updates'] = 0
        self.max_lr = lr
        self._sumsq = None
        self._partial = None
        import os
        self._partial_ok = os.environ.get("IMT_PARTIAL_NORM", "1") != "0"
        self.last_grad_norm_sq = None  # device tensor of the last fused grad-norm^2 (no host sync)

    def get_lr_for_step(self, num_updates):
        if num_updates < self.warmup_updates:
            return self.warmup_init_lr + num_updates * self.lr_step
        return max(self.warmup_init_lr, min(self.max_lr, self.decay_factor * (num_updates ** -0.5)))

    def reset(self):
        for param_group in self.param_groups:
            param_group['num_updates'] = 0

    # ------------------------------------------------------------------ state that travels (checkpoint.py)
    def _params(self):
        return [p for g in self.param_groups for p in g['params']]

    @torch.no_grad()
    def state_dict(self):
        """What torch's Adam would return: ``param_groups`` (with ``num_updates`` and ``lr``) and ``state[i] = {"exp_avg",
        "exp_avg_sq"}`` shaped like parameter ``i``.  On the fused path the moments live in the flat store, not in
        ``self.state``: they are COPIED out of the store's spans here (after an update still running on the side stream)."""
        params = self._params()
        index, groups = {id(p): i for i, p in enumerate(params)}, []
        for g in self.param_groups:
            groups.append({**{k: v for k, v in g.items() if k != 'params'}, 'params': [index[id(p)] for p in g['params']]})
        st = self._store()
        state = {}
        if st is not None:
            st.ensure()
            st.wait_updates(0)
            if st.exp_avg is not None:
                for i, p in enumerate(params):
                    state[i] = {'exp_avg': st._view(st.exp_avg, p).clone(), 'exp_avg_sq': st._view(st.exp_avg_sq, p).clone()}
        else:
            for i, p in enumerate(params):
                if self.state.get(p):
                    state[i] = {k: self.state[p][k].clone() for k in ('exp_avg', 'exp_avg_sq')}
        return {'state': state, 'param_groups': groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Moments back into the flat store at each parameter's offset (generic path: into ``self.state``), ``num_updates``
        from the file, ``lr`` from THIS optimizer's schedule at that update count: a resumed run may be given another --lr or
        --warmup, the file decides only how far the schedule has advanced.  A parameter without saved moments gets zeros.
        Another parameter count or another shape is refused."""
        params, state = self._params(), state_dict['state']
        saved_groups = state_dict['param_groups']
        n_saved = sum(len(g['params']) for g in saved_groups)
        if n_saved != len(params) or len(saved_groups) != len(self.param_groups):
            raise ValueError("optimizer state holds %d parameters in %d groups, this optimizer has %d in %d"
                             % (n_saved, len(saved_groups), len(params), len(self.param_groups)))
        for i, p in enumerate(params):
            for k in ('exp_avg', 'exp_avg_sq'):
                if i in state and tuple(state[i][k].shape) != tuple(p.shape):
                    raise ValueError("optimizer state: %s of parameter %d has shape %s, the parameter has %s"
                                     % (k, i, tuple(state[i][k].shape), tuple(p.shape)))
        st = self._store()
        if st is not None:
            st.ensure()
            st.wait_updates(0)
            m, v = st.moments()
            for i, p in enumerate(params):
                for buf, k in ((m, 'exp_avg'), (v, 'exp_avg_sq')):
                    view = st._view(buf, p)
                    if i in state:
                        view.copy_(state[i][k])
                    else:
                        view.zero_()
        else:
            for i, p in enumerate(params):
                if i in state:
                    self.state[p] = {k: state[i][k].to(device=p.device, dtype=p.dtype).clone() for k in ('exp_avg', 'exp_avg_sq')}
                else:
                    self.state.pop(p, None)
        for g, saved in zip(self.param_groups, saved_groups):
            g['num_updates'] = int(saved['num_updates'])
            g['lr'] = self.get_lr_for_step(g['num_updates'])

    def _store(self):
        st = None
        n = 0
        for g in self.param_groups:
            for p in g['params']:
                ref = getattr(p, "_imt_store", None)
                s = ref() if ref is not None else None
                if s is None or (st is not None and s is not st):
                    return None
                st = s
                n += 1
        if st is None or n != len(st.entries):
            return None
        return st

    def zero_grad(self, set_to_none: bool = False):
        st = self._store()
        if st is not None and st.valid():
            st.zero_grad()
            st.attach_grad_views()
        else:
            super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm: float = 0.0, grad_scale: float = 1.0, zero_grad: bool = False,
             overlap_next_forward: bool = False):
        """``overlap_next_forward`` (fused path only): the update runs on a side stream in three segments -- encoder +
        embeddings, decoder, output layers -- and each stack of the NEXT forward waits only for the segments it reads
        (FlatParams.wait_updates), so the HBM-bound update of the decoder / output layers runs under the encoder's
        latency-bound kernels.  Same arithmetic, same order of operations per parameter."""
        if closure is not None:
            raise ValueError("closures are not supported")
        st = self._store()
        if st is None:
            # parameters that do not (all) live in one flat store: generic per-tensor path on the GPU
            self._generic_step(max_grad_norm, grad_scale)
        else:
            st.ensure()
            g = self.param_groups[0]
            step = g['num_updates'] + 1
            m, v = st.moments()
            sumsq = None
            if max_grad_norm and max_grad_norm > 0:
                sumsq = self._grad_norm_sq(st)
                self.last_grad_norm_sq = sumsq
                if self._partial_ok and getattr(st, "stack_done_hook", None) is None:
                    st.stack_done_hook = self._stack_done  # from the next backward on: part of the norm under the backward
            else:
                self._partial = None
            segs = self._segments(st) if overlap_next_forward else None
            if segs is None:
                O.clip_adam(st.flat, st.grad, m, v, st.shadow_buffer_for_optimizer(), sumsq, float(max_grad_norm or 0.0),
                            float(grad_scale), float(g['lr']), g['betas'][0], g['betas'][1], g['eps'], step,
                            zero_grad=zero_grad)
            else:
                main = torch.cuda.current_stream()
                if getattr(self, "_side", None) is None:
                    self._side = torch.cuda.Stream()
                st.wait_updates(0)
                done = torch.cuda.Event()
                done.record(main)           # backward, all-reduce and the grad norm are enqueued before this point
                self._side.wait_event(done)
                sh = st.shadow_buffer_for_optimizer()
                events = []
                with torch.cuda.stream(self._side):
                    for lo, hi in segs:     # highest offsets first: what the next forward needs first
                        O.clip_adam(st.flat[lo:hi], st.grad[lo:hi], m[lo:hi], v[lo:hi], None if sh is None else sh[lo:hi], sumsq,
                                    float(max_grad_norm or 0.0), float(grad_scale), float(g['lr']), g['betas'][0], g['betas'][1],
                                    g['eps'], step, zero_grad=zero_grad)
                        ev = torch.cuda.Event()
                        ev.record(self._side)
                        events.append((lo, hi, ev))
                st._update_events = events
            if zero_grad:
                st.grad_generation += 1  # (a partial gradient norm taken before this point is void)
            if st.shadow_buffer_for_optimizer() is not None:
                st.note_shadow_written_by_optimizer()
            else:
                st.mark_master_changed()
        for param_group in self.param_groups:
            param_group['num_updates'] += 1
            param_group['lr'] = self.get_lr_for_step(param_group['num_updates'])

    @staticmethod
    def _segments(st):
        """[(lo, hi)] of the flat buffer in the order the next forward needs them: embeddings (and whatever follows them),
        encoder layers 0, 1, ... (each its own segment: the encoder forward waits layer by layer, FlatParams.site_events),
        decoder(s), output layers -- None when the model does not expose that structure."""
        root = st._root()
        try:
            enc_layers = list(root.encoder.encoder.layer)
            starts = [st.span(lyr.ordered_params())[0] for lyr in enc_layers]  # flat order: top layer first
            emb_lo = st.span(root.encoder.embeddings.parameters())[0]
            decs = list(root.decoder) if isinstance(root.decoder, torch.nn.ModuleList) else [root.decoder]
            dec_lo = st.span(p for d in decs for p in d.parameters())[0]
            enc_lo = min(starts)
        except Exception:
            return None
        if not (0 < dec_lo < enc_lo < emb_lo < st.total) or sorted(starts, reverse=True) != starts:
            return None
        segs = [(emb_lo, st.total)]
        for l in range(len(enc_layers)):  # layer l spans [its first parameter, the first parameter of layer l - 1 / the embeddings)
            segs.append((starts[l], starts[l - 1] if l > 0 else emb_lo))
        segs += [(dec_lo, enc_lo), (0, dec_lo)]
        return segs

    # ------------------------------------------------------------------ gradient norm, part of it under the backward
    def _stack_done(self, mod, is_decoder):
        """FlatParams.stack_done_hook: when the DECODER's backward has been enqueued, every gradient below the encoder's range
        (output layers, decoder) is final -- its share of the squared norm is summed on the side stream while the encoder's
        backward runs; step() then only adds the encoder + embedding range.  Fixed order of the two partial sums:
        deterministic.  Off under a data-parallel exchange (the norm is of the REDUCED gradients) and with IMT_PARTIAL_NORM=0."""
        if not is_decoder or not self._partial_ok:
            return  # (the encoder's backward comes after the decoder's and leaves the partial sum valid)
        self._partial = None
        st = self._store()
        if st is None or getattr(st, "segment_hook", None) is not None:
            return
        segs = self._segments(st)
        if segs is None:
            return
        enc_lo = segs[-2][1]
        self._ensure_norm_buffers(st)
        main = torch.cuda.current_stream()
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream()
        ready = torch.cuda.Event()
        ready.record(main)
        self._side.wait_event(ready)
        with torch.cuda.stream(self._side):
            self._sumsq.zero_()
            O.sumsq(st.grad[:enc_lo], self._sumsq, self._sumsq_ws_side)
            done = torch.cuda.Event()
            done.record(self._side)
        self._partial = (enc_lo, done, (st.layout_version, st.grad_generation))

    def _ensure_norm_buffers(self, st):
        if self._sumsq is None or self._sumsq.device != st.flat.device:
            self._sumsq = torch.zeros(1, device=st.flat.device)
            self._sumsq_ws = torch.empty(1024, device=st.flat.device, dtype=torch.float32)
            self._sumsq_ws_side = torch.empty(1024, device=st.flat.device, dtype=torch.float32)

    def _grad_norm_sq(self, st):
        """sum(g^2) over the flat gradient buffer as a device scalar (no host sync)."""
        self._ensure_norm_buffers(st)
        part, self._partial = getattr(self, "_partial", None), None
        if part is not None and part[2] == (st.layout_version, st.grad_generation):
            enc_lo, done, _ = part
            torch.cuda.current_stream().wait_event(done)
            O.sumsq(st.grad[enc_lo:], self._sumsq, self._sumsq_ws)  # adds to the partial sum
        else:
            self._sumsq.zero_()
            O.sumsq(st.grad, self._sumsq, self._sumsq_ws)
        return self._sumsq

    def _generic_step(self, max_grad_norm, grad_scale):
        params = [p for g in self.param_groups for p in g['params'] if p.grad is not None]
        if grad_scale != 1.0:
            for p in params:
                p.grad.mul_(grad_scale)
        if max_grad_norm and max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
        for g in self.param_groups:
            b1, b2 = g['betas']
            t = g['num_updates'] + 1
            for p in g['params']:
                if p.grad is None:
                    continue
                state = self.state[p]
                if not state:
                    state['exp_avg'] = torch.zeros_like(p)
                    state['exp_avg_sq'] = torch.zeros_like(p)
                m, v = state['exp_avg'], state['exp_avg_sq']
                m.mul_(b1).add_(p.grad, alpha=1 - b1)
                v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                denom = (v.sqrt() / math.sqrt(1 - b2 ** t)).add_(g['eps'])
                p.addcdiv_(m, denom, value=-g['lr'] / (1 - b1 ** t))


# ----------------------------------------------------------------------------------------- host batch construction
def _mass_span_start(length_hint: int) -> int:
    """Start of the masked span: 20% from position 1, 20% from the middle bound, 60% uniformly in [2, bound]
    (same draw order as the reference, src/utils.py:52-60, so seeded runs produce the same batches)."""
    draw = random.random()
    if draw > 0.8:
        return 1
    if draw > 0.6:
        return length_hint
    return random.randint(2, length_hint) if length_hint >= 2 else 2


def mass_mask(mask_prob, pad_indices, src_text, text_processor) -> Dict:
    """MASS batch construction on the host (semantics of src/utils.py:41-78): per row a contiguous span of
    int(len/2) tokens is hidden from the encoder; the decoder is fed the span shifted right (``to_recover``) with
    its ORIGINAL positions (``positions``); hidden tokens are replaced 80/10/10 by <mask>/random/unchanged."""
    assert 0 < mask_prob < 1
    n_rows, width = src_text.size()
    pad_id = text_processor.pad_token_id()
    span_mask = torch.zeros((n_rows, width), dtype=torch.bool)
    spans, span_pos = [], []
    bounds = pad_indices - (1 - mask_prob) * pad_indices
    for row in range(n_rows):
        span_len = int(pad_indices[row] / 2)
        first = _mass_span_start(int(math.ceil(bounds[row])))
        last = first + span_len
        span_mask[row, first:last] = True
        spans.append(src_text[row, first - 1:last])
        span_pos.append(torch.arange(first - 1, last))
    to_recover = pad_sequence(spans, batch_first=True, padding_value=pad_id)
    positions = pad_sequence(span_pos, batch_first=True, padding_value=int(width) - 1)

    targets = src_text[:, 1:][span_mask[:, 1:]]
    originals = src_text[span_mask]
    n_special = len(text_processor.special_tokens)
    vocab = text_processor.vocab_size()
    mask_id = text_processor.mask_token_id()
    replaced = []
    for k in range(originals.size(0)):
        draw = random.random()
        if draw < 0.8:
            replaced.append(mask_id)
        elif draw < 0.9:
            replaced.append(random.randint(n_special, vocab - 1))
        else:
            replaced.append(int(originals[k]))
    src_text[span_mask] = torch.tensor(replaced, dtype=torch.long)
    return {"src_mask": span_mask, "targets": targets, "src_text": src_text, "to_recover": to_recover,
            "positions": positions, "mask_idx": originals}


def mass_unmask(src_text, src_mask, masked_ids):
    """Undo mass_mask in place after the step (src/utils.py:81-82)."""
    src_text[src_mask] = masked_ids


def mask_text(mask_prob, pads, texts, text_processor, mask_eos: bool = True):
    """BERT masking on the host (semantics of src/utils.py:19-33): every real token is chosen with probability ``mask_prob``
    (never a pad; never ``</s>`` with ``mask_eos=False``); a chosen token becomes <mask> (80%), a random non-special id (10%)
    or stays (10%).  ``texts`` is modified in place.  Returns (mask, the original ids at the mask in row-major order, texts)."""
    assert 0 < mask_prob < 1
    mask = (torch.rand(texts.size()) < mask_prob) & pads.bool()
    if not mask_eos:
        mask &= texts != text_processor.sep_token_id()
    masked_ids = texts[mask]
    n_special, vocab, mask_id = len(text_processor.special_tokens), text_processor.vocab_size(), text_processor.mask_token_id()
    replaced = []
    for k in range(masked_ids.size(0)):
        draw = random.random()
        if draw < 0.8:
            replaced.append(mask_id)
        elif draw < 0.9:
            replaced.append(random.randint(n_special, vocab - 1))
        else:
            replaced.append(int(masked_ids[k]))
    texts[mask] = torch.tensor(replaced, dtype=torch.long)
    return mask, masked_ids, texts


def unmask_text(mask, masked_ids, texts):
    """Undo mask_text in place (src/utils.py:36-38)."""
    texts[mask] = masked_ids


# ----------------------------------------------------------------------------------------- device batch construction
_U32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    """csrc/common.hpp mix32 on uint64 arrays holding 32-bit values (no product leaves 64 bits)."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _U32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _U32
    return x ^ (x >> np.uint64(16))


def _counter_uniform(seed: int, stream: int, index):
    """csrc/common.hpp counter_uniform(seed, stream, index) for an array of indices below 2^32: float32 in [0, 1), 24 bits."""
    index = np.asarray(index).astype(np.uint64)
    h = _mix32((index ^ np.uint64(seed & 0xFFFFFFFF)) & _U32)
    h = _mix32((h + np.uint64((stream * 0x9E3779B9 + (seed >> 32)) & 0xFFFFFFFF)) & _U32)
    return (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)   # both factors and the product are exact in float32


def mass_span_starts(mask_prob, pad_indices, seed: int):
    """Span start of every row of a MASS batch (src/utils.py:52-60) on the draws imt_mass_mask's generator gives for
    (seed, stream 0 / 1, row): int64 [n_rows] on the host, no device work (numpy: a few microseconds per operator at batch
    sizes).  The bound ceil(pad - (1 - p) * pad) is float32 with TWO roundings like the reference's tensor expression (product,
    then difference; pad = 50, p = 0.3: 50 - 35.0 = 15, a fused multiply-add gives 15.0000006 and a bound of 16), which
    separate array operators keep."""
    pad = pad_indices.detach().cpu().to(torch.int64).numpy()
    rows = np.arange(pad.size, dtype=np.uint64)
    padf = pad.astype(np.float32)
    prod = (np.float32(1.0) - np.float32(mask_prob)) * padf
    hint = np.ceil(padf - prod).astype(np.int64)
    u0, u1 = _counter_uniform(int(seed), 0, rows), _counter_uniform(int(seed), 1, rows)
    drawn = 2 + (u1 * (hint - 1).astype(np.float32)).astype(np.int64)   # float32 product, truncated
    uniform = np.where(hint >= 2, np.minimum(drawn, hint), 2)
    first = np.where(u0 > np.float32(0.8), 1, np.where(u0 > np.float32(0.6), hint, uniform))
    return torch.from_numpy(first.astype(np.int64))


def mass_span_sizes(first, pad_indices, width: int):
    """(span start, number of hidden tokens) of every row as mass_mask_kernel (csrc/batch.hip) reads them -- the host's only
    copy of the kernel's arithmetic (include/imt_hip.h: f, len, hidden), so change the two together: the start clamped to
    [1, width], the span length int(pad / 2) clamped to [0, width], the span clipped at the row's end."""
    first = first.clamp(1, width)
    length = (pad_indices.detach().cpu().to(torch.int64) // 2).clamp(0, width)
    return first, torch.clamp(first + length, max=width) - first


def mass_mask_device(mask_prob, pad_indices, src_text, text_processor, seed: int) -> Dict:
    """mass_mask on the GPU (imt_mass_mask): same outputs and the same in-place semantics as ``mass_mask`` above, all
    tensors on the device of ``src_text``.  Span starts and the 80/10/10 replacement use the kernel's counter-based
    generator keyed by ``seed`` instead of Python's ``random`` (same procedure, different stream).  The span starts are
    drawn on the host (``mass_span_starts``) and handed to the kernel: a span is clipped at the row's end like a Python
    slice, so the number of hidden tokens of a row -- and with it every output size -- depends on where the span starts.
    Nothing is read back from the device."""
    import ctypes
    from . import _lib as L
    if not src_text.is_cuda:
        raise L.ImtError("mass_mask_device needs src_text on the GPU (use mass_mask on the host)")
    assert 0 < mask_prob < 1
    n_rows, width = src_text.shape
    pad_host = pad_indices.detach().cpu().to(torch.int64)
    first, span_len = mass_span_sizes(mass_span_starts(mask_prob, pad_host, seed), pad_host, width)   # hidden tokens per row
    offsets = torch.cumsum(span_len, 0) - span_len
    total, recover_width = int(span_len.sum()), int(span_len.max()) + 1
    dev = src_text.device
    src_text = src_text.contiguous()
    out = {"src_mask": torch.empty((n_rows, width), dtype=torch.uint8, device=dev),
           "to_recover": torch.empty((n_rows, recover_width), dtype=torch.int64, device=dev),
           "positions": torch.empty((n_rows, recover_width), dtype=torch.int64, device=dev),
           "targets": torch.empty(total, dtype=torch.int64, device=dev)}
    pad_dev, off_dev, first_dev = pad_indices.to(dev, torch.int64).contiguous(), offsets.to(dev), first.to(dev)
    a = L.MassArgs()
    a.n_rows, a.width, a.recover_width = n_rows, width, recover_width
    a.n_special, a.vocab = len(text_processor.special_tokens), text_processor.vocab_size()
    a.mask_prob, a.seed = float(mask_prob), int(seed)
    a.mask_id, a.pad_id = text_processor.mask_token_id(), text_processor.pad_token_id()
    a.src_text, a.pad_indices, a.row_offsets = src_text.data_ptr(), pad_dev.data_ptr(), off_dev.data_ptr()
    a.first = first_dev.data_ptr()
    a.src_mask, a.to_recover = out["src_mask"].data_ptr(), out["to_recover"].data_ptr()
    a.positions, a.targets = out["positions"].data_ptr(), out["targets"].data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().imt_mass_mask(ctypes.byref(a), st), "imt_mass_mask")
    out["src_mask"] = out["src_mask"].bool()
    out["src_text"] = src_text
    out["mask_idx"] = out["targets"]
    out["_row_offsets"] = off_dev
    return out


def mass_unmask_device(masked: Dict):
    """Restore the source ids hidden by mass_mask_device (in place)."""
    import ctypes
    from . import _lib as L
    t, m = masked["src_text"], masked["src_mask"].to(torch.uint8).contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().imt_mass_unmask(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(m.data_ptr()),
                                     ctypes.c_void_p(masked["mask_idx"].data_ptr()), ctypes.c_void_p(masked["_row_offsets"].data_ptr()),
                                     t.shape[0], t.shape[1], st), "imt_mass_unmask")


def _mlm_selected(mask_prob, pads, texts, eos_id: int, seed: int, mask_eos: bool = True):
    """selected(p) of imt_mlm_mask (include/imt_hip.h) for host arrays: bool [B, S].  The comparison is float32 on both sides."""
    pads, texts = np.asarray(pads).astype(bool), np.asarray(texts)
    u = _counter_uniform(int(seed), 4, np.arange(texts.size, dtype=np.uint64)).reshape(texts.shape)
    sel = pads & (u < np.float32(mask_prob))
    if not mask_eos:
        sel &= texts != eos_id
    return sel


def mask_text_count(mask_prob, pads, texts, text_processor, seed: int, mask_eos: bool = True) -> int:
    """How many positions imt_mlm_mask selects for this batch and seed, from the HOST copy of the batch: the kernel's draw
    restated in numpy (stream 4 of ``_counter_uniform``, index = flat position), the way ``mass_span_starts`` restates the span
    draws -- so a training step sizes ``idx`` / ``targets`` without reading the device count back."""
    sel = _mlm_selected(mask_prob, pads.detach().cpu().numpy(), texts.detach().cpu().numpy(), text_processor.sep_token_id(), seed,
                        mask_eos)
    return int(sel.sum())


def mask_text_device(mask_prob, pads, texts, text_processor, seed: int, mask_eos: bool = True, count=None) -> Dict:
    """mask_text on the GPU (imt_mlm_mask): the draw, the 80/10/10 replacement in place and the ordered compaction of the masked
    positions in one launch, on the kernel's counter-based generator keyed by ``seed`` (streams 4-6).  ``texts`` is modified in
    place and must therefore be a contiguous int64 CUDA tensor.  Returns {"mask" bool [B, S], "targets" int64 [n] (the original
    ids, == the reference's texts[mask]), "idx" int32 [n] (their flat positions), "texts", "count" (device int32 [1])}.
    ``count``: the number of selected positions when the caller has it on the host (``mask_text_count``) -- nothing is read
    back then; without it the count is read once, as ``hip_ops.select_plan`` does.  IMT_CHECK_COUNT=1 verifies a given count."""
    import ctypes
    import os
    from . import _lib as L
    if not (torch.is_tensor(texts) and texts.is_cuda and texts.dtype == torch.int64 and texts.dim() == 2 and texts.is_contiguous()):
        raise L.ImtError("mask_text_device modifies texts in place: it needs a contiguous int64 [B, S] tensor on the GPU "
                         "(use mask_text on the host)")
    assert 0 < mask_prob < 1
    n_rows, width = texts.shape
    dev = texts.device
    pads = pads.to(dev)
    if pads.dtype == torch.bool:
        pads = pads.view(torch.uint8)  # same element size: the strides stay, a column slice of a wider mask is read in place
    if pads.dtype != torch.uint8 or tuple(pads.shape) != (n_rows, width):
        raise L.ImtError("mask_text_device: pads must be a bool / uint8 tensor of the shape of texts")
    if pads.stride(1) != 1:
        pads = pads.contiguous()
    n = n_rows * width
    mask = torch.empty((n_rows, width), dtype=torch.uint8, device=dev)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    targets = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    count_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return {"mask": mask.bool(), "targets": targets[:0], "idx": idx[:0], "texts": texts, "count": count_dev}
    a = L.MlmArgs()
    a.n_rows, a.width = n_rows, width
    a.n_special, a.vocab = len(text_processor.special_tokens), text_processor.vocab_size()
    a.mask_eos, a.mask_prob, a.seed = int(bool(mask_eos)), float(mask_prob), int(seed)
    a.mask_id, a.eos_id = text_processor.mask_token_id(), text_processor.sep_token_id()
    a.texts, a.pads, a.ld_pads = texts.data_ptr(), pads.data_ptr(), pads.stride(0)
    a.mask, a.idx, a.targets, a.count = mask.data_ptr(), idx.data_ptr(), targets.data_ptr(), count_dev.data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().imt_mlm_mask(ctypes.byref(a), st), "imt_mlm_mask")
    if count is None or os.environ.get("IMT_CHECK_COUNT"):
        k = int(count_dev.item())
        if count is not None and int(count) != k:
            raise L.ImtError("mask_text_device: count hint %d but the kernel selected %d positions" % (int(count), k))
    else:
        k = int(count)
    return {"mask": mask.bool(), "targets": targets[:k], "idx": idx[:k], "texts": texts, "count": count_dev}


def unmask_text_device(masked: Dict):
    """Restore the ids hidden by mask_text_device (in place): the originals scattered back at their flat positions."""
    masked["texts"].view(-1)[masked["idx"].long()] = masked["targets"]
