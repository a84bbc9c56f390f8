"""Beam search -- drop-in for the reference's ``src/seq_gen.py`` (``BeamDecoder`` ``:27-242``,
``get_outputs_until_eos`` ``:6-24``), same constructor / ``forward`` signature and outputs.

What differs is HOW a step is computed:
  * the reference re-runs the decoder over the whole prefix at every step (``:164-166``) and re-projects the
    encoder states to cross-attention K/V in every layer of every step.  Here (``kv_cache=True``, the default) one
    step decodes ONE position per hypothesis against a self-attention q|k|v cache and per-sentence cross K/V
    computed once (``imt_decode_begin`` / ``imt_decode_step``).  Beam re-ordering never moves the cache: a slot
    table maps (hypothesis, position) to the cache row of the ancestor that produced it.
  * log-softmax, EOS / length-limit zeroing, length penalty, top-k over beam*V, the PAD overwrites and the
    gather/cat bookkeeping (``:193-227``) are one on-device call (``imt_beam_step``); the host only checks the
    "every hypothesis has EOS" stop condition (``:134-136``) every ``sync_every`` steps.
  * ``kv_cache=False`` keeps the reference's literal per-step recomputation (on the HIP decoder) -- used by the
    tests to show both modes produce the same tokens.
  * ``objects=`` (build extension, ImageCaptioning with ``use_obj``: pre-extracted detector output ``{"feats", "boxes", "labels"}``
    in place of the frozen Faster-RCNN, see image_model) and ``src_inputs=`` together with ``images=`` on an ``ImageMassSeq2Seq``
    (``:105-106``) give every step a second stream, mixed into the first through a sigmoid gate before the projection:
    ``decoder_streams`` says which stack reads what with which key mask.  With ``kv_cache`` each stream has an incremental
    decoder of its own (cross K/V, workspace, self cache; the slot table is shared).
  * ``sampling=True`` (build extension, the reference only searches): the same loop with ``imt_sample_step`` in place of
    ``imt_beam_step`` -- ``nsamples`` hypotheses per sentence, each extended by one token DRAWN from softmax(logits / temperature)
    over the ``sampling_topk`` best tokens (0: the whole vocabulary); ``last_scores`` holds the model's own log-probabilities.
Ties between equal scores (``torch.topk`` leaves them unspecified, and ``:194-196`` creates them on purpose) are
broken towards the lowest flat index.  ``:216`` is taken as floor division (torch 1.4 semantics).
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib as L
from . import hip_ops as O
from .param_store import store_of
from .seq2seq import DecoderStream, unwrap


def get_outputs_until_eos(eos, outputs, size_limit=None, remove_first_token: bool = False):
    """Rows of ``outputs`` cut before their first ``eos`` (rows without one: cut at ``size_limit[r]``)."""
    if outputs.dim() == 1:
        outputs = outputs.unsqueeze(0)
    outputs = outputs.cpu()
    is_eos = outputs == eos
    has = is_eos.any(dim=1)
    first = is_eos.to(torch.int8).argmax(dim=1)
    begin = 1 if remove_first_token else 0
    cut = []
    for r in range(outputs.size(0)):
        end = int(first[r]) if bool(has[r]) else (outputs.size(1) if size_limit is None else int(size_limit[r]))
        cut.append(outputs[r, begin:end])
    return cut


class _SearchState:
    """Device-resident state of one search (all sizes fixed up front: r_max = B*width rows), seeded with the first tokens.  The
    buffers named in ``pingpong`` come in pairs: a step reads side ``cur`` and writes the other.  ``args``: the step's args
    struct with the sizes and this state's fixed pointers."""

    def __init__(self, args, first_tokens, eos, width, t_max, use_slots):
        B, device = first_tokens.numel(), first_tokens.device
        r = B * width
        i64, i32, f32, u8 = torch.int64, torch.int32, torch.float32, torch.uint8
        self.zeros = z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=device)
        self.B, self.beam, self.t_max = B, width, t_max
        self.hist = [z(r, t_max, dtype=i64), z(r, t_max, dtype=i64)]
        self.slots = [z(r, t_max, dtype=i32), z(r, t_max, dtype=i32)] if use_slots else [None, None]
        self.scores = [z(r, dtype=f32), z(r, dtype=f32)]
        self.eos = [z(r, dtype=u8), z(r, dtype=u8)]
        self.parent, self.tokens, self.eos_count = z(r, dtype=i32), z(r, dtype=i64), z(t_max, dtype=i32)
        self.pingpong = ["hist", "slots", "scores", "eos"]
        self.cur = 0
        self.hist[0][:B, 0] = first_tokens
        self.eos[0][:B] = (first_tokens == eos).to(u8)
        if use_slots:
            self.slots[0][:B, 0] = torch.arange(B, dtype=i32, device=device)
        self.args = a = args
        a.B, a.t_max = B, t_max
        a.parent_out, a.tokens_out, a.eos_count = self.parent.data_ptr(), self.tokens.data_ptr(), self.eos_count.data_ptr()

    def bind_step(self, rep, step):
        """``args`` for one step: it reads side ``cur`` and writes the other."""
        a = self.args
        a.rep, a.step = rep, step
        for name in self.pingpong:
            src, dst = getattr(self, name)[self.cur], getattr(self, name)[self.cur ^ 1]
            setattr(a, name + "_in", None if src is None else src.data_ptr())
            setattr(a, name + "_out", None if dst is None else dst.data_ptr())
        return a

    def best(self, n_cols):
        """The first hypothesis of every sentence, ``n_cols`` columns (1: no step ran, still one row per sentence)."""
        hist = self.hist[self.cur]
        return hist[:self.B, :1] if n_cols == 1 else hist.view(self.B, self.beam, self.t_max)[:, 0, :n_cols]


class _BeamState(_SearchState):
    """The state ``imt_beam_step`` drives (``args``: a ``BeamArgs``): the hypothesis sizes of the length penalty and the candidate
    workspace on top."""

    def __init__(self, first_tokens, eos, beam, t_max, use_slots):
        super().__init__(L.BeamArgs(), first_tokens, eos, beam, t_max, use_slots)
        r, z = self.B * beam, self.zeros
        self.sizes = [z(r, dtype=torch.float32), z(r, dtype=torch.float32)]
        self.pingpong.append("sizes")
        self.cand_scores, self.cand_idx = z(r, beam, dtype=torch.float32), z(r, beam, dtype=torch.int32)
        a = self.args
        a.beam, a.cand_scores, a.cand_idx = beam, self.cand_scores.data_ptr(), self.cand_idx.data_ptr()


class _SampleState(_SearchState):
    """The state ``imt_sample_step`` drives (``args``: a ``SampleArgs``), ``nsamples`` hypotheses per sentence (``beam``)."""

    def __init__(self, first_tokens, eos, nsamples, t_max, use_slots, temperature, topk, seed):
        super().__init__(L.SampleArgs(), first_tokens, eos, nsamples, t_max, use_slots)
        a = self.args
        a.n, a.temperature, a.topk, a.seed = nsamples, float(temperature), int(topk), int(seed)

    def all_rows(self, n_cols):
        """Every hypothesis, sentence-major (sample k of sentence b in row b * nsamples + k), ``n_cols`` columns."""
        return self.hist[self.cur][:, :n_cols]


_SEED_STRIDE = 0x9E3779B97F4A7C15  # search number c of a sampling decoder draws with seed + c * stride (mod 2^64)


def add_sampling_options(parser):
    """--sampling / --sampling-topk / --temperature / --nsamples / --seed of the generation entry points (optparse)."""
    parser.add_option("--sampling", action="store_true", dest="sampling", default=False,
                      help="draw from the model instead of searching it")
    parser.add_option("--sampling-topk", dest="sampling_topk", type="int", default=0, help="draw among the K best tokens (0: all)")
    parser.add_option("--temperature", dest="temperature", type="float", default=1.0)
    parser.add_option("--nsamples", dest="nsamples", type="int", default=1, help="samples per input (output line i*N + k)")
    parser.add_option("--seed", dest="seed", type="int", default=1234)
    return parser


def sampling_kwargs(options):
    """The ``BeamDecoder`` keywords of ``add_sampling_options``' flags."""
    return dict(sampling=options.sampling, sampling_topk=options.sampling_topk, temperature=options.temperature,
                nsamples=options.nsamples, seed=options.seed)


def length_limits(max_len, max_len_a, max_len_b, max_pos, batch_size, src_len=None, src_sizes=None, images=False):
    """(max_len, per-sentence limits, t_max) of one search -- pure host arithmetic (src/seq_gen.py:86-91,113-121).
    ``max_len`` None: 512 when ``images`` are given (:90-91), else the limit of the source width ``src_len`` (:116-117).  With a
    source (``src_len`` not None) sentence b may grow to min(int(max_len_a * src_sizes[b] + max_len_b), max_pos) tokens (:113-114,
    :121); without one every sentence gets ``max_len`` (:118-119).  ``t_max`` >= 2: the first token and one step always fit."""
    limit = lambda s: min(int(max_len_a * s + max_len_b), max_pos)
    if max_len is None:
        max_len = 512 if images else limit(src_len)
    max_lens = [max_len] * batch_size if src_len is None else [limit(int(s)) for s in src_sizes]
    return max_len, max_lens, max(int(max_len), 2)


def decoder_streams(model, batch_lang, text=None, text_mask=None, image=None, objects=None):
    """The ``DecoderStream``s one search step decodes, from already-encoded tensors (no kernel runs here):
      text                 the language's decoder over ``text`` with the source mask (src/seq_gen.py:163-166);
      text + image         and the SAME decoder over ``image`` with no key mask, mixed through multimodal_attention_gate (:181-188);
      caption              the decoder over ``image`` (from ``images`` or ``image_embed``), no key mask (:152-154,164-166);
      caption + objects    and ``obj_decoder`` over ``objects``, no key mask, mixed through multistream_attention_gate (:167-179)."""
    decoder = model._decoder_for(batch_lang)
    if text is not None:
        streams = [DecoderStream(decoder, text, text_mask, None)]
        if image is not None:
            streams.append(DecoderStream(decoder, image, None, model.multimodal_attention_gate))
        return streams
    streams = [DecoderStream(decoder, image, None, None)]
    if objects is not None:
        streams.append(DecoderStream(model._obj_decoder_for(batch_lang), objects, None, model.multistream_attention_gate))
    return streams


def _mixed(out, states, gate):
    """``states`` of a further stream mixed into ``out`` through its gate (the first stream: ``states`` as they are)."""
    return states if out is None else O.gated_mix(out.contiguous(), states.contiguous(), gate)


class _CachedSteps:
    """Step provider of ``kv_cache=True``: per stream an ``_Incremental`` (cross K/V, self cache, workspace) and a hidden buffer;
    a step decodes one position per hypothesis.  The slot table of ``st`` is shared by the streams."""

    def __init__(self, streams, gates, st, first_tokens, type_rows, store, dtype, flat):
        lib, cu_stream = L.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.st, self.first_tokens, self.type_rows, self.gates = st, first_tokens, type_rows, gates
        self.incs = [_Incremental(lib, s.decoder, store, dtype, flat, s.states, s.key_mask, st.B, st.beam, st.t_max, cu_stream)
                     for s in streams]
        self.hidden = [torch.empty((st.B * st.beam, s.states.size(-1)), dtype=dtype, device=s.states.device) for s in streams]

    def states(self, i, rep):
        """[B * rep, d] decoder states of step ``i`` (position i - 1)."""
        st, rows = self.st, self.st.B * rep
        ids, types = (self.first_tokens if i == 1 else st.tokens), self.type_rows[rep > 1]
        out = None
        for inc, hidden, gate in zip(self.incs, self.hidden, self.gates):
            inc.step(i - 1, rows, rep, ids, types, st.slots[st.cur], hidden)
            out = _mixed(out, hidden[:rows], gate)
        return out

    def finish(self):
        """Raises if a one-launch decoder step was abandoned (bounded waits); synchronises, the outputs are read next anyway."""
        for inc in reversed(self.incs):
            inc.check()


class _RecomputedSteps:
    """Step provider of ``kv_cache=False``: every stream's decoder over the whole prefix at every step, the reference's literal
    recomputation (src/seq_gen.py:146-188)."""

    def __init__(self, streams, gates, st, type_rows):
        self.streams, self.gates, self.st, self.type_rows = streams, gates, st, type_rows

    def states(self, i, rep):
        """[B * rep, d] decoder states of step ``i``: the last position of the prefix."""
        prefix = self.st.hist[self.st.cur][:self.st.B * rep, :i].contiguous()
        types = self.type_rows[rep > 1].unsqueeze(-1).expand(-1, i)
        out = None
        for s, gate in zip(self.streams, self.gates):
            enc = s.states if rep == 1 else torch.repeat_interleave(s.states, rep, 0)
            mask = s.key_mask if rep == 1 or s.key_mask is None else torch.repeat_interleave(s.key_mask, rep, 0)
            last = s.decoder(encoder_states=enc, input_ids=prefix, encoder_attention_mask=mask,
                             tgt_attention_mask=torch.ones_like(prefix), token_type_ids=types)[:, -1, :]
            out = _mixed(out, last, gate)
        return out

    def finish(self):
        pass


class BeamDecoder(nn.Module):
    def __init__(self, seq2seq_model, beam_width: int = 5, max_len_a: float = 1.1, max_len_b: int = 5,
                 len_penalty_ratio: float = 0.8, *, kv_cache: bool = True, sync_every: int = 8, sampling: bool = False,
                 sampling_topk: int = 0, temperature: float = 1.0, nsamples: int = 1, seed: int = 1234):
        super(BeamDecoder, self).__init__()
        self.seq2seq_model = seq2seq_model
        self.beam_width = beam_width
        self.max_len_a = max_len_a
        self.max_len_b = max_len_b
        self.len_penalty_ratio = len_penalty_ratio
        self.kv_cache = kv_cache
        self.sync_every = max(1, int(sync_every))
        self.sampling, self.sampling_topk, self.temperature = bool(sampling), int(sampling_topk), float(temperature)
        self.nsamples, self.seed = int(nsamples), int(seed)
        if self.sampling:
            if not 1 <= self.nsamples <= 32:
                raise ValueError("nsamples must be in 1..32, got %d" % self.nsamples)
            if not (0.0 < self.temperature < float("inf")):
                raise ValueError("temperature must be positive and finite, got %r" % (temperature,))
        self.searches = 0        # sampled searches run so far: each draws with a seed of its own
        self.last_scores = None  # sampling: [B, nsamples] fp32 summed model log-probabilities of the last search (CPU)

    def len_penalty(self, lengths: torch.Tensor):
        """GNMT length penalty (https://arxiv.org/abs/1609.08144 section 7); the search itself evaluates it on device."""
        return torch.pow((lengths + 6.0) / 6.0, self.len_penalty_ratio).unsqueeze(-1)

    # ---------------------------------------------------------------- one search
    @torch.no_grad()
    def forward(self, src_inputs=None, src_sizes=None, first_tokens=None, src_mask=None, src_langs=None, tgt_langs=None,
                pad_idx=None, max_len: int = None, unpad_output: bool = True, beam_width: int = None, images=None,
                proposals=None, image_embed=None, objects=None):
        # ---- arguments
        (src_inputs, src_sizes, first_tokens, src_mask, src_langs, tgt_langs, images, proposals, image_embed, objects) = map(
            unwrap, (src_inputs, src_sizes, first_tokens, src_mask, src_langs, tgt_langs, images, proposals, image_embed, objects))
        model = self.seq2seq_model.module if hasattr(self.seq2seq_model, "module") else self.seq2seq_model
        beam = int(self.beam_width if beam_width is None else beam_width)
        if self.sampling:
            if beam_width is not None and int(beam_width) != 1:
                raise ValueError("a sampling BeamDecoder has no beam: beam_width must be None or 1, got %r" % (beam_width,))
            beam = self.nsamples  # the width of the search state
        if pad_idx is None:
            pad_idx = model.text_processor.pad_token_id()
        device = model._device
        if device.type != "cuda":
            raise L.ImtError("imagetranslate_amd: beam search needs the model on the GPU (no CPU fallback)")
        given = [x for x in (src_inputs, images, image_embed) if x is not None]
        if not given:
            raise ValueError("BeamDecoder needs src_inputs, images or image_embed")
        B, batch_lang = given[0].size(0), int(tgt_langs[0])
        eos, V = model.text_processor.sep_token_id(), model.config.vocab_size
        max_len, max_lens_host, t_max = length_limits(
            max_len, self.max_len_a, self.max_len_b, model.encoder.embeddings.position_embeddings.num_embeddings, B,
            src_len=None if src_inputs is None else src_inputs.size(1), src_sizes=src_sizes, images=images is not None)

        # ---- encoder side, once per search
        streams = self._encode(model, batch_lang, B, src_inputs, src_mask, src_langs, images, image_embed, objects)
        dtype, output_layer = model._imt_compute_dtype, model._output_layer(batch_lang)
        store = store_of(streams[0].decoder).ensure()
        flat = store.params_for(dtype)  # the whole buffer as well: the incremental decoders' descriptors point at it
        W, bias, *gates = store.views(dtype, output_layer.layer.weight, output_layer.layer.bias, *(s.gate for s in streams), flat=flat)
        gates = [None if g is None else g.view(-1) for g in gates]

        # ---- search state and step provider
        first_tokens = first_tokens.to(device=device, dtype=torch.int64).contiguous()
        if self.sampling:
            if B * beam * V >= 1 << 32:
                raise ValueError("sampling: batch * nsamples * vocabulary = %d * %d * %d does not fit the 32-bit noise index"
                                 % (B, beam, V))
            st = _SampleState(first_tokens, eos, beam, t_max, self.kv_cache, self.temperature, self.sampling_topk,
                              (self.seed + self.searches * _SEED_STRIDE) % (1 << 64))
            self.searches += 1
        else:
            st = _BeamState(first_tokens, eos, beam, t_max, self.kv_cache)
        langs = tgt_langs.to(device=device, dtype=torch.int64)
        type_rows = [langs.contiguous(), torch.repeat_interleave(langs, beam, 0).contiguous()]  # [rep == 1, rep == beam]
        if self.kv_cache:
            steps = _CachedSteps(streams, gates, st, first_tokens, type_rows, store, dtype, flat)
        else:
            steps = _RecomputedSteps(streams, gates, st, type_rows)
        logits = O.alloc_rows(B * beam, V, torch.float32, device)  # leading dimension padded to 8 for odd vocabularies
        max_lens = torch.tensor(max_lens_host, dtype=torch.int64).to(device)
        a = st.args  # the rest of what no step changes
        a.V, a.logits, a.ld, a.max_lens = V, logits.data_ptr(), logits.stride(0), max_lens.data_ptr()
        a.pad_idx, a.eos = int(pad_idx), int(eos)
        if not self.sampling:
            a.len_penalty_ratio = float(self.len_penalty_ratio)

        def project(states, rep):  # [B * rep, d] states -> logits[:B * rep]
            if model.use_proposals:
                states = model.attend_proposal(states.contiguous(), proposals, pad_idx, rows_per_group=rep)
            O.gemm(states.contiguous(), W, O.IMT_NT, bias=bias, out=logits[:B * rep])

        nothing_to_decode = beam == 1 and bool((first_tokens == eos).all())
        n_cols = 1 if nothing_to_decode else self._search(steps, project, st, max_len)
        steps.finish()
        object_gate = getattr(model, "multistream_attention_gate", None)
        if any(s.gate is object_gate for s in streams[1:]):  # an object stream: its labels may have been device tensors
            model.image_model.check_object_labels(wait=True)  # the search has synchronised anyway

        # ---- outputs
        if self.sampling:
            self.last_scores = st.scores[st.cur].view(B, beam).cpu()
            if beam > 1:  # every sample, sentence-major (a search without a step is a single sample per sentence: below)
                rows = st.all_rows(n_cols) if n_cols > 1 else torch.repeat_interleave(st.best(1), beam, 0)  # (no step ran)
                if unpad_output:
                    return get_outputs_until_eos(eos, rows, size_limit=[m for m in max_lens_host for _ in range(beam)])
                return list(rows.cpu())
        if unpad_output:
            return get_outputs_until_eos(eos, st.best(n_cols), size_limit=max_lens_host)
        return list(st.best(n_cols).cpu())

    @staticmethod
    def _encode(model, batch_lang, B, src_inputs, src_mask, src_langs, images, image_embed, objects):
        """The encoder side of one search (src/seq_gen.py:93-106) as ``decoder_streams``: states in the compute dtype, the source
        mask as uint8.  ``src_inputs`` with ``images``: text + image (``image_embed``, when given as well, replaces the image
        head's output); ``src_inputs`` without ``images``: the text search, whatever ``image_embed`` is (:94)."""
        device, dtype = model._device, model._imt_compute_dtype
        ready = lambda t: None if t is None else t.to(device).to(dtype).contiguous()
        if src_inputs is None:
            if image_embed is None:
                image, obj_fc = model.encode(images=images.to(device), **({"objects": objects} if objects is not None else {}))
            else:
                image, obj_fc = image_embed, None
                if objects is not None and "obj_decoder" in model._modules:
                    obj_fc = model.image_model.objects_forward(objects, dtype)
            return decoder_streams(model, batch_lang, image=ready(image), objects=ready(obj_fc))
        src_mask = src_mask.to(device)
        text = model.encode(src_inputs, src_mask, src_langs.unsqueeze(-1).expand(-1, src_inputs.size(-1)))[0]
        image = None
        if images is not None:  # a source sentence AND an image (:105-106): the decoder also attends to the regions
            if not hasattr(model, "multimodal_attention_gate"):
                raise ValueError("text + image beam search needs an ImageMassSeq2Seq (multimodal_attention_gate)")
            image = image_embed if image_embed is not None else model.image_model(images.to(device), dtype)[0]  # element 0, DESIGN.md
            if image.size(0) != B:
                raise ValueError("text + image beam search: %d images for %d sentences" % (image.size(0), B))
        return decoder_streams(model, batch_lang, text=ready(text), text_mask=src_mask.to(torch.uint8).contiguous(), image=ready(image))

    def _search(self, steps, project, st, max_len):
        """The search loop: ``steps.states`` -> ``project`` -> ``imt_beam_step`` (sampling: ``imt_sample_step``) per step; ``st.args``
        holds everything that no step changes.  Returns the number of columns of the history that hold the result (1: no step ran)."""
        advance = O.sample_step if self.sampling else O.beam_step
        for i in range(1, max_len):
            rep = 1 if i == 1 else st.beam
            project(steps.states(i, rep), rep)
            advance(st.bind_step(rep, i))
            st.cur ^= 1
            # stop condition (:134-136), looked at every `sync_every` steps; columns decoded past it are dropped
            if i % self.sync_every == 0 or i == max_len - 1:
                full = (st.eos_count[1:i + 1] == st.B * st.beam).nonzero()
                if full.numel() > 0:
                    return int(full[0, 0]) + 2
        return max(1, max_len)


class _Incremental:
    """Owns the caches of one search and issues imt_decode_begin / imt_decode_step."""

    def __init__(self, lib, decoder, store, dtype, flat, encoder_states, enc_mask, B, beam, t_max, stream):
        self.lib, self.stream = lib, stream
        desc, self._keep = decoder._desc(store, dtype)
        desc.params = flat.data_ptr()
        desc.grads = None
        self.desc = desc
        self.flat = flat
        dev = encoder_states.device
        self.B, self.r_max, self.t_max, self.Tk = B, B * beam, t_max, encoder_states.size(1)
        nbytes = lambda n, what: self._positive(n, what)
        self.ws_bytes = nbytes(lib.imt_decode_workspace_bytes(ctypes.byref(desc), self.r_max), "imt_decode_workspace_bytes")
        # zeros: the sticky status word of the one-launch step (read by check()) is clean even if the search issues no step
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.cache = torch.empty(nbytes(lib.imt_decode_self_cache_bytes(ctypes.byref(desc), self.r_max, t_max),
                                        "imt_decode_self_cache_bytes"), dtype=torch.uint8, device=dev)
        self.cross = torch.empty(nbytes(lib.imt_decode_cross_bytes(ctypes.byref(desc), B, self.Tk), "imt_decode_cross_bytes"),
                                 dtype=torch.uint8, device=dev)
        self.enc_mask = enc_mask
        self.pos_table = torch.arange(t_max, dtype=torch.int64, device=dev).unsqueeze(1).expand(t_max, self.r_max).contiguous()
        L.check(lib.imt_decode_begin(ctypes.byref(desc), ctypes.c_void_p(encoder_states.data_ptr()), B, self.Tk,
                                     ctypes.c_void_p(self.cross.data_ptr()), stream), "imt_decode_begin")

    @staticmethod
    def _positive(n, what):
        if n <= 0:
            raise L.ImtError("%s failed" % what)
        return n

    def step(self, pos, rows, rep, ids, type_ids, slots, out):
        io = L.DecodeIO()
        io.R, io.rep, io.pos, io.Tk, io.t_max, io.r_max = rows, rep, pos, self.Tk, self.t_max, self.r_max
        io.ids, io.type_ids, io.pos_ids = ids.data_ptr(), type_ids.data_ptr(), self.pos_table[pos].data_ptr()
        io.slots = slots.data_ptr()
        io.enc_mask = self.enc_mask.data_ptr() if self.enc_mask is not None else None
        io.self_cache, io.cross_kv, io.out = self.cache.data_ptr(), self.cross.data_ptr(), out.data_ptr()
        L.check(self.lib.imt_decode_step(ctypes.byref(self.desc), ctypes.byref(io), ctypes.c_void_p(self.ws.data_ptr()),
                                         self.ws_bytes, self.stream), "imt_decode_step")

    def check(self):
        """End of a search: did every one-launch step run to its end (include/imt_hip.h: imt_decode_check)?  Synchronises."""
        L.check(self.lib.imt_decode_check(ctypes.byref(self.desc), self.r_max, ctypes.c_void_p(self.ws.data_ptr()), self.stream),
                "imt_decode_check")
