"""CPU tests of the scorer: the test oracle pinned by a second route, host-side argument validation of imt_score_rows,
the option table of the entry point, and the packing / window logic of score_pairs (no GPU anywhere)."""
import ctypes
import json
import os
import random

import torch

from oracle import reference_model as R
from tests.score_oracle import oracle_scores

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = dict(enc_layer=2, dec_layer=2, embed_dim=128, intermediate_dim=512, num_attention_heads=4)


def toy_batch(B=6, S=14, T=12, V=1000, seed=3):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(7, V, (B, S), generator=g)
    tgt = torch.randint(7, V, (B, T), generator=g)
    src[:, 0], tgt[:, 0] = 5, 6
    slen = torch.randint(4, S + 1, (B,), generator=g)
    tlen = torch.randint(3, T + 1, (B,), generator=g)
    slen[0], tlen[0] = S, T
    for b in range(B):
        src[b, slen[b] - 1], tgt[b, tlen[b] - 1] = 4, 4
        src[b, slen[b]:], tgt[b, tlen[b]:] = 0, 0
    return (src, tgt, src != 0, tgt != 0, torch.zeros(B, dtype=torch.long), torch.ones(B, dtype=torch.long))


def test_oracle_equals_gather_from_forward_log_softmax():
    """tests/score_oracle.py (decoder on the full padded grid) against a second route through the oracle model: gather the
    targets from forward(log_softmax=True)'s non-pad rows and average per sentence.  Same fp32 operations on a different
    row set: equal within 1e-5 of the largest |score|."""
    from tests.util import beam_state_dict
    for lang_dec in (False, True):
        torch.manual_seed(11)
        ref = R.Seq2Seq(R.SyntheticTextProcessor(1000), lang_dec=lang_dec, **TOY).eval()
        ref.load_state_dict(beam_state_dict(ref.state_dict()))
        args = toy_batch()
        for normalize in (True, False):
            scores, tok_lp = oracle_scores(ref, *args, normalize=normalize, rows_per_block=4)
            with torch.no_grad():
                lp = ref(*args, log_softmax=True)
            mask = args[3][:, 1:]
            picked = lp.gather(1, args[1][:, 1:][mask].unsqueeze(1)).squeeze(1)
            counts = mask.sum(1)
            want = torch.stack([c.sum() for c in picked.split(counts.tolist())])
            if normalize:
                want = want / counts
            assert float((scores - want).abs().max()) <= 1e-5 * float(want.abs().max()), (scores, want)
            assert float((tok_lp[mask] - picked).abs().max()) <= 1e-5 * float(picked.abs().max())
            assert float(tok_lp[~mask].abs().max()) == 0.0


def _args(lib, L, **kw):
    """A complete, valid argument block with fake (never dereferenced) device addresses; kw overrides fields."""
    a = L.ScoreArgs()
    a.dtype, a.N, a.V, a.K = L.IMT_BF16, 300, 1000, 512
    a.x, a.ldx, a.w, a.ldw = 0x10000, 512, 0x20000, 512
    a.bias, a.target, a.logprob, a.lse = 0x30000, 0x40000, 0x50000, 0x60000
    a.ws, a.ws_bytes = 0x70000, lib.imt_score_ws_bytes(300, 1000)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_score_rows_refuses_bad_arguments_before_any_launch():
    from imagetranslate_amd import _lib as L
    lib = L.load()
    cases = [(dict(dtype=7), b"dtype"), (dict(x=None), b" x is null"), (dict(w=None), b" w is null"), (dict(target=None), b" target is null"),
             (dict(logprob=None), b" logprob is null"), (dict(N=0), b" N = 0"), (dict(V=-3), b" V = -3"), (dict(K=0), b" K = 0"),
             (dict(ws_bytes=lib.imt_score_ws_bytes(300, 1000) - 1), b"ws_bytes"), (dict(ws=None), b"ws_bytes"),
             (dict(K=520, ldx=520, ldw=520), b"K 520"), (dict(dtype=L.IMT_F32, K=48, ldx=48, ldw=48), b"K 48")]
    for kw, name in cases:
        assert lib.imt_score_rows(ctypes.byref(_args(lib, L, **kw)), None) == -1, kw
        msg = lib.imt_last_error()
        assert msg.startswith(b"score_rows:") and name in msg, (kw, msg)
    assert lib.imt_score_rows(None, None) == -1
    # segments need their output
    a = _args(lib, L, seg_offsets=0x80000, n_seg=4)
    assert lib.imt_score_rows(ctypes.byref(a), None) == -1 and b"seg_score" in lib.imt_last_error()


def test_score_supported_and_workspace_size():
    from imagetranslate_amd import _lib as L
    lib = L.load()
    assert lib.imt_abi_sizeof(b"imt_score_args") == ctypes.sizeof(L.ScoreArgs)
    for K in (512, 768, 64):
        assert lib.imt_score_supported(L.IMT_BF16, 30000, K) == 1
        assert lib.imt_score_supported(L.IMT_F32, 30000, K) == 1
    assert lib.imt_score_supported(L.IMT_BF16, 30000, 32) == 0    # half a bf16 K tile
    assert lib.imt_score_supported(L.IMT_F32, 1000, 32) == 1
    assert lib.imt_score_supported(L.IMT_BF16, 1000, 520) == 0
    assert lib.imt_score_supported(3, 1000, 512) == 0 and lib.imt_score_supported(L.IMT_BF16, 0, 512) == 0
    # one float per row (the target's logit) + one float2 per (row, 256-column tile)
    for N, V in ((1, 250), (37, 1000), (8128, 30000)):
        tiles = (V + 255) // 256
        assert lib.imt_score_ws_bytes(N, V) >= 4 * N + 8 * N * tiles
        assert lib.imt_score_ws_bytes(N, V) <= 4 * N + 8 * N * tiles + 256
        assert lib.imt_score_ws_bytes(N + 1, V) > lib.imt_score_ws_bytes(N, V)
        assert lib.imt_score_ws_bytes(N, V + 256) > lib.imt_score_ws_bytes(N, V)
    assert lib.imt_score_ws_bytes(8128, 30000) == 8128 * 4 + 118 * 8128 * 8


def test_option_table_matches_the_reference_flags():
    """Names, destinations, types and defaults of src/score_pairs.py:15-27 (tests/golden/score_options_kat.json) + --fp32."""
    from imagetranslate_amd.score_pairs import get_option_parser
    with open(os.path.join(GOLD, "score_options_kat.json")) as fp:
        want = [tuple(r) for r in json.load(fp)]
    parser = get_option_parser()
    got = []
    for o in parser.option_list:
        if o.dest is None or o.get_opt_string() == "--help":
            continue
        kind = "flag" if o.action == "store_true" else {"string": "str"}.get(o.type, o.type)
        got.append((o.get_opt_string(), o.dest, kind, parser.defaults.get(o.dest)))
    assert got == want + [("--fp32", "fp32", "flag", False)]
    opts, _ = parser.parse_args(["--capacity", "7", "--resume", "3", "--end", "9", "--fp16"])
    assert (opts.total_capacity, opts.resume_index, opts.end_index, opts.fp16, opts.fp32) == (7, 3, 9, True, False)


def _synthetic_table(n_src=40, seed=0):
    rnd = random.Random(seed)
    entries, tid = [], 1000
    for sid in range(n_src):
        n_c = rnd.randint(1, 9)
        s_len = rnd.choice([4, 9, 20, 60, 200])
        lang = rnd.randint(0, 1)
        tids, cands, langs = [], [], []
        for _ in range(n_c):
            tid += 1
            tids.append(tid)
            cands.append([7] * rnd.randint(2, 2 * s_len))
            langs.append(1 - lang if rnd.random() < 0.8 else lang)   # mixed target languages inside one source too
        entries.append((sid, [7] * s_len, lang, tids, cands, langs))
    return entries


def test_packing_covers_every_pair_once_within_the_capacity():
    from imagetranslate_amd.score_pairs import decoder_calls, make_packs, work_estimate
    entries = _synthetic_table()
    for cap in (10 ** 5, 3 * 10 ** 6, 10 ** 9):
        packs = list(make_packs(iter(entries), cap))
        seen = []
        multi = 0
        for pack in packs:
            est = sum(work_estimate(len(p[1]), max(len(c) for c in p[4]), len(p[3])) for p in pack)
            assert est <= cap or len(pack) == 1, "a pack over the cap must be one (split) source"
            if est > cap:
                assert len(pack[0][3]) == 1, "a split source over the cap is down to single candidates"
            multi += len(pack) > 1
            calls = decoder_calls(pack)
            for lang, rows in calls.items():
                for k, tid, ids in rows:
                    sid, _, _, tids, cands, langs = pack[k]
                    j = tids.index(tid)
                    assert langs[j] == lang and cands[j] is ids, "one target language per decoder call"
                    seen.append((sid, tid))
            assert sum(len(r) for r in calls.values()) == sum(len(p[3]) for p in pack)
        want = [(e[0], t) for e in entries for t in e[3]]
        assert sorted(seen) == sorted(want) and len(seen) == len(set(seen)), "every (source, candidate) exactly once"
        assert [s for s, _ in seen if True][0] == 0  # table order kept
        if cap == 10 ** 9:
            assert multi >= 1 and len(packs) < len(entries), "sources are packed together under a generous cap"
    # a source over the cap splits as the reference does: ceil(est / cap) parts of floor(n / parts) candidates
    big = (0, [7] * 100, 0, list(range(8)), [[7] * 100] * 8, [1] * 8)
    est = work_estimate(100, 100, 8)
    packs = list(make_packs(iter([big]), est // 3 + 1))
    assert [len(p[0][3]) for p in packs] == [2, 2, 2, 2] and all(len(p) == 1 for p in packs)


def test_resume_end_window():
    from imagetranslate_amd.score_pairs import window
    table = {sid: [sid + 100] for sid in range(10, 22)}    # 12 sources, insertion order
    assert list(window(table)) == list(range(10, 22))
    assert list(window(table, 3, 9)) == [13, 14, 15, 16, 17]   # 1-based: indices 4..8
    assert list(window(table, 0, 1)) == [] and list(window(table, 11, -1)) == [21]
    assert list(window(table, 0, 0)) == list(range(10, 22))    # end <= 0: no end
