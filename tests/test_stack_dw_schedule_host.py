"""Where imt_stack_backward sends the weight-gradient launch of each layer (csrc/model.hip DwPlan, through the host-only entry
point imt_stack_dw_schedule), WITHOUT a GPU.

The rules, as the layer loop applied them before they became an object of their own (layers l = layer_hi - 1 .. layer_lo):
  * pairs and the side stream only when the call covers a whole stack of at least two layers;
  * before layer l writes scratch set l % 4, wait for done[l + 4] if the side stream is on and l + 4 < layer_hi;
  * hold layer l's products for the layer below if nothing is held, l > layer_lo and they are pairable; otherwise launch them,
    with the held layer's if there is one, on the side stream (recording done[l] and done[held]) or on the main stream;
  * at the end wait for done of the last side launch.
The expected records below are written out from these rules by hand; the second half checks what the scheme is for."""
import itertools

import pytest

from imagetranslate_amd import hip_ops as O

H, M, S = O.DW_HOLD, O.DW_FLUSH_MAIN, O.DW_FLUSH_SIDE


def plan(n, pairable=True, side=True, lo=0, hi=None):
    pairable = [pairable] * n if isinstance(pairable, bool) else pairable
    return O.stack_dw_schedule(n, lo, n if hi is None else hi, side, pairable)


# (layer, wait_done, action, with_held) per layer, and the layer whose done the call ends on
ALL_PAIRABLE = {
    1: ([(0, -1, M, -1)], -1),                                                        # never side, never held
    2: ([(1, -1, H, -1), (0, -1, S, 1)], 0),
    3: ([(2, -1, H, -1), (1, -1, S, 2), (0, -1, S, -1)], 0),                          # a pair, then layer 0 alone
    5: ([(4, -1, H, -1), (3, -1, S, 4), (2, -1, H, -1), (1, -1, S, 2), (0, 4, S, -1)], 0),
    6: ([(5, -1, H, -1), (4, -1, S, 5), (3, -1, H, -1), (2, -1, S, 3), (1, 5, H, -1), (0, 4, S, 1)], 0),
}
NONE_PAIRABLE = {
    1: ([(0, -1, M, -1)], -1),
    2: ([(1, -1, S, -1), (0, -1, S, -1)], 0),
    3: ([(2, -1, S, -1), (1, -1, S, -1), (0, -1, S, -1)], 0),
    5: ([(4, -1, S, -1), (3, -1, S, -1), (2, -1, S, -1), (1, -1, S, -1), (0, 4, S, -1)], 0),
    6: ([(5, -1, S, -1), (4, -1, S, -1), (3, -1, S, -1), (2, -1, S, -1), (1, 5, S, -1), (0, 4, S, -1)], 0),
}
TOP_UNPAIRABLE = {
    2: ([(1, -1, S, -1), (0, -1, S, -1)], 0),                                         # layer 0 is never held
    3: ([(2, -1, S, -1), (1, -1, H, -1), (0, -1, S, 1)], 0),
    5: ([(4, -1, S, -1), (3, -1, H, -1), (2, -1, S, 3), (1, -1, H, -1), (0, 4, S, 1)], 0),
    6: ([(5, -1, S, -1), (4, -1, H, -1), (3, -1, S, 4), (2, -1, H, -1), (1, 5, S, 2), (0, 4, S, -1)], 0),
}
SIDE_OFF = {
    1: ([(0, -1, M, -1)], -1),
    2: ([(1, -1, H, -1), (0, -1, M, 1)], -1),
    3: ([(2, -1, H, -1), (1, -1, M, 2), (0, -1, M, -1)], -1),
    5: ([(4, -1, H, -1), (3, -1, M, 4), (2, -1, H, -1), (1, -1, M, 2), (0, -1, M, -1)], -1),
    6: ([(5, -1, H, -1), (4, -1, M, 5), (3, -1, H, -1), (2, -1, M, 3), (1, -1, H, -1), (0, -1, M, 1)], -1),
}


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6])
def test_records_of_whole_stack_calls(n):
    assert plan(n) == ALL_PAIRABLE[n]
    assert plan(n, pairable=False) == NONE_PAIRABLE[n]
    assert plan(n, side=False) == SIDE_OFF[n]
    if n in TOP_UNPAIRABLE:
        assert plan(n, pairable=[True] * (n - 1) + [False]) == TOP_UNPAIRABLE[n]


@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_per_layer_segment_calls_stay_on_the_main_stream(n):
    """A data-parallel run calls (l, l + 1): main stream, nothing held, no wait -- whatever the side stream and the tiles say."""
    for l in range(n):
        assert plan(n, lo=l, hi=l + 1) == ([(l, -1, M, -1)], -1), l
    assert plan(n, lo=0, hi=0) == ([], -1)
    if n == 6:  # a segment of several layers that is not the whole stack: the same
        assert plan(n, lo=2, hi=6) == ([(l, -1, M, -1) for l in (5, 4, 3, 2)], -1)
        assert plan(n, lo=0, hi=5) == ([(l, -1, M, -1) for l in (4, 3, 2, 1, 0)], -1)


def test_bad_arguments_are_refused():
    from imagetranslate_amd._lib import ImtError
    for args in ((3, 2, 1), (3, 0, 4), (3, -1, 2), (65, 0, 65)):
        with pytest.raises(ImtError):
            O.stack_dw_schedule(args[0], args[1], args[2], True, [True] * args[0])


def _patterns(n):
    """Every pairable pattern of n layers with at most two unpairable ones."""
    yield [True] * n
    for k in (1, 2):
        for off in itertools.combinations(range(n), k):
            yield [l not in off for l in range(n)]


@pytest.mark.parametrize("n", range(2, 13))
def test_no_scratch_set_is_overwritten_under_a_running_launch(n):
    """Replay the records on a model of the two streams.  A side launch is 'synced' once the main stream has waited for a done
    event recorded behind it (or behind a later launch of the same stream).  When layer l writes scratch set l % 4, the launch
    that read layer l + 4's operands must have been issued, and be on the main stream or synced; no layer stays held; the call
    ends on the done of the last side launch."""
    for pairable in _patterns(n):
        records, join = plan(n, pairable)
        assert [r[0] for r in records] == list(range(n - 1, -1, -1))
        launch_of = {}          # layer -> ("main", None) | ("side", sequence number of its launch on the side stream)
        done_seq = {}           # layer -> sequence number of the side launch its done event was recorded behind
        synced, n_side, held, last_side = 0, 0, -1, -1
        for l, wait, action, with_held in records:
            if wait >= 0:
                assert wait in done_seq, (pairable, l, "waits for an event nobody recorded")
                synced = max(synced, done_seq[wait])
            if l + 4 < n:       # layer l + 4 used this scratch set
                assert l + 4 in launch_of, (pairable, l, "layer %d is still held" % (l + 4))
                stream, seq = launch_of[l + 4]
                assert stream == "main" or seq <= synced, (pairable, l, "layer %d's launch may still read the set" % (l + 4))
            if action == H:
                assert held < 0 and with_held == -1 and l > 0 and pairable[l], (pairable, l)
                held = l
                continue
            assert action == S and with_held == held, (pairable, l)
            n_side += 1
            for k in (l,) + ((held,) if held >= 0 else ()):
                launch_of[k] = ("side", n_side)
                done_seq[k] = n_side
            held, last_side = -1, l
        assert held < 0 and sorted(launch_of) == list(range(n)), pairable
        assert join == last_side == 0, pairable
