"""CPU test: utils.mass_span_starts, the host restatement of MASS span starts that sizes every output of mass_mask_device
and is handed to imt_mass_mask, against the loop-form oracle (oracle/batch_oracle.py: counter_uniform streams 0 / 1 and
span_start with its two-rounding float32 bound), row by row."""
import numpy as np
import pytest
import torch

from oracle import batch_oracle as BO

N_ROWS = 10000
SEED = (0x5EED << 32) | 0x1234ABCD   # both halves of the 64-bit seed are used by the generator


@pytest.mark.parametrize("mask_prob", [0.15, 0.3, 0.5, 0.9, 1 - 1e-6])
def test_host_span_starts_equal_the_oracle(mask_prob):
    from imagetranslate_amd.utils import mass_span_starts
    g = torch.Generator().manual_seed(17)
    pad = torch.randint(1, 601, (N_ROWS,), generator=g)
    pad[:600] = torch.arange(1, 601)      # every pad index once, whatever the draw
    got = mass_span_starts(mask_prob, pad, SEED)
    assert got.dtype == torch.int64 and tuple(got.shape) == (N_ROWS,)
    want = [BO.span_start(mask_prob, int(pad[r]), BO.counter_uniform(SEED, 0, r), BO.counter_uniform(SEED, 1, r)) for r in range(N_ROWS)]
    want = torch.tensor(want, dtype=torch.int64)
    bad = (got != want).nonzero().view(-1)
    assert bad.numel() == 0, "row %d (pad %d): host %d, oracle %d" % (int(bad[0]), int(pad[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
    # the three branches of the rule all occur, and so does a start of 2 below a bound of 2
    assert bool((want == 1).any()) and bool((want > 2).any()) and bool(((want == 2) & (pad <= 2)).any())


def test_host_generator_equals_the_oracle_generator():
    from imagetranslate_amd.utils import _counter_uniform
    idx = torch.cat([torch.arange(0, 300), torch.tensor([2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1])])
    for seed in (0, 5, SEED, 2 ** 62 - 1):
        for stream in (0, 1, 3):
            got = _counter_uniform(seed, stream, idx)
            want = np.array([BO.counter_uniform(seed, stream, int(i)) for i in idx], dtype=np.float32)
            assert got.dtype == np.float32 and np.array_equal(got, want), (seed, stream)


@pytest.mark.parametrize("name", ["wrap", "wrap-clipped", "clipped", "short-pads"])
def test_gpu_mass_case_has_the_property_it_is_named_for(name):
    """The case definitions of tests/test_gpu_batch_edges.py, with the oracle alone: guarded here too, where no GPU is needed."""
    from tests import test_gpu_batch_edges as E
    assert list(E.MASS_CASES) == ["wrap", "wrap-clipped", "clipped", "short-pads"]
    E.check_mass_case(name)


def test_span_sizes_clamp_like_the_kernel():
    """mass_span_sizes: start clamped to [1, width], length to [0, width], span clipped at the row's end."""
    from imagetranslate_amd.utils import mass_span_sizes
    first, hidden = mass_span_sizes(torch.tensor([0, 3, 9, 12, 2, 5]), torch.tensor([8, 8, 8, 8, 1, 40]), 10)
    assert first.tolist() == [1, 3, 9, 10, 2, 5] and hidden.tolist() == [4, 4, 1, 0, 0, 5]


def test_two_rounding_bound():
    """pad = 50, p = 0.3: 50 - 35.0 = 15 with the product rounded first; a fused multiply-add gives 15.0000006 -> 16."""
    from imagetranslate_amd.utils import mass_span_starts
    seeds = [s for s in range(200) if np.float32(0.6) < BO.counter_uniform(s, 0, 0) <= np.float32(0.8)][:3]
    assert seeds
    for s in seeds:   # the branch that returns the bound itself
        assert int(mass_span_starts(0.3, torch.tensor([50]), s)[0]) == 15
