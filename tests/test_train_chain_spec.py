"""The CPU side of tests/test_gpu_train_chain.py: the numpy emulations the
GPU probe is held to, its two inputs, and the seed rule of the end-to-end
cases (tests/train_chain_cases.py). No GPU."""

import numpy as np
import pytest

import gpu_variant_cases as vc
import train_chain_cases as tc


def test_probe_sizes_are_the_template_shapes():
    assert sorted(tc.PROBE_TPS) == sorted(tc.shape_tps())
    assert max(tc.PROBE_TPS) <= 64


@pytest.mark.parametrize("tp", tc.PROBE_TPS)
def test_butterfly_has_the_bits_of_the_tree(tp):
    """The reduce-scatter adds, in every lane that keeps an entry, the two
    values the shuffle-down tree adds (commuted in half the lanes): equal
    bits over 200 wide-magnitude draws, on which a left-to-right sum
    differs, so the draw can tell summation orders apart."""
    differs = 0
    for seed in range(200):
        wide, _ = tc.probe_inputs(tp, seed)
        tree = tc.tree_reduce(wide)
        assert tc.same_bits(tc.scatter_reduce(wide), tree), seed
        differs += not tc.same_bits(tc.left_to_right(wide), tree)
    assert differs >= 190, differs


@pytest.mark.parametrize("tp", tc.PROBE_TPS)
def test_routing_case_is_exact(tp):
    _, route = tc.probe_inputs(tp)
    want = (4096.0 * np.arange(tp) + 2016.0).astype(np.float32)
    assert float(route.max()) * 64 < 2 ** 24
    assert tc.same_bits(tc.tree_reduce(route), want)
    assert tc.same_bits(tc.scatter_reduce(route), want)
    assert tc.same_bits(tc.left_to_right(route), want)
    # a column or a lane swapped changes the result
    swapped = route.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    assert not tc.same_bits(tc.tree_reduce(swapped), want)


def test_owner_lanes():
    assert [tc.bitrev6(p) for p in (0, 1, 2, 3, 37)] == [0, 32, 16, 48, 41]
    assert sorted(tc.bitrev6(p) for p in range(64)) == list(range(64))


@pytest.mark.parametrize("lens", [tc.CHAIN_LENS, tc.CHAIN_LENS_256])
def test_step_table(lens):
    t = tc.step_table(lens)
    assert t.shape == (tc.G, tc.E)
    assert set(t.view(-1).tolist()) == set(lens)
    assert t[0, 0] == 0 and t[0, 1] > 0          # first
    assert t[1, -1] == 0 and t[1, -2] > 0        # last
    assert t[2, 1] == 0 and t[2, 2] == 0         # twice in a row
    # E = 1 keeps a zero-length and a non-zero only step
    assert (t[:, 0] == 0).any() and (t[:, 0] > 0).any()


@pytest.mark.parametrize("lens,seeds", [
    (tc.CHAIN_LENS, tc.CHAIN_SEEDS), (tc.CHAIN_LENS_256, tc.CHAIN_SEEDS_256)])
def test_seeds_follow_the_err32_rule(lens, seeds):
    """fp32 torch resolves every draw (err32 <= 1e-5), and each seed is the
    first from 100 + shape index that does."""
    assert tuple(seeds) == tuple(100 + i for i in range(len(vc.SMALL_SHAPES)))
    worst = tc.measure_err32(lens, seeds)
    assert max(worst.values()) <= tc.ERR32_MAX, worst
