"""mlp_train_small_kernel's step chain (ops/hip/feddrift_kernels.hip): the
wave reduce-scatter, the owner lane's register-resident optimizer step and
the up-front sample loads.

The reduce runs alone through the test-only binding train_reduce_probe and
has to give the bits of the shuffle-down tree it replaced (numpy float32
emulation; tests/test_train_chain_spec.py checks the emulation and the
inputs without a GPU). End to end, all five template shapes run against the
float64 specification under vc.MLP_TRAIN_TOL with step lengths on both
sides of the prefetch bound and zero-length steps first, last and twice in
a row; bodies, cases and seeds: tests/train_chain_cases.py.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import gpu_variant_cases as vc  # noqa: E402
import train_chain_cases as tc  # noqa: E402
from feddrift_amd.ops import hip_loader  # noqa: E402

DEV = torch.device("cuda:0")

CASES = list(tc.chain_cases(tc.CHAIN_LENS, tc.CHAIN_SEEDS))


def _probe(vals):
    out = hip_loader.load().train_reduce_probe(
        torch.from_numpy(vals).to(DEV).contiguous())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("tp", tc.PROBE_TPS)
def test_reduce_probe_has_the_bits_of_the_tree(tp):
    wide, route = tc.probe_inputs(tp)
    got = _probe(route)
    assert tc.same_bits(got, tc.tree_reduce(route)), (tp, got)
    for seed in range(4):
        wide, _ = tc.probe_inputs(tp, seed)
        want = tc.tree_reduce(wide)
        assert not tc.same_bits(tc.left_to_right(wide), want)
        got = _probe(wide)
        assert tc.same_bits(got, want), (tp, seed, got, want)


def test_reduce_probe_rejects_other_sizes():
    with pytest.raises(RuntimeError):
        hip_loader.load().train_reduce_probe(torch.zeros(64, 7, device=DEV))
    with pytest.raises(RuntimeError):
        hip_loader.load().train_reduce_probe(torch.zeros(32, 38, device=DEV))


@pytest.mark.parametrize("c", CASES,
                         ids=[c[0].replace(" ", "-") for c in CASES])
def test_chain(c):
    """G = 6, E = 4 (or 1), lengths (0, 1, 64, 511, 512, 513, 600):
    64-thread blocks (the default)."""
    tc.check_chain(c, tc.CHAIN_LENS)


@pytest.mark.parametrize("kind,d,o", vc.SMALL_SHAPES)
def test_rows_outside_the_launch_keep_every_bit(kind, d, o):
    i = vc.SMALL_SHAPES.index((kind, d, o))
    tc.check_carried_rows(kind, d, o, tc.CHAIN_LENS, tc.CHAIN_SEEDS[i])


def test_chain_256_thread_blocks():
    """The same cases at lengths (0, 1, 255, 256, 257, 600) in a child
    process with FEDDRIFT_TRAIN_BS64_MIN_G set huge (latched once per
    process): the waves' sums meet in wave order in wave 0's owner lanes."""
    hip_loader.load()                  # the child must find it built
    env = dict(os.environ, FEDDRIFT_TRAIN_BS64_MIN_G="1000000")
    r = subprocess.run([sys.executable, tc.__file__, "chain_bs256"], env=env,
                       timeout=240, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-4000:])
    assert "case chain_bs256 OK" in r.stdout
