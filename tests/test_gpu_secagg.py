"""secure_agg=2 HIP kernels (ops/hip/secagg_kernels.hip) against the numpy
specification (comm/secure_agg.py), bit for bit: vector lengths around a
block's element span and at CNN size, upload counts below and above one
slice's share, unsorted and non-contiguous replica rows, 0 / 1 / d edges
with both signs, intra-rank pairs included and skipped, an emulated world
of 3, the dequantise kernel, the range-guard flag, and FLJob on the device
against a float64 mean with the bound computed from the inputs."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import secagg_cases as sc  # noqa: E402
from feddrift_amd.comm import secure_agg as sa  # noqa: E402
from feddrift_amd.ops import secagg_hip  # noqa: E402

DEV = torch.device("cuda:0")
F = sc.F


def _kernel(case, rank=0, world=1, skip_intra=True, n_workers=None):
    out, flag = secagg_hip.contribution(
        torch.from_numpy(case.bank).to(DEV), case.plan(rank, world),
        case.base, case.ctr, F, n_workers or case.W, rank, world,
        skip_intra=skip_intra)
    return out.cpu().numpy(), int(flag.item())


def _check(case, rank=0, world=1, skip_intra=True):
    got, flag = _kernel(case, rank, world, skip_intra)
    want, bad = case.reference(rank, world, skip_intra)
    assert not bad and flag == 0
    assert got.dtype == np.int64 and got.min() >= 0 \
        and got.max() < 2 ** sa.RING_BITS
    assert np.array_equal(got, want)
    return got


def _span_lengths():
    s = secagg_hip.span()
    return [2, 35, s - 1, s, s + 1]


@pytest.mark.parametrize("idx", range(5))
def test_vector_lengths(idx):
    L = _span_lengths()[idx]
    case = sc.Case(L - 1, sc.act_matrix(3, 1, [range(3)]), seed=L)
    masked = _check(case, skip_intra=False)
    plain, _ = case.reference(masked=False)
    # the three pair masks cancel inside the one rank
    assert np.array_equal(masked, plain)
    # and they are real: one worker's share of the same model is masked
    part = _check(case, rank=1, world=3, skip_intra=True)
    assert np.all(part != case.reference(1, 3, masked=False)[0])


def test_cnn_sized_vector():
    from feddrift_amd.models import zoo
    from feddrift_amd.models.generic_packer import ModulePacker
    P = ModulePacker(zoo.CNN_DropOut()).n_params
    case = sc.Case(P, sc.act_matrix(4, 1, [range(4)]), seed=4, scale=0.05)
    # 4 uploads, 3 edges each (world 1, intra-rank pairs included)
    _check(case, skip_intra=False)


@pytest.mark.parametrize("n_up,degree", [(1, 0), (2, 0), (3, 0), (70, 4)])
def test_upload_counts_and_edges(n_up, degree):
    """1 upload: no edge. 2: one edge each, one of each sign. 70 with
    degree 4: d edges per upload and more uploads than one slice sums."""
    case = sc.Case(34, sc.act_matrix(n_up, 1, [range(n_up)]),
                   degree=degree, seed=n_up)
    plan = case.plan()
    assert (plan.slices > 1) == (n_up == 70)
    if degree:
        assert set(plan.up_ec.tolist()) == {degree}
    for skip in (False, True):
        _check(case, skip_intra=skip)
    if n_up > 1:
        plain, _ = case.reference(masked=False)
        for world in (2, 3):
            parts = [_check(case, r, world) for r in range(world)]
            assert np.array_equal(sc.ring_sum(parts), plain)


def test_three_models_one_empty_unsorted_rows():
    act = sc.act_matrix(7, 3, [[], [4], [0, 1, 2, 3, 5, 6]])
    case = sc.Case(229, act, seed=11)
    # upload order is mixed across models and the rows have holes
    assert np.any(np.diff(case.rows) < 0)
    assert np.any(np.diff(case.pairs[:, 1]) < 0)
    plain, _ = case.reference(masked=False)
    full = _check(case, skip_intra=False)
    assert np.array_equal(full, plain) and not full[0].any()
    parts = [_check(case, r, 3) for r in range(3)]
    assert np.array_equal(sc.ring_sum(parts), plain)
    for r in range(3):
        own_plain, _ = case.reference(r, 3, masked=False)
        for m in case.cross_rank_models(r, 3):
            assert np.all(parts[r][m] != own_plain[m])


def test_dequantise_bits():
    rng = np.random.default_rng(5)
    M = sa.RING_BITS
    ring = rng.integers(0, 1 << M, size=(3, 1027), dtype=np.int64)
    # a full world of contributions: sums of 128 values in [0, 2^M)
    ring[1] = ring[1] * 128 - rng.integers(0, 128, size=1027)
    # small negative and positive sums, and the sign boundary
    ring[2, :6] = [-3 << F, (1 << M) - 1, 1 << (M - 1), (1 << (M - 1)) - 1,
                   0, (5 << F) + (1 << M) * 100]
    ring[2, 6:500] = rng.integers(-(1 << 40), 1 << 40, size=494) % (1 << M)
    out = torch.empty(3, 1027, device=DEV)
    secagg_hip.dequantise(torch.from_numpy(ring).to(DEV), out, F)
    want = sa.dequantise(ring, F)
    assert np.array_equal(out.cpu().numpy().view(np.uint32),
                          want.view(np.uint32))
    assert want[2, 0] == -3.0 and want[2, 5] == 5.0


def test_guard_flag():
    limit = np.float32(2.0 ** 55 / 4 / 2.0 ** F)
    under = np.nextafter(limit, np.float32(0))
    for value, fires in ((limit, True), (np.nan, True), (-np.inf, True),
                         (under, False), (-under, False)):
        case = sc.Case(6, sc.act_matrix(4, 1, [range(4)]), seed=2)
        case.weights[:] = 1.0
        case.bank[case.rows[1], 3] = value
        got, flag = _kernel(case, skip_intra=False)
        want, bad = case.reference(skip_intra=False)
        assert bad == fires and (flag != 0) == fires, value
        assert np.array_equal(got, want)


def test_fljob_on_device_matches_float64_mean(tmp_path):
    job = sc.make_job(tmp_path, secure_agg=2, use_hip_kernels="always")
    assert job.device.type == "cuda"
    job.secagg_skip_intra = False           # world 1: draw every mask
    prev = job.global_params.double().cpu().numpy().copy()
    for gp, mean, bound, upd in sc.rounds_against_float64(job, 3):
        touched = 0
        for m in range(gp.shape[0]):
            if not upd[m] or np.array_equal(gp[m], prev[m]):
                continue
            touched += 1
            err = np.abs(gp[m] - mean[m])
            print(f"model {m}: max err/bound {(err / bound[m]).max():.3f}")
            assert np.all(err <= bound[m]), (m, (err / bound[m]).max())
        assert touched
        prev = gp
    job.check_secure_guard()
