"""secure_agg=2: exact ring-arithmetic secure aggregation, on the CPU.

The numpy functions of comm/secure_agg.py are the specification the HIP
kernels are held to (tests/test_gpu_secagg.py); here the specification
itself is checked: Philox known answers, quantisation against exact
rational arithmetic, exact cancellation of the masks under the
`w % world` ownership rule, the mask graph, the range guard, and FLJob
end to end against a float64 mean with a bound computed from the inputs.
"""

from fractions import Fraction

import numpy as np
import pytest
import torch

import secagg_cases as sc
from feddrift_amd.comm import secure_agg as sa
from feddrift_amd.config import Config, config_from_argv
from feddrift_amd.ops import secagg_hip

F = sc.F


# ---------------------------------------------------------------- Philox

@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, expect):
    got = sa.philox4x32(ctr, key)
    assert " ".join(f"{int(v):08x}" for v in got) == expect


def test_ring_mask_layout():
    key = 0x299f31d0a4093822
    r = sa.ring_mask(key, 5)
    for j in range(3):
        x = [int(v) for v in sa.philox4x32(
            (j, 0, 0, 0), (key & 0xffffffff, key >> 32))]
        assert int(r[2 * j]) == (x[0] | x[1] << 32) & sa.RING_MASK
        if 2 * j + 1 < 5:
            assert int(r[2 * j + 1]) == (x[2] | x[3] << 32) & sa.RING_MASK
    assert r.max() < 2 ** sa.RING_BITS


# ---------------------------------------------------------- quantisation

def _exact_q(n, theta):
    """round-half-even(fp32(n * theta) * 2^F) in rational arithmetic."""
    prod = np.float32(n) * np.float32(theta)
    return round(Fraction(float(prod)) * 2 ** F) % 2 ** sa.RING_BITS


def test_quantise_matches_rational_arithmetic():
    ulp = 2.0 ** -F
    theta = np.array([-1.75, -0.0, 0.0, 0.3, -0.3, 1e-9, -1e-9,
                      0.5 * ulp, 1.5 * ulp, 2.5 * ulp, -0.5 * ulp,
                      -1.5 * ulp, 1000.25 + 0.5 * ulp], dtype=np.float32)
    for n in (1.0, 2.5, 120.0):
        q, bad = sa.quantise_upload(n, theta, F, 4)
        assert not bad
        for i, t in enumerate(theta):
            assert int(q[i]) == _exact_q(n, t), (n, t)
        assert int(q[-1]) == _exact_q(n, 1.0)
    # exact ties go to even; +-0 both give 0
    q, _ = sa.quantise_upload(1.0, theta, F, 4)
    assert [int(v) for v in q[7:10]] == [0, 2, 2]
    assert int(q[10]) == 0 and int(q[11]) == sa.RING_MASK - 1   # -2
    assert int(q[1]) == 0 and int(q[2]) == 0


def test_dequantise_of_quantise_within_half_step():
    rng = np.random.default_rng(1)
    theta = (rng.standard_normal(500) * 3).astype(np.float32)
    q, bad = sa.quantise_upload(1.0, theta, F, 4)
    assert not bad
    # with F = 24 and |q| < 2^24 * 16 every q / 2^F that arises from an
    # fp32 theta is an fp32 number again, so dequantise's final rounding to
    # fp32 adds nothing here and the half-step bound holds as stated
    back = sa.dequantise(q, F).astype(np.float64)
    assert back.dtype == np.float64 and sa.dequantise(q, F).dtype == np.float32
    assert np.all(np.abs(back[:-1] - theta.astype(np.float64))
                  <= 2.0 ** -(F + 1))
    assert back[-1] == 1.0
    # negative sums and sums that left [0, 2^M) reduce and sign-extend
    ring = np.array([-3 << F, (1 << 56) + (5 << F), (1 << 56) - (1 << F),
                     (1 << 55) - 1, 1 << 55], dtype=np.int64)
    assert sa.dequantise(ring, F).tolist() == [
        -3.0, 5.0, -1.0, float(np.float32((2 ** 55 - 1) / 2 ** F)),
        float(-2 ** (55 - F))]


# --------------------------------------------------- exact cancellation

def _seven_worker_act():
    # model 0: no active worker; model 1: one; model 2: six of seven
    return sc.act_matrix(7, 3, [[], [4], [0, 1, 2, 3, 5, 6]])


@pytest.mark.parametrize("P", [1, 34, 229])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_masks_cancel_exactly_complete_graph(P, world):
    case = sc.Case(P, _seven_worker_act(), seed=P)
    plain, bad = case.reference(masked=False)
    assert not bad
    for skip in (True, False):
        contribs = [case.reference(r, world, skip_intra=skip)[0]
                    for r in range(world)]
        assert np.array_equal(sc.ring_sum(contribs), plain)
    # model 0 has no upload, model 1 a single unmasked one
    assert not plain[0].any()


@pytest.mark.parametrize("degree", [2, 4])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_masks_cancel_exactly_sparse_graph(degree, world):
    act = sc.act_matrix(12, 3, [range(12), [3], range(1, 12)])
    case = sc.Case(34, act, degree=degree, seed=degree)
    assert all(case.graph.nbr[m] is not None for m in (0, 2))
    plain, _ = case.reference(masked=False)
    contribs = [case.reference(r, world)[0] for r in range(world)]
    assert np.array_equal(sc.ring_sum(contribs), plain)


@pytest.mark.parametrize("degree", [0, 4])
def test_skipping_intra_rank_pairs_is_bit_identical(degree):
    act = sc.act_matrix(12, 2, [range(12), range(0, 12, 2)])
    case = sc.Case(34, act, degree=degree, seed=3)
    for world in (1, 2, 3):
        for r in range(world):
            a, _ = case.reference(r, world, skip_intra=True)
            b, _ = case.reference(r, world, skip_intra=False)
            assert np.array_equal(a, b)


def test_masking_is_real():
    case = sc.Case(229, _seven_worker_act(), seed=9)
    for r in range(2):
        masked, _ = case.reference(r, 2)
        plain, _ = case.reference(r, 2, masked=False)
        cross = case.cross_rank_models(r, 2)
        assert cross == [2]
        for m in range(case.K):
            if m in cross:
                assert np.all(masked[m] != plain[m])
            else:
                assert np.array_equal(masked[m], plain[m])


# ----------------------------------------------------------------- graph

@pytest.mark.parametrize("degree", [0, 2, 4, 16])
def test_graph_symmetric_regular_and_shared(degree):
    act = sc.act_matrix(20, 4, [range(20), range(0, 20, 3), [5], []])
    g = sa.build_mask_graph(act, degree, 7, 2)
    g_other_rank = sa.build_mask_graph(act.copy(), degree, 7, 2)
    for m in range(4):
        a = g.active[m]
        A = len(a)
        for w in a:
            nb = g.neighbours(m, int(w))
            assert np.array_equal(nb, g_other_rank.neighbours(m, int(w)))
            assert w not in nb and len(set(nb.tolist())) == len(nb)
            for o in nb:                                   # symmetric
                assert w in g.neighbours(m, int(o))
            if A < 2:
                assert len(nb) == 0
            elif degree and A >= degree + 2:
                assert len(nb) == degree
            else:                                          # complete
                assert len(nb) == A - 1
    # 7 active workers: complete under degree 16, sparse under degree 2
    assert (g.nbr[1] is None) == (degree == 0 or 7 < degree + 2)


def test_graph_rejects_odd_degree():
    with pytest.raises(ValueError):
        sa.build_mask_graph(np.ones((6, 1), bool), 3, 0, 0)


def test_keys_differ_between_aggregations_and_pairs():
    base = sa.job_key(0, 1)
    lo, hi = np.triu_indices(12, 1)
    k1 = sa.pair_keys(base, 1, 0, lo, hi)
    k2 = sa.pair_keys(base, 2, 0, lo, hi)
    k1m = sa.pair_keys(base, 1, 1, lo, hi)
    allk = np.concatenate([k1, k2, k1m])
    assert len(np.unique(allk)) == len(allk)
    assert sa.job_key(0, 1) != sa.job_key(0, 2) != sa.job_key(1, 1)


# ----------------------------------------------------------- range guard

def _guard_case(value):
    act = sc.act_matrix(4, 1, [range(4)])
    case = sc.Case(6, act, seed=2)
    case.weights[:] = 1.0
    case.bank[case.rows[1], 3] = value
    return case


def test_range_guard():
    limit = 2.0 ** 55 / 4 / 2.0 ** F           # 2^29 with 4 workers
    under = np.nextafter(np.float32(limit), np.float32(0))
    for value, fires in ((limit, True), (-limit, True), (np.nan, True),
                         (np.inf, True), (under, False), (-under, False)):
        case = _guard_case(value)
        _, bad = case.reference()
        assert bad == fires, value
        out, flag = secagg_hip.contribution(
            torch.from_numpy(case.bank), case.plan(), case.base, case.ctr,
            F, case.W, skip_intra=False)
        assert np.array_equal(out.numpy(), case.reference(
            skip_intra=False)[0])
        if fires:
            with pytest.raises(RuntimeError, match="secure_agg_frac_bits"):
                secagg_hip.check_flag(flag, F)
        else:
            secagg_hip.check_flag(flag, F)


def test_range_guard_raises_from_fljob(tmp_path):
    job = sc.make_job(tmp_path, secure_agg=2)
    ci = job.client_sampling(0)
    plan = job.algo.plan(job, 0, ci)
    job.train(plan)
    job.replicas[0, 0] = float("nan")
    with pytest.raises(RuntimeError, match="secure_agg_frac_bits"):
        job.algo.aggregate(job, 0, plan, ci)


# ------------------------------------------------------------ end to end

def _check_rounds(results, prev0):
    prev = prev0
    for gp, mean, bound, upd in results:
        touched = 0
        for m in range(gp.shape[0]):
            if not upd[m] or np.array_equal(gp[m], prev[m]):
                continue          # no weight, or skipped by the model mask
            touched += 1
            err = np.abs(gp[m] - mean[m])
            assert np.all(err <= bound[m]), (m, (err / bound[m]).max())
        assert touched
        prev = gp


@pytest.mark.parametrize("skip_intra", [True, False])
def test_fljob_matches_float64_mean(tmp_path, skip_intra):
    job = sc.make_job(tmp_path, secure_agg=2)
    job.secagg_skip_intra = skip_intra
    prev0 = job.global_params.double().numpy().copy()
    _check_rounds(sc.rounds_against_float64(job, 3), prev0)


def test_fljob_sparse_graph(tmp_path):
    job = sc.make_job(tmp_path, n_clients=8, secure_agg=2,
                      secure_agg_degree=2)
    job.secagg_skip_intra = False
    prev0 = job.global_params.double().numpy().copy()
    _check_rounds(sc.rounds_against_float64(job, 3), prev0)


@pytest.mark.parametrize("kw", [dict(robust_norm_bound=0.5),
                                dict(server_optimizer="sgd")])
def test_fljob_composes_like_mode0(tmp_path, kw):
    """Same replicas into both modes each round: mode 2 stays within the
    derived bound plus mode 0's own distance from the float64 result."""
    j2 = sc.make_job(tmp_path, secure_agg=2, **kw)
    j0 = sc.make_job(tmp_path, secure_agg=0, **kw)
    ci = j2.client_sampling(0)
    for r in range(3):
        j0.global_params.copy_(j2.global_params)
        before = j2.global_params.double().numpy().copy()
        p2 = j2.algo.plan(j2, r, ci)
        p0 = j0.algo.plan(j0, r, ci)
        j2.train(p2)
        j0.train(p0)
        assert np.array_equal(p0.sample_num, p2.sample_num)
        j0.replicas.copy_(j2.replicas)
        mean, bound, upd = sc.mean_and_bound(j2.replicas, p2.sample_num,
                                             j2.n_models)
        j2.algo.aggregate(j2, r, p2, ci)
        j0.algo.aggregate(j0, r, p0, ci)
        g2 = j2.global_params.double().numpy()
        g0 = j0.global_params.double().numpy()
        touched = 0
        for m in range(j2.n_models):
            if not upd[m] or np.array_equal(g0[m], before[m]):
                continue
            touched += 1
            own0 = np.abs(g0[m] - mean[m])
            assert np.all(np.abs(g2[m] - g0[m]) <= bound[m] + own0), m
        assert touched


# ---------------------------------------------------------------- config

def test_config_fields_parse():
    cfg = config_from_argv(["--secure_agg", "2", "--secure_agg_degree", "4",
                            "--secure_agg_frac_bits", "20"])
    assert (cfg.secure_agg, cfg.secure_agg_degree,
            cfg.secure_agg_frac_bits) == (2, 4, 20)
    assert Config().secure_agg_degree == 0
    assert Config().secure_agg_frac_bits == 24
    with pytest.raises(ValueError):
        Config(secure_agg=2, secure_agg_degree=3)
    with pytest.raises(ValueError):
        config_from_argv(["--secure_agg_degree", "5"])
