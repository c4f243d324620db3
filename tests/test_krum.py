"""Multi-Krum aggregation (robust_agg = multi_krum) on the CPU: the numpy
specification's own properties (comm/robust.py), the op-level cases of
tests/krum_cases.py against the specification path of ops/krum_hip.py, the
collusion case the coordinate-wise rules lose, FLJob on a CPU device, and
the config. Bounds: tests/krum_cases.py."""

import numpy as np
import pytest
import torch

import krum_cases as kc
import robust_cases as rc
import secagg_cases as sc
from feddrift_amd.comm import robust as rb
from feddrift_amd.config import Config, config_from_argv
from feddrift_amd.ops import krum_hip

CPU = torch.device("cpu")


# ------------------------------------------------------------ specification

def test_krum_f_edges():
    want = {0.0: [0] * 7, 0.2: [0, 0, 0, 0, 1, 1, 1],
            0.49: [0, 0, 0, 0, 1, 1, 2]}
    for frac, fs in want.items():
        assert [rb.krum_f(frac, n) for n in range(1, 8)] == fs, frac
    for frac in want:
        for n in range(3, 60):
            assert n >= 2 * rb.krum_f(frac, n) + 3
    assert rb.krum_f(0.2, 10) == 2 and rb.krum_f(0.2, 20) == 4
    assert rb.krum_f(0.1, 10) == 1          # floor(0.1 * 10 + 1e-9)


def test_sqdist_is_direct_symmetric_and_infinite_for_nonfinite_rows():
    v = kc.normal(6, 33, 0)
    v[4, 3] = np.nan
    v[5, 0] = np.inf
    D = rb.krum_sqdist(v)
    assert np.all(np.diag(D) == 0.0)
    assert np.array_equal(kc.bits64(D), kc.bits64(D.T))
    assert np.all(np.isposinf(D[4, :4])) and np.all(np.isposinf(D[5, :5]))
    want = ((v[0].astype(np.float64) - v[1].astype(np.float64)) ** 2).sum()
    assert abs(D[0, 1] - want) <= 2 * 35 * kc.U53 * want
    # where the Gram form cancels: a shared offset of 1e4 and updates of
    # 1e-3 leave the direct differences exact to the bound
    base = np.float32(1e4) + np.float32(1e-3) * kc.normal(4, 9, 1, 1.0)
    exact = ((base[0].astype(np.float64) - base[1].astype(np.float64)) ** 2
             ).sum()
    assert abs(rb.krum_sqdist(base)[0, 1] - exact) <= 2 * 11 * kc.U53 * exact


def test_scores_sum_the_q_smallest_in_ascending_order():
    D = rb.krum_sqdist(kc.normal(7, 5, 2))
    f = 2                                   # q = 3
    got = rb.krum_scores(D, f)
    for i in range(7):
        off = np.sort(np.delete(D[i], i))
        assert got[i] == (off[0] + off[1]) + off[2]
    assert np.array_equal(rb.krum_scores(np.zeros((1, 1)), 0), [0.0])
    two = rb.krum_scores(np.array([[0.0, 4.0], [4.0, 0.0]]), 0)
    assert np.array_equal(two, [4.0, 4.0])


def test_select_orders_by_score_then_id():
    pos = rb.krum_select([2.0, 1.0, 1.0, np.inf, 0.5], [5, 9, 3, 0, 7], 4)
    assert list(pos) == [4, 2, 1, 0]


def _agg(values, ids, frac, select, weights=None):
    values = np.ascontiguousarray(values, dtype=np.float32)
    n = len(values)
    out = np.full((1, values.shape[1]), 7.0, np.float32)
    w = np.ones(n, np.float32) if weights is None else weights
    res = rb.multi_krum_aggregate(values, np.arange(n), np.zeros(n, int), w,
                                  ids, 1, frac, select, out)
    return out[0], res


def test_one_and_two_participants():
    v = kc.normal(2, 9, 3)
    out, (n, f, s, chosen, scores) = _agg(v[:1], [4], 0.2, 0)
    assert np.array_equal(kc.bits(out), kc.bits(v[0]))
    assert (n[0], f[0], s[0]) == (1, 0, 1) and scores[0][0] == 0.0
    # n = 2, classic Krum: the scores tie (one distance), the lower id wins
    for ids, win in (([4, 2], 1), ([2, 4], 0)):
        out, (_, _, s, chosen, scores) = _agg(v, ids, 0.2, 1)
        assert scores[0][0] == scores[0][1]
        assert list(chosen[0]) == [2]
        assert np.array_equal(kc.bits(out), kc.bits(v[win]))


def test_select_1_returns_a_participants_bits():
    v = kc.normal(9, 21, 4)
    v[:, 0] = np.array([1e-45, -0.0, 3e-39, 1.5, -2.25, 0.0, 7e-41, 1e-38, 2],
                       np.float32)
    out, (_, _, s, chosen, _) = _agg(v, np.arange(9), 0.2, 1)
    assert s[0] == 1
    assert np.array_equal(kc.bits(out), kc.bits(v[int(chosen[0][0])]))


def test_frac_0_select_0_is_the_unweighted_mean():
    v = kc.normal(13, 17, 5)
    w = np.linspace(1, 50, 13).astype(np.float32)      # weights do not count
    out, (_, f, s, chosen, _) = _agg(v, np.arange(13), 0.0, 0, weights=w)
    assert f[0] == 0 and s[0] == 13
    assert sorted(chosen[0]) == list(range(13))
    mean = v.astype(np.float64).mean(axis=0)
    bound = kc.U24 * (np.abs(v.astype(np.float64)).sum(axis=0)
                      + 2.0 * np.abs(mean))
    assert np.all(np.abs(out.astype(np.float64) - mean) <= bound)


def test_zero_weight_pair_is_no_participant():
    v = np.concatenate([kc.normal(6, 11, 6),
                        np.full((1, 11), 50.0, np.float32)])
    w = np.array([1, 2.5, 7, 1, 1, 120, 0], np.float32)
    out, (n, f, s, chosen, scores) = _agg(v, np.arange(7), 0.0, 0, weights=w)
    assert n[0] == 6 and s[0] == 6 and len(scores[0]) == 6
    assert 6 not in set(chosen[0])
    assert np.abs(out).max() < 1.0


def test_aggregate_returns_counts_and_leaves_other_rows():
    bank = kc.normal(9, 6, 0)
    out = np.full((3, 6), 7.0, np.float32)
    before = bank.copy()
    n, f, s, chosen, scores = rb.multi_krum_aggregate(
        bank, [0, 2, 4, 6, 8, 1], [2, 2, 2, 2, 2, 0],
        [1.0, 1.0, 2.0, 1.0, 1.0, 0.0], [10, 11, 12, 13, 14, 15], 3, 0.2, 0,
        out)
    assert list(n) == [0, 0, 5] and list(f) == [0, 0, 1]
    assert list(s) == [0, 0, 4]
    assert np.all(out[:2] == 7.0) and len(chosen[0]) == len(chosen[1]) == 0
    assert set(chosen[2]) <= {10, 11, 12, 13, 14} and len(chosen[2]) == 4
    assert np.array_equal(kc.bits(bank), kc.bits(before))


# --------------------------------------------- the op on a CPU device

@pytest.mark.parametrize("n,P,select", kc.n_edge_list(32))
def test_n_edges(n, P, select):
    kc.case_shape(CPU, n, P, select)


@pytest.mark.parametrize("n,P,select",
                         [c for c in kc.p_edge_list(32, 64) if c[0] == 5])
def test_p_edges(n, P, select):
    kc.case_shape(CPU, n, P, select, scale=1.0)


@pytest.mark.parametrize("case", kc.OP_CASES, ids=lambda f: f.__name__)
def test_op_case(case):
    case(CPU)


@pytest.mark.parametrize("n,P", kc.COLLUSION_SHAPES)
def test_collusion(n, P):
    kc.case_collusion(CPU, n, P)


def test_last_selection_needs_an_aggregation():
    plan = krum_hip.KrumPlan([0, 1, 2], [0, 0, 0], [1, 1, 1], 1, 0.2)
    with pytest.raises(RuntimeError, match="last_selection"):
        krum_hip.last_selection(plan)


def test_scratch_layout_respects_the_bounds():
    n = np.array([5000, 0, 17, 5000])
    slab, d_off, need = krum_hip.scratch_layout(n, 1, 8192, 1 << 27)
    assert slab == 5000 and need == 2 * 5000 * 5000 + 17 * 17
    assert list(d_off) == [0, 25_000_000, 25_000_000, 25_000_289]
    slab, d_off, need = krum_hip.scratch_layout(n, 1, 100, 1 << 27)
    assert slab == 100 and need == 2 * 100 * 5000 + 17 * 17
    # the element budget wins over the row bound
    slab, d_off, need = krum_hip.scratch_layout(n, 3, 8192, 1 << 20)
    assert need <= 1 << 20
    assert 3 * int((np.minimum(slab + 1, n) * n).sum()) > 1 << 20
    with pytest.raises(ValueError, match="scratch"):
        krum_hip.scratch_layout(np.array([1 << 20]), 2, 8192, 1 << 20)


# -------------------------------------------------------------------- FLJob

def test_fljob_poisoned_upload(tmp_path):
    kc.fljob_poison(tmp_path, CPU)


def test_fljob_module_path(tmp_path):
    job = kc.fljob_cnn_round(tmp_path, device=CPU)
    assert job.is_module_path


COMPOSE = dict(robust_norm_bound=0.05, robust_noise=1e-3,
               server_optimizer="adam", server_lr=0.01,
               robust_agg="multi_krum", robust_krum_frac=0.2, n_clients=10)


def test_fljob_composition_fused_and_unfused_select_alike(tmp_path):
    """clip -> multi_krum -> noise -> adam for three rounds with
    robust_fused 1 and 0, both fed the same clipped replicas: the selection
    is the specification's on both, totals are the weight sums, the
    replicas keep every bit and the noise counter advances once a round."""
    j1 = sc.make_job(tmp_path, device=CPU, robust_fused=1, **COMPOSE)
    j0 = sc.make_job(tmp_path, device=CPU, robust_fused=0, **COMPOSE)
    ci = j1.client_sampling(0)
    K = j1.n_models
    for r in range(3):
        j0.global_params.copy_(j1.global_params)
        before = j1.global_params.double().numpy().copy()
        p1 = rc.job_round(j1, r, ci)
        p0 = rc.job_round(j0, r, ci, replicas_from=j1)
        assert rc.update_norms(j1, p1, before).max() <= 0.05 * (1 + 2.0 ** -20)
        _, _, upd, kept = kc.job_stat_and_bound(j1, p1, 0.2, 0)
        assert upd.all() and all(len(k) == 4 for k in kept)
        reps = j1.replicas.numpy().copy()
        for j, p in ((j1, p1), (j0, p0)):
            totals = j.aggregate(p)
            assert np.array_equal(
                totals.numpy(),
                np.asarray(p.sample_num, np.float32).reshape(-1, K).sum(0))
            picked = j.krum_selection()
            for m in range(K):
                assert np.array_equal(picked[m], kept[m]), (r, m)
            assert np.all(np.isfinite(j.global_params.numpy()))
            assert not np.array_equal(j.global_params.double().numpy(),
                                      before)
        assert np.array_equal(kc.bits(j1.replicas.numpy()), kc.bits(reps))
    assert j1._noise_ctr == 3


def test_fljob_fused_matches_unfused_without_noise(tmp_path):
    """clip -> multi_krum -> adam: robust_fused=1 against robust_fused=0,
    in the manner of test_orderstat.py's test_fljob_fused_matches_unfused."""
    kw = dict(COMPOSE, robust_noise=0.0, device=CPU)
    j1 = sc.make_job(tmp_path, robust_fused=1, **kw)
    j0 = sc.make_job(tmp_path, robust_fused=0, **kw)
    ci = j1.client_sampling(0)
    state = rb.new_server_state("adam")
    for r in range(3):
        j0.global_params.copy_(j1.global_params)
        before = j1.global_params.double().numpy().copy()
        p1 = rc.job_round(j1, r, ci)
        p0 = rc.job_round(j0, r, ci, replicas_from=j1)
        stat, bound, upd, _ = kc.job_stat_and_bound(j1, p1, 0.2, 0)
        j1.algo.aggregate(j1, r, p1, ci)
        j0.algo.aggregate(j0, r, p0, ci)
        g1 = j1.global_params.double().numpy()
        g0 = j0.global_params.double().numpy()
        ref = torch.from_numpy(before.copy())
        rb.server_step("adam", ref, torch.from_numpy(stat),
                       torch.from_numpy(upd), state, 0.01, 0.0)
        ref = ref.numpy()
        assert upd.any()
        for m in np.nonzero(upd)[0]:
            own0 = np.abs(g0[m] - ref[m])
            diff = np.abs(g1[m] - g0[m])
            print(f"FIG fljob multi_krum round {r} model {m} | "
                  f"max|fused-unfused|={diff.max():.3e} | "
                  f"own0={own0.max():.3e} | bound={bound[m].max():.3e}")
            assert np.all(diff <= bound[m] + own0), (r, m)


def test_fljob_model_mask_keeps_every_bit(tmp_path):
    job = sc.make_job(tmp_path, device=CPU, n_clients=10,
                      robust_agg="multi_krum")
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    before = job.global_params.numpy().copy()
    reps = job.replicas.numpy().copy()
    stat, bound, upd, kept = kc.job_stat_and_bound(job, plan, 0.2, 0)
    assert upd.all()
    totals = job.aggregate(plan, model_mask=np.array([False, True]))
    after = job.global_params.numpy()
    assert np.array_equal(kc.bits(after[0]), kc.bits(before[0]))
    assert np.all(np.abs(after[1].astype(np.float64) - stat[1]) <= bound[1])
    assert np.array_equal(kc.bits(job.replicas.numpy()), kc.bits(reps))
    assert np.array_equal(
        totals.numpy(), np.asarray(plan.sample_num, np.float32).sum(axis=0))
    assert np.array_equal(job.krum_selection()[1], kept[1])


def test_fljob_classic_krum_stores_an_upload(tmp_path):
    job = sc.make_job(tmp_path, device=CPU, n_clients=10,
                      robust_agg="multi_krum", robust_krum_select=1)
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    _, _, upd, kept = kc.job_stat_and_bound(job, plan, 0.2, 1)
    job.aggregate(plan)
    parts = kc.job_participants(job, plan)
    for m in np.nonzero(upd)[0]:
        rows, wid = parts[m]
        row = int(rows[list(wid).index(int(kept[m][0]))])
        assert np.array_equal(kc.bits(job.global_params[m].numpy()),
                              kc.bits(job.replicas[row].numpy()))


# ------------------------------------------------------------------- config

def test_config_validation():
    cfg = Config(robust_agg="multi_krum")
    assert cfg.robust_krum_frac == 0.2 and cfg.robust_krum_select == 0
    with pytest.raises(ValueError, match="robust_agg"):
        Config(robust_agg="krum")
    for frac in (0.5, -0.1):
        with pytest.raises(ValueError, match="robust_krum_frac"):
            Config(robust_krum_frac=frac)
    with pytest.raises(ValueError, match="robust_krum_select"):
        Config(robust_krum_select=-1)
    for secure in (1, 2):
        with pytest.raises(ValueError, match="secure_agg"):
            Config(robust_agg="multi_krum", secure_agg=secure)
    Config(robust_agg="multi_krum", robust_krum_frac=0.0,
           robust_krum_select=1)
    cfg = config_from_argv(["--robust_agg", "multi_krum",
                            "--robust_krum_frac", "0.25",
                            "--robust_krum_select", "3"])
    assert (cfg.robust_agg, cfg.robust_krum_frac, cfg.robust_krum_select) \
        == ("multi_krum", 0.25, 3)
