"""Order-statistic aggregation (robust_agg = trimmed_mean | median) on the
CPU: the specification (comm/robust.py) against np.sort, np.median and
scipy.stats.trim_mean, the op-level cases of tests/orderstat_cases.py
against the specification path of ops/orderstat_hip.py, FLJob with a
poisoned upload, the composition with clipping and the server optimizer,
model_mask, the returned totals and the config checks. Bounds:
tests/orderstat_cases.py."""

import numpy as np
import pytest
import torch

import orderstat_cases as oc
import robust_cases as rc
import secagg_cases as sc
from feddrift_amd.comm import robust as rb
from feddrift_amd.config import Config, config_from_argv

CPU = torch.device("cpu")
# the block shape of the kernel (the GPU suite reads it from the extension);
# the CPU path has no tiles, the same shapes are run all the same
TP, LDS_ROWS, SMALL = 16, 768, 16


# ------------------------------------------------------------ specification

def test_ordered_key_is_a_total_order_that_agrees_with_np_sort():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        (rng.standard_normal(500) * 10.0 ** rng.integers(-44, 38, 500)
         ).astype(np.float32),
        np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf,
                  3.4e38, -3.4e38], np.float32)])
    keys = rb.ordered_key(x)
    assert keys.dtype == np.uint32
    by_key = x[np.argsort(keys, kind="stable")]
    assert np.array_equal(by_key, np.sort(x))          # -0 == +0 here
    ends = np.array([oc.NEG_NAN, 0xFF800000, 0x80000000, 0, 0x7F800000,
                     oc.POS_NAN], np.uint32).view(np.float32)
    k = rb.ordered_key(ends).astype(np.int64)
    assert np.all(np.diff(k) > 0)                      # -NaN < -Inf < -0 < ...
    assert k[0] < rb.ordered_key(x).min() and k[-1] > rb.ordered_key(x).max()


def test_trim_count_checked_values():
    for frac, n, k in ((0.1, 10, 1), (0.3, 10, 3), (0.29, 100, 29),
                       (0.2, 5, 1), (0.49, 3400, 1666), (0.0, 7, 0),
                       (0.49, 1, 0), (0.49, 2, 0), (0.4, 3, 1)):
        assert rb.trim_count("trimmed_mean", frac, n) == k, (frac, n)
    for n in range(1, 12):
        k = rb.trim_count("median", 0.0, n)
        assert k == (n - 1) // 2 and n - 2 * k in (1, 2)
    with pytest.raises(ValueError):
        rb.trim_count("mean", 0.1, 5)


@pytest.mark.parametrize("n", [1, 2, 7, 10, 70])
def test_specification_against_numpy_and_scipy(n):
    from scipy.stats import trim_mean
    vals = oc.normal(n, 13, n)
    v64 = vals.astype(np.float64)
    med = rb.order_stat_mean(vals, rb.trim_count("median", 0, n), np.float64)
    assert np.allclose(med, np.median(v64, axis=0), rtol=1e-15, atol=0)
    for frac in (0.0, 0.1, 0.2, 0.49):
        k = rb.trim_count("trimmed_mean", frac, n)
        got = rb.order_stat_mean(vals, k, np.float64)
        # scipy cuts int(frac * n) rows at either end
        if int(frac * n) == k:
            assert np.allclose(got, trim_mean(v64, frac, axis=0),
                               rtol=1e-14, atol=0), (n, frac)
        want = np.sort(v64, axis=0)[k:n - k].mean(axis=0)
        assert np.allclose(got, want, rtol=1e-14, atol=0)


def test_specification_is_invariant_under_row_permutation():
    vals, _ = oc.poisoned(70, 7, 9, 1)
    perm = np.random.default_rng(2).permutation(70)
    for dt in (np.float32, np.float64):
        a = rb.order_stat_mean(vals, 7, dt)
        b = rb.order_stat_mean(vals[perm], 7, dt)
        assert a.dtype == dt and a.tobytes() == b.tobytes()


def test_float32_specification_stays_inside_the_bound():
    """The bound comes from the formats; the float32 specification must
    meet it with room (a survey of n = 1 ... 3,400 saw at most 0.30)."""
    worst = 0.0
    for n in (3, 10, 70, 3400):
        for kind, frac in (("trimmed_mean", 0.0), ("trimmed_mean", 0.1),
                           ("trimmed_mean", 0.49), ("median", 0.0)):
            k = rb.trim_count(kind, frac, n)
            if n - 2 * k <= 2:
                continue
            vals = oc.normal(n, 11, n)
            ref = rb.order_stat_mean(vals, k, np.float64)
            s32 = rb.order_stat_mean(vals, k, np.float32)
            surv = oc.survivors(vals, k).astype(np.float64)
            bound = oc.U24 * (np.abs(surv).sum(0) + 4 * np.abs(ref))
            worst = max(worst, float((np.abs(s32 - ref) / bound).max()))
    print(f"FIG float32 specification | worst err/bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------ op-level cases

@pytest.mark.parametrize("n,k,P", oc.n_edge_list(TP, LDS_ROWS, SMALL))
def test_n_edges(n, k, P):
    oc.case_shape(CPU, n, k, P)


@pytest.mark.parametrize("n,k,P", oc.p_edge_list(TP, SMALL))
def test_p_edges(n, k, P):
    oc.case_shape(CPU, n, k, P)


@pytest.mark.parametrize("k", [2, 1])
def test_cnn_sized_vector(k):
    oc.case_cnn(CPU, k)


@pytest.mark.parametrize("case", oc.OP_CASES, ids=lambda f: f.__name__)
def test_op_case(case):
    case(CPU)


@pytest.mark.parametrize("n,k,P", oc.POISON_CASES)
def test_poison(n, k, P):
    oc.case_poison(CPU, n, k, P)


def test_aggregate_returns_counts_and_leaves_other_rows():
    bank = oc.normal(9, 6, 0)
    out = np.full((3, 6), 7.0, np.float32)
    n, k = rb.order_stat_aggregate(
        bank, [0, 2, 4, 6, 8, 1], [2, 2, 2, 2, 2, 0],
        [1.0, 1.0, 2.0, 1.0, 1.0, 0.0], 3, "trimmed_mean", 0.2, out)
    assert list(n) == [0, 0, 5] and list(k) == [0, 0, 1]
    assert np.all(out[:2] == 7.0)
    oc.check_stat("aggregate", out[2], bank[[0, 2, 4, 6, 8]], 1)


# -------------------------------------------------------------------- FLJob

@pytest.mark.parametrize("kind", ["trimmed_mean", "median"])
def test_fljob_poisoned_upload(tmp_path, kind):
    oc.fljob_poison(tmp_path, CPU, kind, 0.2,
                    n_clients=10 if kind == "trimmed_mean" else 6)


def test_fljob_model_mask_keeps_every_bit(tmp_path):
    job = sc.make_job(tmp_path, device=CPU, n_clients=6, robust_agg="median")
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    before = job.global_params.numpy().copy()
    _, _, upd, _ = oc.job_stat_and_bound(job.replicas, plan, job.n_models,
                                         "median", 0.0)
    assert upd.all()
    mask = np.array([False, True])
    totals = job.aggregate(plan, model_mask=mask)
    after = job.global_params.numpy()
    assert np.array_equal(oc.bits(after[0]), oc.bits(before[0]))
    assert not np.array_equal(after[1], before[1])
    assert np.array_equal(
        totals.numpy(), np.asarray(plan.sample_num, np.float32).sum(axis=0))


PAIR_KW = [dict(robust_norm_bound=0.05),
           dict(robust_norm_bound=0.05, server_optimizer="adam",
                server_lr=0.01)]


@pytest.mark.parametrize("kw", PAIR_KW)
def test_fljob_fused_matches_unfused(tmp_path, kw):
    """robust_fused=1 against robust_fused=0 under a trimmed mean, both fed
    the same clipped replicas, in the manner of test_robust_fused.py."""
    kw = dict(kw, robust_agg="trimmed_mean", robust_trim_frac=0.2,
              n_clients=10, device=CPU)      # n = 5 per model, k = 1
    j1 = sc.make_job(tmp_path, robust_fused=1, **kw)
    j0 = sc.make_job(tmp_path, robust_fused=0, **kw)
    ci = j1.client_sampling(0)
    state = rb.new_server_state(kw.get("server_optimizer", "avg"))
    for r in range(3):
        j0.global_params.copy_(j1.global_params)
        before = j1.global_params.double().numpy().copy()
        p1 = rc.job_round(j1, r, ci)
        p0 = rc.job_round(j0, r, ci, replicas_from=j1)
        norms = rc.update_norms(j1, p1, before)
        assert norms.max() <= 0.05 * (1 + 2.0 ** -20)
        stat, bound, upd, ks = oc.job_stat_and_bound(
            j1.replicas, p1, j1.n_models, "trimmed_mean", 0.2)
        assert ks.max() >= 1
        j1.algo.aggregate(j1, r, p1, ci)
        j0.algo.aggregate(j0, r, p0, ci)
        g1 = j1.global_params.double().numpy()
        g0 = j0.global_params.double().numpy()
        live = upd & ~np.all(g0 == before, axis=1) \
            if state["kind"] == "avg" else upd
        ref = torch.from_numpy(before.copy())
        rb.server_step(state["kind"], ref, torch.from_numpy(stat),
                       torch.from_numpy(live), state,
                       kw.get("server_lr", 1.0), 0.0)
        ref = ref.numpy()
        touched = 0
        for m in range(j1.n_models):
            if not live[m]:
                continue
            touched += 1
            own0 = np.abs(g0[m] - ref[m])
            diff = np.abs(g1[m] - g0[m])
            print(f"FIG fljob order-stat round {r} model {m} | "
                  f"max|fused-unfused|={diff.max():.3e} | "
                  f"own0={own0.max():.3e} | bound={bound[m].max():.3e}")
            assert np.all(diff <= bound[m] + own0), (r, m)
            if state["kind"] == "avg":
                assert np.all(np.abs(g1[m] - stat[m]) <= bound[m])
        assert touched


def test_fljob_noise_counter_advances_as_before(tmp_path):
    kw = dict(robust_fused=1, robust_noise=1e-3, n_clients=6, device=CPU)
    ja = sc.make_job(tmp_path / "a", robust_agg="median", **kw)
    jb = sc.make_job(tmp_path / "b", **kw)
    ci = ja.client_sampling(0)
    for r in range(2):
        for j in (ja, jb):
            j.algo.aggregate(j, r, rc.job_round(j, r, ci), ci)
    assert ja._noise_ctr == jb._noise_ctr == 2


def test_module_path_runs_the_statistic(tmp_path):
    """The op only reads replica rows: the CNN (module) path takes it too."""
    from feddrift_amd.comm import Communicator
    from feddrift_amd.data.generators import sample_mnist
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.engine.timeline import clean_state_files
    from feddrift_amd.eval.metrics import MetricLogger
    import os
    ds = DriftDataset(data_dir="/nonexistent", dataset="MNIST", num_client=3)
    rng = np.random.default_rng(0)
    for c in range(3):
        for t in range(2):
            arr = sample_mnist(48, 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    cfg = Config(model="cnn", dataset="MNIST", data_dir="/nonexistent",
                 client_num_in_total=3, client_num_per_round=3,
                 batch_size=48, lr=0.01, epochs=1, comm_round=1,
                 total_train_iteration=2, concept_num=2,
                 concept_drift_algo="softcluster",
                 concept_drift_algo_arg="mmacc_06",
                 log_dir=str(tmp_path / "m"), report_client=0,
                 robust_agg="median")
    os.makedirs(cfg.log_dir, exist_ok=True)
    clean_state_files(cfg)
    job = FLJob(cfg, Communicator(device=CPU),
                MetricLogger(enabled=False, to_file=False), dataset=ds)
    assert job.is_module_path
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    before = job.global_params.numpy().copy()
    stat, bound, upd, ks = oc.job_stat_and_bound(
        job.replicas, plan, job.n_models, "median", 0.0)
    job.algo.aggregate(job, 0, plan, ci)
    got = job.global_params.numpy()
    assert upd.any()
    for m in range(job.n_models):
        if upd[m] and not np.array_equal(got[m], before[m]):
            rows = plan.rows[plan.rows % job.n_models == m]
            oc.check_stat(f"module path m={m}", got[m],
                          job.replicas.numpy()[rows], int(ks[m]))
        else:
            assert np.array_equal(oc.bits(got[m]), oc.bits(before[m]))


# ------------------------------------------------------------------- config

def test_config_validation():
    with pytest.raises(ValueError, match="robust_agg"):
        Config(robust_agg="krum")
    for frac in (0.5, -0.1, 0.7):
        with pytest.raises(ValueError, match="robust_trim_frac"):
            Config(robust_trim_frac=frac)
    for secure in (1, 2):
        with pytest.raises(ValueError, match="individual uploads"):
            Config(robust_agg="median", secure_agg=secure)
    assert Config().robust_agg == "mean" and Config().robust_trim_frac == 0.1
    Config(robust_agg="mean", secure_agg=2)
    Config(robust_agg="trimmed_mean", robust_trim_frac=0.0)
    cfg = config_from_argv(["--robust_agg", "trimmed_mean",
                            "--robust_trim_frac", "0.25"])
    assert cfg.robust_agg == "trimmed_mean" and cfg.robust_trim_frac == 0.25
