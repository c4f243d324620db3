"""robust_fused=1 on the CPU: the specification of the defended aggregation
(comm/robust.py: clip_and_accumulate, gaussian_noise, server_step) against
norm_diff_clipping + einsum and ServerOptimizer in float64, and FLJob with
the option on against the option off on the same replicas."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import robust_cases as rc
import secagg_cases as sc
from feddrift_amd.comm import robust as rb
from feddrift_amd.comm import secure_agg as sa

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEY = sa.job_key(3, 1)


# ------------------------------------------------------------------- noise

@pytest.mark.parametrize("P", [1, 5, 38])
def test_noise_chunking_and_odd_lengths(P):
    K = 3
    full = rb.gaussian_noise(KEY, 7, K, P)
    assert full.shape == (K, P) and full.dtype == np.float64
    assert np.isfinite(full).all()
    for m in range(K):
        for p0 in range(P):
            for p1 in (p0 + 1, P):
                part = rb.gaussian_noise(KEY, 7, K, P, models=[m], p0=p0,
                                         p1=p1)
                assert np.array_equal(part[0], full[m, p0:p1])
    # a longer row starts with the shorter one
    assert np.array_equal(rb.gaussian_noise(KEY, 7, K, P + 3)[:, :P], full)


def test_noise_differs_across_ctr_model_key():
    a = rb.gaussian_noise(KEY, 1, 2, 64)
    assert not np.any(a[0] == a[1])
    assert not np.any(a == rb.gaussian_noise(KEY, 2, 2, 64))
    assert not np.any(a == rb.gaussian_noise(KEY, 1 + (1 << 32), 2, 64))
    assert not np.any(a == rb.gaussian_noise(sa.job_key(3, 2), 1, 2, 64))
    assert rb.noise_key(3, 2) == sa.job_key(3, 2)


def test_noise_moments_and_float32_form():
    n = 1 << 16
    z = rb.gaussian_noise(KEY, 1, 4, n // 4).reshape(-1)
    print(f"FIG noise | mean={z.mean():.4e} (5/sqrt n={5 / np.sqrt(n):.4e})"
          f" | var={z.var():.5f}")
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 0.05
    z32 = rb.gaussian_noise(KEY, 1, 4, n // 4, dtype=np.float32).reshape(-1)
    assert z32.dtype == np.float32
    # float32 rounds x to 24 bits before the logarithm and the angle
    assert np.abs(z32 - z).max() < 1e-5


# ---------------------------------------------------------------- clipping

def test_clip_scale():
    assert rb.clip_scale(0.0, 0.05) == 1.0
    assert rb.clip_scale(0.04, 0.05) == 1.0
    assert rb.clip_scale(5.0, 0.05) == pytest.approx(0.01)
    t = rb.clip_scale(torch.tensor([0.0, 0.1], dtype=torch.float64), 0.05)
    assert t.tolist() == [1.0, pytest.approx(0.5)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_clip_and_accumulate_against_norm_diff_clipping(dtype):
    case = rc.ClipCase(229, 3, rc.five_norm_pairs(), seed=1)
    assert np.any(np.diff(case.rows) < 0)              # unsorted, with holes
    assert set(case.models) == {0, 2}                   # model 1: no pair
    bank, partial, c, s = case.spec(dtype)
    got_bank = bank.astype(np.float32) if dtype == torch.float64 else bank
    if dtype == torch.float64:
        ref_bank, ref_partial = case.reference(torch.float64)
        assert np.abs(bank - ref_bank).max() <= 1e-15
        assert np.abs(partial - ref_partial).max() <= 1e-12
        for i, kind in enumerate(case.kinds):
            if kind in ("zero", "near"):
                assert np.array_equal(bank[case.rows[i]],
                                      case.bank[case.rows[i]].astype(float))
        hc, hs = case.hand_counts()
        assert np.array_equal(c, hc) and np.array_equal(s, hs)
        assert hc.sum() > 0 and hs[1] == 0 and not partial[1].any()
    else:
        rc.check_clip("spec32 five norms", case, got_bank, partial,
                      np.stack([c, s], 1))
    # partial=None: only the replicas change, and in the same way
    bank2, none, c2, s2 = case.spec(dtype, with_partial=False)
    assert none is None and np.array_equal(bank2, bank)
    assert np.array_equal(c2, c) and np.array_equal(s2, s)


def test_zero_weight_row_is_clipped_but_adds_nothing():
    case = rc.ClipCase(5, 1, [(0, 0.0, "far"), (0, 0.0, "rand")], seed=2)
    bank, partial, c, s = case.spec(torch.float64)
    assert not partial.any()
    norms = np.linalg.norm(bank[case.rows] - case.glob[0], axis=1)
    assert np.all(norms <= case.bound * (1 + 1e-9))
    assert c[0] >= 1 and s[0] == 2


# ------------------------------------------------------------- server step

@pytest.mark.parametrize("kind,lr,momentum", rc.SERVER_CASES)
def test_server_step_matches_server_optimizer(kind, lr, momentum):
    glob, avgs, upds = rc.server_inputs(3, 41, seed=4)
    want = rc.server_reference(kind, lr, momentum, glob, avgs, upds)
    got = rc.server_spec(kind, lr, momentum, glob, avgs, upds, torch.float64)
    for step, (w, g) in enumerate(zip(want, got)):
        err = np.abs(w - g).max()
        print(f"FIG server_step {kind} step {step} | max diff {err:.3e}")
        # same formulas in float64, operations grouped differently
        assert err <= 1e-13
    if kind != "avg":
        # the non-updated row was still stepped (state decay), or kept
        moved = not np.array_equal(got[1][2], got[0][2])
        assert moved == (kind == "adam" or momentum != 0)


def test_sgd_lr1_equals_avg():
    glob, avgs, upds = rc.server_inputs(3, 17, seed=5)
    a = rc.server_spec("avg", 1.0, 0.0, glob, avgs, upds, torch.float64)
    s = rc.server_spec("sgd", 1.0, 0.0, glob, avgs, upds, torch.float64)
    for x, y in zip(a, s):
        assert np.abs(x - y).max() <= 1e-15


def test_server_step_rejects_unknown_kind():
    with pytest.raises(ValueError, match="adagrad"):
        rb.new_server_state("rmsprop")


# ---------------------------------------------------------- FLJob equality

def _paired_rounds(tmp_path, kw, rounds=3):
    """robust_fused=1 and =0 jobs fed the same replicas every round; yields
    per round (j1, j0, plan, before, mean, bound, upd)."""
    j1 = sc.make_job(tmp_path, robust_fused=1, **kw)
    j0 = sc.make_job(tmp_path, robust_fused=0, **kw)
    ci = j1.client_sampling(0)
    for r in range(rounds):
        j0.global_params.copy_(j1.global_params)
        before = j1.global_params.double().numpy().copy()
        p1 = rc.job_round(j1, r, ci)
        p0 = rc.job_round(j0, r, ci, replicas_from=j1)
        assert np.array_equal(p0.sample_num, p1.sample_num)
        mean, bound, upd = sc.mean_and_bound_atomic(
            j1.replicas, p1.sample_num, j1.n_models)
        j1.algo.aggregate(j1, r, p1, ci)
        j0.algo.aggregate(j0, r, p0, ci)
        yield j1, j0, p1, before, mean, bound, upd


def _float64_step(kw, state, before, mean, upd):
    """The float64 result of one defended step on the float64 mean."""
    g = torch.from_numpy(before.copy())
    rb.server_step(kw.get("server_optimizer", "avg"), g,
                   torch.from_numpy(mean), torch.from_numpy(upd), state,
                   kw.get("server_lr", 1.0), kw.get("server_momentum", 0.0))
    return g.numpy()


@pytest.mark.parametrize("kw", [
    dict(robust_norm_bound=0.05),
    dict(server_optimizer="adam", server_lr=0.01),
    dict(server_optimizer="sgd", server_lr=0.5, server_momentum=0.9)])
def test_fljob_fused_matches_unfused(tmp_path, kw):
    state = rb.new_server_state(kw.get("server_optimizer", "avg"))
    for r, (j1, j0, plan, before, mean, bound, upd) in enumerate(
            _paired_rounds(tmp_path, kw)):
        g1 = j1.global_params.double().numpy()
        g0 = j0.global_params.double().numpy()
        # models the softcluster mask skipped keep their rows in both jobs
        live = upd & ~np.all(g0 == before, axis=1) \
            if state["kind"] == "avg" else upd
        ref = _float64_step(kw, state, before, mean, live)
        touched = 0
        for m in range(j1.n_models):
            if not live[m]:
                continue
            touched += 1
            own0 = np.abs(g0[m] - ref[m])
            diff = np.abs(g1[m] - g0[m])
            print(f"FIG fljob {kw} round {r} model {m} | "
                  f"max|fused-unfused|={diff.max():.3e} | "
                  f"own0={own0.max():.3e} | bound={bound[m].max():.3e}")
            assert np.all(diff <= bound[m] + own0), (r, m)
        assert touched
        if "robust_norm_bound" in kw:
            st = j1.clip_stats()
            assert np.array_equal(st[:, 0], st[:, 1]) and st[:, 1].sum() > 0
            assert not j1.clip_stats().any()            # reset by the call


def test_fljob_wide_bound_clips_nothing(tmp_path):
    """Update norms are 0.11-0.12 here: 0.5 clips no pair, and the result
    agrees with the undefended job's."""
    for r, (j1, j0, plan, before, mean, bound, upd) in enumerate(
            _paired_rounds(tmp_path / "a", dict(robust_norm_bound=0.5))):
        norms = rc.update_norms(j1, plan, before)
        assert 0.05 < norms.min() and norms.max() < 0.5
        st = j1.clip_stats()
        assert st[:, 0].sum() == 0 and st[:, 1].sum() == len(plan.rows)
    wide = j1.global_params.clone()
    for r, (k1, k0, plan, before, mean, bound, upd) in enumerate(
            _paired_rounds(tmp_path / "b", dict(robust_norm_bound=0.0))):
        pass
    # both pairs of jobs trained the same replicas from the same seeds
    g1, g0 = wide.double().numpy(), k1.global_params.double().numpy()
    for m in range(j1.n_models):
        if upd[m]:
            own0 = np.abs(k0.global_params[m].double().numpy() - mean[m])
            print(f"FIG wide bound model {m} | "
                  f"diff={np.abs(g1[m] - g0[m]).max():.3e}")
            assert np.all(np.abs(g1[m] - g0[m]) <= bound[m] + own0)


# ------------------------------------------------------------- composition

def test_composes_with_ring_secure_agg(tmp_path):
    job = sc.make_job(tmp_path, robust_fused=1, robust_norm_bound=0.05,
                      secure_agg=2)
    job.secagg_skip_intra = False
    ci = job.client_sampling(0)
    prev = job.global_params.double().numpy().copy()
    for r in range(3):
        plan = rc.job_round(job, r, ci)
        norms = rc.update_norms(job, plan, prev)
        assert norms.max() <= 0.05 * (1 + 2.0 ** -20)
        mean, bound, upd = sc.mean_and_bound(job.replicas, plan.sample_num,
                                             job.n_models)
        job.algo.aggregate(job, r, plan, ci)
        gp = job.global_params.double().numpy()
        touched = 0
        for m in range(job.n_models):
            if not upd[m] or np.array_equal(gp[m], prev[m]):
                continue
            touched += 1
            err = np.abs(gp[m] - mean[m])
            print(f"FIG ring+clip round {r} model {m} | "
                  f"err/bound={(err / bound[m]).max():.3f}")
            assert np.all(err <= bound[m])
        assert touched
        prev = gp
    st = job.clip_stats()
    assert np.array_equal(st[:, 0], st[:, 1]) and st[:, 1].sum() > 0


def test_noise_moves_only_updated_models(tmp_path):
    job = sc.make_job(tmp_path, robust_fused=1, robust_noise=1e-3)
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    K, P = job.n_models, job.n_params
    # model 1: zero weight everywhere; model 0 aggregates
    plan.sample_num = np.asarray(plan.sample_num, dtype=np.float32).copy()
    plan.sample_num[:, 0] = np.maximum(plan.sample_num[:, 0], 1.0)
    plan.sample_num[:, 1] = 0.0
    plan.template = None
    job._partial_fused = False                # weights changed after train
    before = job.global_params.clone()
    mean, _, upd = sc.mean_and_bound_atomic(job.replicas, plan.sample_num, K)
    job.aggregate(plan)
    assert torch.equal(job.global_params[1], before[1])
    z = rb.gaussian_noise(job._noise_key, 1, K, P, dtype=np.float32)
    want = mean[0] + 1e-3 * z[0].astype(np.float64)
    assert np.abs(job.global_params[0].double().numpy() - want).max() < 1e-6
    assert np.abs(job.global_params[0].double().numpy() - mean[0]).max() \
        > 1e-4
    # masked out: the bits stay, whatever the weights
    plan2 = rc.job_round(job, 1, ci)
    before = job.global_params.clone()
    job.aggregate(plan2, model_mask=np.zeros(K, dtype=bool))
    assert torch.equal(job.global_params, before)
    assert not job._partial.any()


def test_noise_depends_on_iteration(tmp_path):
    a = sc.make_job(tmp_path / "a", robust_fused=1, robust_noise=1e-3)
    from dataclasses import replace
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    cfg_b = replace(a.cfg, curr_train_iteration=0,
                    log_dir=str(tmp_path / "b"))
    b = FLJob(cfg_b, a.comm, MetricLogger(enabled=False, to_file=False),
              dataset=a.dataset)
    assert a.cfg.dummy_arg == b.cfg.dummy_arg and a.curr_iter != b.curr_iter
    assert a._noise_key != b._noise_key
    za = rb.gaussian_noise(a._noise_key, 1, 2, 16)
    zb = rb.gaussian_noise(b._noise_key, 1, 2, 16)
    assert not np.any(za == zb)


def test_unsupported_optimizer_raises(tmp_path):
    with pytest.raises(ValueError, match="avg.*sgd.*adam.*adagrad"):
        sc.make_job(tmp_path, robust_fused=1, server_optimizer="rmsprop")


def test_fused_with_no_option_is_the_plain_round(tmp_path):
    for r, (j1, j0, plan, before, mean, bound, upd) in enumerate(
            _paired_rounds(tmp_path, {})):
        g1 = j1.global_params.double().numpy()
        g0 = j0.global_params.double().numpy()
        for m in range(j1.n_models):
            if upd[m] and not np.array_equal(g0[m], before[m]):
                own0 = np.abs(g0[m] - mean[m])
                assert np.all(np.abs(g1[m] - g0[m]) <= bound[m] + own0)
            else:
                assert np.array_equal(g1[m], g0[m])
        assert not j1.clip_stats().any()


def test_config_and_cli_fields():
    from feddrift_amd.config import Config, config_from_argv
    cfg = config_from_argv(["--robust_fused", "1", "--server_momentum",
                            "0.9"])
    assert cfg.robust_fused == 1 and cfg.server_momentum == 0.9
    assert Config().robust_fused == 0 and Config().server_momentum == 0.0
    with pytest.raises(ValueError, match="robust_fused"):
        Config(robust_fused=2)


def test_torch_engine_forwards_momentum(tmp_path):
    job = sc.make_job(tmp_path, server_optimizer="sgd", server_lr=0.5,
                      server_momentum=0.9)
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    job.algo.aggregate(job, 0, plan, ci)
    assert job._server_opt.opt.defaults["momentum"] == 0.9


# --------------------------------------------------------------- multi-rank

_WORKER = r"""
import os, sys, pathlib
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
import torch
import secagg_cases as sc

job = sc.make_job(pathlib.Path({log!r}), device=torch.device("cpu"),
                  n_clients=6, robust_fused=1, robust_norm_bound=0.05,
                  robust_noise=1e-3, server_optimizer="adam", server_lr=0.01)
ci = job.client_sampling(0)
K = job.n_models
for r in range(2):
    plan = job.algo.plan(job, r, ci)
    job.train(plan)
    # replicas that depend only on the global (worker, model) id and the
    # round, so every world size uploads the same values
    for wi, w in enumerate(job.owned_workers):
        for m in range(K):
            g = torch.Generator().manual_seed(1000 + (r * 64 + w) * K + m)
            job.replicas[wi * K + m] = job.global_params[m] + \
                0.1 * torch.randn(job.n_params, generator=g)
    job._partial.zero_()
    job._robust_clip_fused(plan, False)
    job.algo.aggregate(job, r, plan, ci)
stats = job.clip_stats()
np.savez(os.path.join({log!r}, "rank%d.npz" % job.comm.rank),
         global_params=job.global_params.numpy(), stats=stats,
         replicas=job.replicas.numpy(),
         sample_num=np.asarray(plan.sample_num, dtype=np.float32))
"""


def _launch(nproc, log, port):
    os.makedirs(log, exist_ok=True)
    path = os.path.join(log, "worker.py")
    with open(path, "w") as f:
        f.write(_WORKER.format(repo=REPO, log=log))
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           "--nnodes", "1", "--nproc-per-node", str(nproc), path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_world2_matches_world1(tmp_path):
    w1, w2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    _launch(1, w1, 29671)
    _launch(2, w2, 29672)
    one = np.load(os.path.join(w1, "rank0.npz"))
    two = [np.load(os.path.join(w2, f"rank{r}.npz")) for r in range(2)]
    # identical noise and identical all-reduced sums on both ranks
    assert np.array_equal(two[0]["global_params"].view(np.uint32),
                          two[1]["global_params"].view(np.uint32))
    assert np.array_equal(two[0]["stats"], one["stats"])
    assert np.array_equal(two[0]["stats"][:, 0], two[0]["stats"][:, 1])
    assert one["stats"][:, 1].sum() > 0
    # the last round's clipped replicas, as world 1 holds them
    K = one["sample_num"].shape[1]
    mean, bound, upd = sc.mean_and_bound_atomic(
        torch.from_numpy(one["replicas"]), one["sample_num"], K)
    diff = np.abs(two[0]["global_params"].astype(np.float64)
                  - one["global_params"].astype(np.float64))
    # server_lr 0.01: an Adam step moves a parameter by about lr, so its
    # own float32 rounding stays far inside the bound of the mean
    for m in range(K):
        if upd[m]:
            print(f"FIG world2 model {m} | max diff {diff[m].max():.3e} | "
                  f"bound {bound[m].max():.3e}")
            assert np.all(diff[m] <= bound[m])


# -------------------------------------------------------------- module path

def test_module_path_fused_matches_unfused(tmp_path):
    """The CNN (module) path: the clip pass after mod_engine.train fills
    the partial tensor, and the round agrees with the unfused one."""
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_mnist
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.engine.timeline import clean_state_files
    from feddrift_amd.eval.metrics import MetricLogger
    ds = DriftDataset(data_dir="/nonexistent", dataset="MNIST", num_client=3)
    rng = np.random.default_rng(0)
    for c in range(3):
        for t in range(2):
            arr = sample_mnist(48, 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    jobs = []
    for fused in (1, 0):
        cfg = Config(model="cnn", dataset="MNIST", data_dir="/nonexistent",
                     client_num_in_total=3, client_num_per_round=3,
                     batch_size=48, lr=0.01, epochs=1, comm_round=1,
                     total_train_iteration=2, concept_num=2,
                     concept_drift_algo="softcluster",
                     concept_drift_algo_arg="mmacc_06",
                     log_dir=str(tmp_path / f"f{fused}"), report_client=0,
                     robust_fused=fused, robust_norm_bound=0.05)
        os.makedirs(cfg.log_dir, exist_ok=True)
        clean_state_files(cfg)
        jobs.append(FLJob(cfg, Communicator(),
                          MetricLogger(enabled=False, to_file=False),
                          dataset=ds))
    j1, j0 = jobs
    assert j1.is_module_path
    ci = j1.client_sampling(0)
    before = j1.global_params.double().numpy().copy()
    p1 = rc.job_round(j1, 0, ci)
    assert j1._partial_fused                 # aggregate skips the einsum
    p0 = rc.job_round(j0, 0, ci, replicas_from=j1)
    norms = rc.update_norms(j1, p1, before)
    assert norms.max() <= 0.05 * (1 + 2.0 ** -20)
    mean, bound, upd = sc.mean_and_bound_atomic(j1.replicas, p1.sample_num,
                                                j1.n_models)
    j1.algo.aggregate(j1, 0, p1, ci)
    j0.algo.aggregate(j0, 0, p0, ci)
    g1 = j1.global_params.double().numpy()
    g0 = j0.global_params.double().numpy()
    assert upd.any()
    for m in range(j1.n_models):
        if upd[m] and not np.array_equal(g0[m], before[m]):
            own0 = np.abs(g0[m] - mean[m])
            diff = np.abs(g1[m] - g0[m])
            print(f"FIG module path model {m} | diff {diff.max():.3e} | "
                  f"bound {bound[m].max():.3e}")
            assert np.all(diff <= bound[m] + own0)
        else:
            assert np.array_equal(g1[m], g0[m])
    st = j1.clip_stats()
    assert st[:, 1].sum() == len(p1.rows) and st[:, 0].sum() > 0


def test_clip_fraction_is_logged_only_when_fused(tmp_path):
    from feddrift_amd.eval.metrics import MetricLogger
    for fused in (1, 0):
        job = sc.make_job(tmp_path, robust_fused=fused,
                          robust_norm_bound=0.05)
        job.logger = MetricLogger(enabled=True, to_file=False)
        ci = job.client_sampling(0)
        plan = rc.job_round(job, 0, ci)
        job.algo.aggregate(job, 0, plan, ci)
        job.algo.test(job, 0)
        keys = {k for rec in job.logger.records for k in rec}
        logged = {k for k in keys if k.startswith("Robust/ClipFrac-m")}
        if fused:
            assert logged and all(job.logger.series(k) == [1.0]
                                  for k in logged)
        else:
            assert not logged
