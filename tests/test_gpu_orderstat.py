"""Order-statistic aggregation HIP kernel (ops/hip/orderstat_kernels.hip)
against the float64 specification (comm/robust.py order_stat_mean): the
op-level cases of tests/orderstat_cases.py — participant counts around the
block's slice rows and the LDS-resident limit, vector lengths around a
tile and at CNN size, several models at once, ties, selection exactness,
poisoned rows, determinism — and FLJob on the device. Bounds:
tests/orderstat_cases.py."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import orderstat_cases as oc  # noqa: E402
import robust_cases as rc  # noqa: E402
import secagg_cases as sc  # noqa: E402
from feddrift_amd.ops import hip_loader, orderstat_hip  # noqa: E402

DEV = torch.device("cuda:0")
TP, LDS_ROWS = orderstat_hip.tile(), orderstat_hip.lds_rows()
SMALL = orderstat_hip.small_rows()


def test_native_extension_has_the_kernel():
    mod = hip_loader.load()
    assert mod.__file__.endswith(".so")
    assert hasattr(mod, "order_stat")
    assert 256 % TP == 0 and LDS_ROWS >= 256 // TP


@pytest.mark.parametrize("n,k,P", oc.n_edge_list(TP, LDS_ROWS, SMALL))
def test_n_edges(n, k, P):
    oc.case_shape(DEV, n, k, P)


@pytest.mark.parametrize("n,k,P", oc.p_edge_list(TP, SMALL))
def test_p_edges(n, k, P):
    oc.case_shape(DEV, n, k, P)


@pytest.mark.parametrize("k", [2, 1])
def test_cnn_sized_vector(k):
    oc.case_cnn(DEV, k)


@pytest.mark.parametrize("case", oc.OP_CASES, ids=lambda f: f.__name__)
def test_op_case(case):
    case(DEV)


@pytest.mark.parametrize("n,k,P", oc.POISON_CASES)
def test_poison(n, k, P):
    oc.case_poison(DEV, n, k, P)


def test_streamed_and_resident_models_in_one_launch():
    """Blocks of one launch take either path by their model's own count."""
    P, K = 2 * TP + 1, 3
    ns = [LDS_ROWS + 5, 3, LDS_ROWS]
    rng = np.random.default_rng(0)
    vals = [oc.normal(n, P, 40 + i) for i, n in enumerate(ns)]
    bank = np.concatenate(vals)
    perm = rng.permutation(len(bank))
    inv = np.argsort(perm)
    models = np.concatenate([np.full(n, m) for m, n in enumerate(ns)])
    out, plan = oc.run(DEV, bank[perm], inv, models,
                       np.ones(len(bank), np.float32), K, "trimmed_mean",
                       0.1)
    for m in range(K):
        oc.check_stat(f"mixed launch m={m}", out[m], vals[m],
                      int(plan.k[m]))


# ------------------------------------------------------------------ FLJob

@pytest.mark.parametrize("kind", ["trimmed_mean", "median"])
def test_fljob_poisoned_upload_on_device(tmp_path, kind):
    oc.fljob_poison(tmp_path, DEV, kind, 0.2, use_hip="always",
                    n_clients=10 if kind == "trimmed_mean" else 6)


def test_fljob_composition_matches_cpu_specification(tmp_path):
    """clip -> trimmed mean -> noise -> Adam for three rounds on the device
    against the same job on the CPU, fed the device's replicas (the pattern
    of test_gpu_robust.py). server_lr 1e-3: an Adam step is
    lr m / (sqrt v + eps), so a relative error e of the pseudo-gradient
    moves the parameter by about lr e, far inside the statistic's bound."""
    kw = dict(robust_fused=1, robust_norm_bound=0.05, robust_noise=1e-3,
              server_optimizer="adam", server_lr=1e-3,
              robust_agg="trimmed_mean", robust_trim_frac=0.2, n_clients=10)
    jg = sc.make_job(tmp_path / "g", use_hip_kernels="always", **kw)
    jc = sc.make_job(tmp_path / "c", device=torch.device("cpu"), **kw)
    assert jg.device.type == "cuda" and jc.device.type == "cpu"
    ci = jg.client_sampling(0)
    for r in range(3):
        jc.global_params.copy_(jg.global_params.cpu())
        pg = rc.job_round(jg, r, ci)
        sc.torch_sync(jg)
        pc = jc.algo.plan(jc, r, ci)
        jc.train(pc)
        assert np.array_equal(pc.sample_num, pg.sample_num)
        jc.replicas.copy_(jg.replicas.cpu())
        stat, bound, upd, ks = oc.job_stat_and_bound(
            jg.replicas, pg, jg.n_models, "trimmed_mean", 0.2)
        assert ks.max() >= 1
        jg.algo.aggregate(jg, r, pg, ci)
        jc.algo.aggregate(jc, r, pc, ci)
        gg = jg.global_params.double().cpu().numpy()
        gc = jc.global_params.double().numpy()
        for m in range(jg.n_models):
            diff = np.abs(gg[m] - gc[m])
            print(f"FIG fljob order-stat gpu-vs-spec round {r} model {m} | "
                  f"diff {diff.max():.3e} | bound {bound[m].max():.3e}")
            assert np.all(diff <= bound[m])
    assert jg._noise_ctr == jc._noise_ctr == 3


def test_fljob_model_mask_keeps_every_bit_on_device(tmp_path):
    job = sc.make_job(tmp_path, use_hip_kernels="always", n_clients=6,
                      robust_agg="median")
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    sc.torch_sync(job)
    before = job.global_params.cpu().numpy().copy()
    reps = job.replicas.cpu().numpy().copy()
    totals = job.aggregate(plan, model_mask=np.array([False, True]))
    sc.torch_sync(job)
    after = job.global_params.cpu().numpy()
    assert np.array_equal(oc.bits(after[0]), oc.bits(before[0]))
    rows = plan.rows[plan.rows % 2 == 1]
    oc.check_stat("fljob mask m=1", after[1], reps[rows], 1)
    assert np.array_equal(oc.bits(job.replicas.cpu().numpy()), oc.bits(reps))
    assert np.array_equal(
        totals.cpu().numpy(),
        np.asarray(plan.sample_num, np.float32).sum(axis=0))
