"""Multi-Krum HIP kernels (ops/hip/krum_kernels.hip) against the float64
specification (comm/robust.py): the op-level cases of tests/krum_cases.py —
participant counts around the row tile, vector lengths around the
coordinate chunk and at CNN size, slab seams, several models in one launch,
identical rows, non-finite rows, determinism, the collusion case — and FLJob
on the device. Bounds: tests/krum_cases.py."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import krum_cases as kc  # noqa: E402
import robust_cases as rc  # noqa: E402
import secagg_cases as sc  # noqa: E402
from feddrift_amd.ops import hip_loader, krum_hip  # noqa: E402

DEV = torch.device("cuda:0")
T, C = krum_hip.tile(), krum_hip.chunk()


def test_native_extension_has_the_kernels():
    mod = hip_loader.load()
    assert mod.__file__.endswith(".so")
    assert hasattr(mod, "krum")
    assert T >= 2 and C >= T and krum_hip.score_lds() >= T
    # the default slab keeps one model's rows within the 1 GiB of scratch
    assert 8 * krum_hip.scratch_rows() ** 2 <= 1 << 30
    assert 8 * int(mod.krum_scratch_elems()) <= 1 << 30


@pytest.mark.parametrize("n,P,select", kc.n_edge_list(T))
def test_n_edges(n, P, select):
    kc.case_shape(DEV, n, P, select)


@pytest.mark.parametrize("n,P,select", kc.p_edge_list(T, C))
def test_p_edges(n, P, select):
    kc.case_shape(DEV, n, P, select, scale=1.0)


@pytest.mark.parametrize("select", [0, 1])
def test_cnn_sized_vector(select):
    kc.case_cnn(DEV, select)


def test_row_longer_than_the_score_kernels_lds():
    """One participant more than the score kernel stages: the tail of every
    distance row streams from global memory."""
    n = krum_hip.score_lds() + 1
    kc.one_model(DEV, f"score row n={n}", kc.normal(n, 2, 21, 1.0), 0.2, 0)


@pytest.mark.parametrize("case", kc.OP_CASES, ids=lambda f: f.__name__)
def test_op_case(case):
    case(DEV)


def test_mutual_nearest_tie_across_slabs():
    """scratch_rows = 1: D[0, 1] and D[1, 0] come from different passes."""
    kc.case_mutual_nearest_tie(DEV, scratch_rows=1)


def test_scratch_bound_splits_several_models():
    """Two models of 40 and 25 rows under scratch_rows = 16: 3 passes, the
    smaller model idle in the last one; bit-equal to the whole launch."""
    vals = [kc.normal(40, 19, 1), kc.normal(25, 19, 2)]
    bank = np.concatenate(vals)
    models = np.concatenate([np.zeros(40, int), np.ones(25, int)])
    ids = 100 + np.random.default_rng(0).permutation(65)
    args = (DEV, bank, np.arange(65), models, np.ones(65, np.float32), ids,
            2, 0.2, 0)
    whole = kc.run(*args)
    slabs = kc.run(*args, scratch_rows=16)
    assert slabs[1]._scratch[1] == 16
    assert np.array_equal(kc.bits(whole[0]), kc.bits(slabs[0]))
    for m in range(2):
        assert np.array_equal(whole[2][m], slabs[2][m])
        assert np.array_equal(kc.bits64(whole[3][m]), kc.bits64(slabs[3][m]))
        kc.check_model(f"two models m={m}", vals[m], ids[models == m], 0.2,
                       0, slabs[0][m], slabs[2][m], slabs[3][m])


@pytest.mark.parametrize("n,P", kc.COLLUSION_SHAPES)
def test_collusion(n, P):
    kc.case_collusion(DEV, n, P)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_copy_to_the_host_in_an_aggregation():
    """A steady-state aggregation enqueues kernels only: with the plan's
    tensors uploaded, a second call runs under torch's synchronisation
    debug mode, in which a synchronising copy raises."""
    vals = kc.normal(12, 19, 8)
    bank = torch.from_numpy(vals).to(DEV)
    out = torch.zeros(1, 19, device=DEV)
    plan = krum_hip.KrumPlan(np.arange(12), np.zeros(12, int),
                             np.ones(12, np.float32), 1, 0.2)
    krum_hip.aggregate(bank, plan, out)
    torch.cuda.synchronize()
    first = out.clone()
    torch.cuda.set_sync_debug_mode("error")
    try:
        krum_hip.aggregate(bank, plan, out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(first, out)


# ------------------------------------------------------------------ FLJob

def test_fljob_poisoned_upload_on_device(tmp_path):
    kc.fljob_poison(tmp_path, DEV, use_hip="always")


def test_fljob_composition_matches_cpu_specification(tmp_path):
    """clip -> multi_krum -> noise -> Adam for three rounds on the device
    against the same job on the CPU, fed the device's replicas (the pattern
    of test_gpu_orderstat.py). server_lr 1e-3: an Adam step is
    lr m / (sqrt v + eps), so a relative error e of the pseudo-gradient
    moves the parameter by about lr e, far inside the output bound."""
    kw = dict(robust_fused=1, robust_norm_bound=0.05, robust_noise=1e-3,
              server_optimizer="adam", server_lr=1e-3,
              robust_agg="multi_krum", robust_krum_frac=0.2, n_clients=10)
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
        stat, bound, upd, kept = kc.job_stat_and_bound(jg, pg, 0.2, 0)
        assert upd.all() and all(len(k) == 4 for k in kept)
        jg.algo.aggregate(jg, r, pg, ci)
        jc.algo.aggregate(jc, r, pc, ci)
        for m, (a, b) in enumerate(zip(jg.krum_selection(),
                                       jc.krum_selection())):
            assert np.array_equal(a, b) and np.array_equal(a, kept[m]), (r, m)
        gg = jg.global_params.double().cpu().numpy()
        gc = jc.global_params.double().numpy()
        for m in range(jg.n_models):
            diff = np.abs(gg[m] - gc[m])
            print(f"FIG fljob multi_krum gpu-vs-spec round {r} model {m} | "
                  f"diff {diff.max():.3e} | bound {bound[m].max():.3e}")
            assert np.all(diff <= bound[m])
    assert jg._noise_ctr == jc._noise_ctr == 3


def test_fljob_model_mask_keeps_every_bit_on_device(tmp_path):
    job = sc.make_job(tmp_path, use_hip_kernels="always", n_clients=10,
                      robust_agg="multi_krum")
    ci = job.client_sampling(0)
    plan = rc.job_round(job, 0, ci)
    sc.torch_sync(job)
    before = job.global_params.cpu().numpy().copy()
    reps = job.replicas.cpu().numpy().copy()
    stat, bound, upd, kept = kc.job_stat_and_bound(job, plan, 0.2, 0)
    totals = job.aggregate(plan, model_mask=np.array([False, True]))
    sc.torch_sync(job)
    after = job.global_params.cpu().numpy()
    assert np.array_equal(kc.bits(after[0]), kc.bits(before[0]))
    assert np.all(np.abs(after[1].astype(np.float64) - stat[1]) <= bound[1])
    assert np.array_equal(kc.bits(job.replicas.cpu().numpy()), kc.bits(reps))
    assert np.array_equal(
        totals.cpu().numpy(),
        np.asarray(plan.sample_num, np.float32).sum(axis=0))
    assert np.array_equal(job.krum_selection()[1], kept[1])


def test_fljob_cnn_engine_round(tmp_path):
    from feddrift_amd.ops.cnn_hip import CnnHipEngine
    job = kc.fljob_cnn_round(tmp_path)
    assert job.device.type == "cuda"
    assert isinstance(job.mod_engine, CnnHipEngine)
