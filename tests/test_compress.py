"""upload_compress=topk on the CPU: the specification
(feddrift_amd/comm/compress.py) on hand-written rows, the options, and FLJob
against a by-hand loop of plain training plus the specification, bit for
bit. Shared bodies: tests/compress_cases.py."""

import numpy as np
import pytest
import torch

import compress_cases as cc
import secagg_cases as sc
from feddrift_amd.comm import compress as spec
from feddrift_amd.config import Config
from feddrift_amd.ops import compress_hip

CPU = torch.device("cpu")


# ------------------------------------------------------------ specification

def test_keep_count_edges():
    assert spec.keep_count(1e-9, 1000) == 1          # ratio -> k = 1
    assert spec.keep_count(0.01, 1) == 1
    assert spec.keep_count(1.0, 38) == 38            # k = P
    assert spec.keep_count(0.999, 38) == 38
    assert spec.keep_count(0.25, 1000) == 250        # an exact integer
    assert spec.keep_count(0.5, 38) == 19
    assert spec.keep_count(0.1, 38) == 4             # ceil(3.8)
    assert spec.keep_count(0.01, 1199882) == 11999


@pytest.mark.parametrize("case", cc.hand_cases(), ids=lambda c: c[0])
def test_hand_written_row(case):
    name, theta, g, e, k, sent = case
    n = cc.check_hand_case(*case)
    if name.startswith("ties"):
        assert n == 3 > k
    if name in ("all-zero update", "residual cancels"):
        assert n == 0
    if name == "fewer non-zeros than k":
        assert n == 1 < k


def test_more_non_finite_than_k_keeps_the_residual_finite():
    name, theta, g, e, k, sent = cc.hand_cases()[-1]
    nt, nr, a, got = spec.topk_rows(theta[None], g[None], e[None], k)
    assert np.isinf(a[0, 1]) and not got[0, 1]       # an Inf was held back
    assert np.all(np.isfinite(nr))
    assert nr[0, 2] == 8.0 and nr[0, 5] == 0.25      # finite ones carried


def test_invariant_on_random_rows():
    for P, k, seed in ((1, 1, 0), (38, 4, 1), (257, 26, 2), (300, 300, 3)):
        theta, g = cc.normal((4, P), seed), cc.normal((4, P), seed + 10, .5)
        e = cc.normal((4, P), seed + 20, 0.05)
        nt, nr, a, sent = spec.topk_rows(theta, g, e, k)
        assert np.all(sent.sum(axis=1) == k)
        for i in range(4):
            cc.check_invariant(f"P={P}", a[i], g[i], nt[i], nr[i], sent[i])


# ------------------------------------------------------- op on a CPU device

@pytest.mark.parametrize("P", [1, 2, 38, 65, 257])
def test_op_shapes(P):
    cc.case_shape(CPU, P)
    cc.case_shape(CPU, P, ef=False)


@pytest.mark.parametrize("case", [cc.case_odd_offsets, cc.case_shuffled_rows,
                                  cc.case_three_models, cc.case_hand_rows,
                                  cc.case_digits],
                         ids=lambda f: f.__name__)
def test_op_case(case):
    case(CPU)


def test_op_integer_ties():
    cc.case_integer_ties(CPU, 65)


def test_op_two_calls():
    cc.case_two_calls(CPU, 65)


def test_op_rejects_k_outside_the_row():
    bank = torch.zeros(2, 5)
    plan = compress_hip.CompressPlan([0], [0], 1)
    for k in (0, 6):
        with pytest.raises(ValueError):
            compress_hip.topk(bank, plan, torch.zeros(1, 5), None, k,
                              compress_hip.new_counts(1, CPU))


def test_infinite_bound_leaves_every_bit():
    """robust_fused=1 without a norm bound runs its clip pass with an
    infinite bound: min(1, inf / (norm + 1e-12)) is 1 for every finite norm
    and NaN for an infinite or NaN one; a row is rewritten only where the
    factor is < 1, so no row is and nothing counts as clipped."""
    from feddrift_amd.comm import robust as rb
    from feddrift_amd.ops import robust_hip
    norms = np.array([0.0, 1e-30, 1.0, 3e38], dtype=np.float32)
    assert np.all(rb.clip_scale(norms, float("inf")) == 1.0)
    assert bool(
        (rb.clip_scale(torch.from_numpy(norms), float("inf")) == 1.0).all())
    odd = np.array([np.inf, np.nan], dtype=np.float32)
    with np.errstate(all="ignore"):
        assert not np.any(rb.clip_scale(odd, float("inf")) < 1.0)
    assert not bool(
        (rb.clip_scale(torch.from_numpy(odd), float("inf")) < 1.0).any())
    bank = cc.normal((6, 38), 0)
    bank[2, 5] = np.nan
    bank[3] *= 1e30                                  # the norm overflows
    bank[4, 0] = np.inf
    glob = cc.normal((2, 38), 1)
    b = torch.from_numpy(bank.copy())
    partial = torch.zeros(2, 39)
    counts = robust_hip.new_counts(2, CPU)
    plan = robust_hip.ClipPlan(np.arange(6), np.arange(6) % 2,
                               np.ones(6, np.float32), 2)
    robust_hip.clip_accumulate(b, plan, torch.from_numpy(glob), float("inf"),
                               partial, counts)
    assert np.array_equal(cc.bits(b), cc.bits(bank))
    assert counts[:, 0].tolist() == [0, 0] and counts[:, 1].tolist() == [3, 3]
    assert partial[:, 38].tolist() == [3.0, 3.0]


# ------------------------------------------------------------------ options

@pytest.mark.parametrize("kw", [
    dict(upload_compress="top_k"), dict(upload_compress="qsgd"),
    dict(compress_ratio=0.0), dict(compress_ratio=-0.1),
    dict(compress_ratio=1.5), dict(compress_ratio=float("nan")),
    dict(compress_ratio=float("inf")),
    dict(compress_error_feedback=2), dict(compress_error_feedback=-1)])
def test_config_validation(kw):
    with pytest.raises(ValueError) as ei:
        Config(**kw)
    if "upload_compress" in kw:
        assert "none" in str(ei.value) and "topk" in str(ei.value)


def test_config_defaults():
    cfg = Config()
    assert (cfg.upload_compress, cfg.compress_ratio,
            cfg.compress_error_feedback) == ("none", 0.01, 1)
    Config(upload_compress="topk", compress_ratio=1.0,
           compress_error_feedback=0)


def test_batchnorm_model_raises(tmp_path):
    from feddrift_amd.comm import Communicator
    from feddrift_amd.data.generators import sample_cifar
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    ds = DriftDataset(data_dir="/nonexistent", dataset="cifar", num_client=2)
    rng = np.random.default_rng(0)
    for c in range(2):
        for t in range(3):
            arr = sample_cifar(8, 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    cfg = Config(model="resnet", dataset="cifar", data_dir="/nonexistent",
                 client_num_in_total=2, client_num_per_round=2, batch_size=8,
                 epochs=1, comm_round=1, total_train_iteration=2,
                 curr_train_iteration=1, concept_num=2,
                 concept_drift_algo="softcluster",
                 concept_drift_algo_arg="mmacc_06", bench_mode=1,
                 report_client=0, log_dir=str(tmp_path),
                 upload_compress="topk")
    with pytest.raises(ValueError, match="lr, fnn, cnn"):
        FLJob(cfg, Communicator(device=CPU),
              MetricLogger(enabled=False, to_file=False), dataset=ds)


# -------------------------------------------------------------------- FLJob

@pytest.mark.parametrize("ef", [0, 1])
@pytest.mark.parametrize("fused", [0, 1])
def test_fljob_against_hand_loop(tmp_path, ef, fused):
    cc.fljob_against_hand_loop(tmp_path, CPU, 3, ef, robust_fused=fused)


def test_fljob_median(tmp_path):
    cc.fljob_against_hand_loop(tmp_path, CPU, 3, 1, robust_agg="median")


def test_fljob_secure_ring(tmp_path):
    cc.fljob_against_hand_loop(tmp_path, CPU, 3, 1, secure_agg=2)


def test_fljob_clip_follows_compress(tmp_path):
    """train -> compress -> clip: with a norm bound the rows the server
    defends on are the compressed ones."""
    from feddrift_amd.comm.robust import robustify_replicas
    bound = 0.05
    A = sc.make_job(tmp_path / "a", device=CPU, n_clients=10,
                    upload_compress="topk", compress_ratio=0.1,
                    robust_norm_bound=bound)
    B = sc.make_job(tmp_path / "b", device=CPU, n_clients=10)
    ci = A.client_sampling(0)
    pa = cc_plan_train(A, ci)
    pb = cc_plan_train(B, ci)
    K = B.n_models
    glob = B.global_params.numpy()
    reps, _, _ = cc.expected(B.replicas.numpy(), glob, pb.rows, pb.rows % K,
                             np.zeros_like(B.replicas.numpy()), A._compress_k)
    reps = torch.from_numpy(reps)
    robustify_replicas(reps, B.global_params, torch.as_tensor(pb.rows),
                       torch.as_tensor(pb.rows % K), bound)
    assert np.array_equal(cc.bits(A.replicas), cc.bits(reps))
    norms = (A.replicas[pa.rows] - A.global_params[pa.rows % K]).norm(dim=1)
    assert float(norms.max()) <= bound * (1 + 1e-5)


def cc_plan_train(job, ci, r=0):
    plan = job.algo.plan(job, r, ci)
    job.train(plan)
    return plan


def test_residual_carries_into_the_next_round(tmp_path):
    A = sc.make_job(tmp_path, device=CPU, n_clients=10,
                    upload_compress="topk", compress_ratio=0.1)
    ci = A.client_sampling(0)
    assert not A._residual.any()                     # zero at job start
    p0 = cc_plan_train(A, ci, 0)
    e1 = A._residual.clone()
    assert e1[p0.rows].abs().sum() > 0
    untrained = np.setdiff1d(np.arange(e1.shape[0]), p0.rows)
    assert not e1[untrained].any()
    A.algo.aggregate(A, 0, p0, ci)
    assert torch.equal(A._residual, e1)              # aggregation keeps it
    # round 2 by hand from round 1's residual
    plan = A.algo.plan(A, 1, ci)
    saved = A._compress
    A._compress = False                              # plain training
    A.train(plan)
    A._compress = saved
    K = A.n_models
    reps, resid, _ = cc.expected(
        A.replicas.numpy(), A.global_params.numpy(), plan.rows,
        plan.rows % K, e1.numpy(), A._compress_k)
    reps0, _, _ = cc.expected(
        A.replicas.numpy(), A.global_params.numpy(), plan.rows,
        plan.rows % K, np.zeros_like(e1.numpy()), A._compress_k)
    A._compress_pass(plan)
    assert np.array_equal(cc.bits(A.replicas), cc.bits(reps))
    assert np.array_equal(cc.bits(A._residual), cc.bits(resid))
    assert not np.array_equal(cc.bits(reps), cc.bits(reps0))


def test_model_bank_operations_zero_the_right_residual_rows(tmp_path):
    A = sc.make_job(tmp_path, device=CPU, n_clients=4, k=3,
                    upload_compress="topk", compress_ratio=0.1)
    K, nW = A.n_models, len(A.owned_workers)
    assert K == 3

    def fill():
        A._residual.copy_(torch.arange(1, nW * K + 1, dtype=torch.float32)
                          .unsqueeze(1).expand(-1, A.n_params))

    def zeroed():
        return sorted(np.nonzero(~A._residual.bool().any(dim=1).numpy())[0]
                      .tolist())

    fill()
    A.reinit_model(1)
    assert zeroed() == [w * K + 1 for w in range(nW)]
    fill()
    A.copy_model(2, 0)
    assert zeroed() == [w * K + 2 for w in range(nW)]
    fill()
    A.merge_models(0, 1, 0.5, 0.5)
    assert zeroed() == []                            # a merge keeps it
    A.randomize_models_unseeded()
    assert zeroed() == list(range(nW * K))


def test_compress_stats_sum_and_reset(tmp_path):
    A = sc.make_job(tmp_path, device=CPU, n_clients=10,
                    upload_compress="topk", compress_ratio=0.1)
    ci = A.client_sampling(0)
    K, P, k = A.n_models, A.n_params, A._compress_k
    pairs = np.zeros(K, dtype=np.int64)
    for r in range(2):
        plan = cc_plan_train(A, ci, r)
        pairs += np.bincount(plan.rows % K, minlength=K)
        A.algo.aggregate(A, r, plan, ci)
    st = A.compress_stats()
    assert st.shape == (K, 2) and st.dtype == np.int64
    assert np.array_equal(st[:, 1], pairs * P)
    assert np.all(st[:, 0] >= pairs * k) and np.all(st[:, 0] <= st[:, 1])
    assert np.all(A.compress_stats() == 0)           # reset
    plain = sc.make_job(tmp_path / "p", device=CPU, n_clients=10)
    assert np.all(plain.compress_stats() == 0)


def test_sent_fraction_is_logged(tmp_path):
    A = sc.make_job(tmp_path, device=CPU, n_clients=10,
                    upload_compress="topk", compress_ratio=0.1)
    seen = {}
    A.logger.log = lambda d, step: seen.update(d)
    ci = A.client_sampling(0)
    plan = cc_plan_train(A, ci)
    A.algo.aggregate(A, 0, plan, ci)
    tr, te = A.client_eval(np.zeros(10, dtype=np.int64))
    A.cfg.report_client = 0
    A.log_round_stats(0, tr, te)
    keys = [k for k in seen if k.startswith("Compress/SentFrac-m")]
    assert keys and all(0 < seen[k] <= 1 for k in keys)


@pytest.mark.parametrize("fused", [0, 1])
def test_none_is_the_plain_round(tmp_path, fused):
    """upload_compress=none (spelled out) against a job built without the
    option: global rows bit-equal over three rounds, no residual bank."""
    A = sc.make_job(tmp_path / "a", device=CPU, n_clients=10,
                    upload_compress="none", robust_fused=fused)
    B = sc.make_job(tmp_path / "b", device=CPU, n_clients=10,
                    robust_fused=fused)
    assert A._residual is None and not A._compress
    assert not hasattr(A, "_compress_counts")
    ci = A.client_sampling(0)
    for r in range(3):
        for j in (A, B):
            plan = cc_plan_train(j, ci, r)
            j.algo.aggregate(j, r, plan, ci)
        assert np.array_equal(cc.bits(A.global_params),
                              cc.bits(B.global_params))
        assert np.array_equal(cc.bits(A.replicas), cc.bits(B.replicas))
