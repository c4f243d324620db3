"""upload_compress=quant and topk_quant on the CPU: the specification
(comm/compress.py:quant_rows), the options, the wire-bit count and FLJob on
the CPU backend. Shared bodies: tests/quant_cases.py."""

import numpy as np
import pytest
import torch

import quant_cases as qc
import secagg_cases as sc
from feddrift_amd.comm import compress as spec
from feddrift_amd.comm import robust as rb
from feddrift_amd.comm.secure_agg import job_key, philox4x32
from feddrift_amd.config import Config

CPU = torch.device("cpu")


# ------------------------------------------------------------ specification

@pytest.mark.parametrize("case", qc.hand_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("k", [0, 2])
def test_hand_rows(case, k):
    qc.check_hand_case(*case, k=k)


def test_ternary_row_over_many_passes():
    """b = 2 on a = [1, -1, 0.5, 0, -0.25]: +-1 come back exactly, 0 never
    travels, the others take both values of {0, sign}."""
    name, theta, g, e, nbits, _ = qc.hand_cases()[0]
    seen = {2: set(), 4: set()}
    for c in range(64):
        nt, _, _, travel, q, written, _, _ = qc.spec_rows(
            theta, g, e, 0, nbits, [0], [0], c)
        assert nt[0, 0] == 1.0 and nt[0, 1] == -1.0
        assert not travel[0, 3] and not written[0, 3]
        for j in seen:
            assert q[0, j] in (0.0, 1.0)
            seen[j].add(float(nt[0, j]))
    assert seen[2] == {0.0, 1.0} and seen[4] == {0.0, -1.0}


@pytest.mark.parametrize("P", [1, 3, 38, 257])
@pytest.mark.parametrize("nbits", [2, 4, 8, 16])
@pytest.mark.parametrize("ef", [0, 1])
def test_invariants_on_random_rows(P, nbits, ef):
    n = 4
    theta = qc.normal((n, P), P + nbits)
    g = qc.normal((n, P), P + nbits + 1, 0.5)
    e = qc.normal((n, P), P + nbits + 2, 0.05) if ef else None
    for k in sorted({0, 1, spec.keep_count(0.1, P), P}):
        out = qc.spec_rows(theta, g, e, k, nbits, np.arange(n) + 3,
                           np.arange(n) % 2, 9)
        qc.check_invariants(f"P={P} b={nbits} k={k}", theta, g, e, k, nbits,
                            out)


@pytest.mark.parametrize("nbits", [2, 8])
def test_clamp_is_reachable(nbits):
    """x = L and u = 1 - 2^-24: fl32(x + u) is L + 1, and q is L."""
    L = spec.levels(nbits)
    u = qc.clamp_draw()
    assert np.floor(np.float32(np.float32(L) + u)) == L + 1
    name, theta, g, e, _, ctr = qc.hand_cases()[-1]
    assert name == "clamp"
    qc.check_hand_case(name, theta, g, e, nbits, ctr)


@pytest.mark.parametrize("nbits", [2, 4, 8])
def test_specification_is_unbiased(nbits):
    """One row of P = 38 over passes 0 .. 4095. Every draw lies within one
    step s / L of a_j, so its variance is at most (s / L)^2 / 4 and the
    mean of 4096 stays within 6 standard errors; the keys are fixed.
    Measured: 0.31, 0.30 and 0.26 of the bound at b = 2, 4, 8."""
    P, n = 38, 4096
    a = qc.normal((1, P), 77)
    z = np.zeros((1, P), np.float32)
    L = spec.levels(nbits)
    u = np.concatenate([spec.quant_uniform(qc.KEY, c, [4], [1], P)
                        for c in range(n)])
    out = spec.quant_rows(np.repeat(a, n, 0), np.repeat(z, n, 0), None, 0,
                          nbits, u)
    s = float(out[6][0])
    assert s == np.abs(a).max()
    err = np.abs(out[0].astype(np.float64).mean(axis=0) - a[0]).max()
    bound = 6 * s / (2 * L * np.sqrt(n))
    print(f"b={nbits}: max |mean(v) - a| = {err:.3e}, bound {bound:.3e}, "
          f"ratio {err / bound:.2f}")
    assert err <= bound


# ------------------------------------------------------------------ streams

def _draws(key=qc.KEY, ctr=0, w=0, m=0, P=64):
    return spec.quant_uniform(key, ctr, [w], [m], P)[0]


def test_draws_lie_in_the_unit_interval_with_24_bits():
    u = _draws(P=1001)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))
    assert np.all(u * np.float32(2 ** 24) == np.floor(u * np.float32(2 ** 24)))
    assert 0.4 < u.mean() < 0.6


def test_draw_layout():
    """Coordinate j takes word j % 4 of the block at (j // 4, w, m, c)."""
    key, c, w, m = qc.KEY, 11, 5, 1
    k = np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint64)
    u = _draws(ctr=c, w=w, m=m, P=10)
    for j in (0, 1, 6, 9):
        x = philox4x32(np.array([j // 4, w, m, c], np.uint64), k)[j % 4]
        assert u[j] == np.float32(x >> 8) * np.float32(2.0 ** -24)


def test_streams_are_separate():
    base = _draws()
    assert not np.array_equal(base, _draws(key=spec.quant_key(7, 4)))
    assert not np.array_equal(base, _draws(key=spec.quant_key(8, 3)))
    assert not np.array_equal(base, _draws(ctr=1))
    assert not np.array_equal(base, _draws(ctr=1 << 16))
    assert not np.array_equal(base, _draws(w=1))
    assert not np.array_equal(base, _draws(m=1))
    assert not np.array_equal(_draws(w=1), _draws(m=1))
    # not the aggregation noise's stream: another key, and other words
    assert spec.quant_key(7, 3) != job_key(7, 3) == rb.noise_key(7, 3)
    bare = _draws(key=job_key(7, 3))
    assert not np.array_equal(base, bare)
    assert 0 <= spec.quant_key(7, 3) < 2 ** 64


# ---------------------------------------------------------------- wire bits

def test_wire_bits():
    # P = 1000: 10 index bits
    assert spec.wire_bits("topk", 50, 3, 1000, 4) == 50 * 42
    assert spec.wire_bits("quant", 2900, 3, 1000, 4) == 3 * (32 + 4000)
    assert spec.wire_bits("topk_quant", 50, 3, 1000, 4) == 96 + 50 * 14
    # ceil(log2 P) at and around a power of two, and a row of one
    assert spec.wire_bits("topk", 1, 1, 1024, 8) == 32 + 10
    assert spec.wire_bits("topk", 1, 1, 1025, 8) == 32 + 11
    assert spec.wire_bits("topk", 1, 1, 1, 8) == 32
    with pytest.raises(ValueError):
        spec.wire_bits("none", 0, 0, 10, 8)


# ------------------------------------------------------------------ options

def test_config_defaults_and_kinds():
    cfg = Config()
    assert (cfg.upload_compress, cfg.compress_bits) == ("none", 8)
    assert spec.KINDS == ("none", "topk", "quant", "topk_quant")
    for kind in spec.KINDS:
        for b in (2, 16):
            Config(upload_compress=kind, compress_bits=b)
    assert [spec.levels(b) for b in (2, 4, 8, 16)] == [1, 7, 127, 32767]


@pytest.mark.parametrize("b", [1, 0, -8, 17, 32, 8.0, 7.5, "8", None, True,
                               float("nan")])
def test_invalid_compress_bits(b):
    with pytest.raises(ValueError, match="compress_bits"):
        Config(compress_bits=b)


def test_cli_reads_the_options():
    from feddrift_amd.config import config_from_argv
    cfg = config_from_argv(["--upload_compress", "topk_quant",
                            "--compress_bits", "4"])
    assert (cfg.upload_compress, cfg.compress_bits) == ("topk_quant", 4)


def test_quant_ignores_compress_ratio(tmp_path):
    A = sc.make_job(tmp_path / "a", device=CPU, upload_compress="quant",
                    compress_ratio=0.5)
    B = sc.make_job(tmp_path / "b", device=CPU, upload_compress="quant",
                    compress_ratio=0.01)
    assert A._compress_k == B._compress_k == 0
    ci = A.client_sampling(0)
    for j in (A, B):
        j.train(j.algo.plan(j, 0, ci))
    assert np.array_equal(qc.bits(A.replicas), qc.bits(B.replicas))
    assert np.array_equal(qc.bits(A._residual), qc.bits(B._residual))


@pytest.mark.parametrize("kind", ["quant", "topk_quant"])
def test_batchnorm_model_raises(tmp_path, kind):
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
                 upload_compress=kind)
    with pytest.raises(ValueError, match="lr, fnn, cnn"):
        FLJob(cfg, Communicator(device=CPU),
              MetricLogger(enabled=False, to_file=False), dataset=ds)


# -------------------------------------------------------------------- FLJob

@pytest.mark.parametrize("kind", ["quant", "topk_quant"])
@pytest.mark.parametrize("ef", [0, 1])
@pytest.mark.parametrize("fused", [0, 1])
def test_fljob_against_hand_loop(tmp_path, kind, ef, fused):
    qc.fljob_against_hand_loop(tmp_path, CPU, 3, kind, ef,
                               robust_fused=fused)


def test_fljob_median(tmp_path):
    qc.fljob_against_hand_loop(tmp_path, CPU, 3, "topk_quant", 1,
                               robust_agg="median")


def test_fljob_secure_ring(tmp_path):
    qc.fljob_against_hand_loop(tmp_path, CPU, 3, "quant", 1, nbits=8,
                               secure_agg=2)


def test_reinit_model_zeroes_the_residual(tmp_path):
    A = sc.make_job(tmp_path, device=CPU, n_clients=4, k=3,
                    upload_compress="quant", compress_bits=2)
    K, nW = A.n_models, len(A.owned_workers)
    ci = A.client_sampling(0)
    A.train(A.algo.plan(A, 0, ci))
    assert A._residual.abs().sum() > 0               # the rounding error
    A._residual.fill_(1.0)
    A.reinit_model(1)
    zero = ~A._residual.bool().any(dim=1).numpy()
    assert sorted(np.nonzero(zero)[0].tolist()) == \
        [w * K + 1 for w in range(nW)]
    A._residual.fill_(1.0)
    A.merge_models(0, 1, 0.5, 0.5)
    assert A._residual.bool().all()                  # a merge keeps it


@pytest.mark.parametrize("kind", ["topk", "quant", "topk_quant"])
def test_empty_plan_still_advances_the_counter(tmp_path, kind):
    import copy
    A = sc.make_job(tmp_path, device=CPU, n_clients=10, upload_compress=kind)
    ci = A.client_sampling(0)
    plan = A.algo.plan(A, 0, ci)
    empty = copy.copy(plan)
    empty.rows = plan.rows[:0]
    empty.template = None
    before = A.replicas.clone()
    assert A._compress_ctr == 0
    A.train(empty)
    assert A._compress_ctr == 1
    assert np.all(A.compress_stats() == 0)
    A.train(plan)
    assert A._compress_ctr == 2
    assert not torch.equal(A.replicas, before)
    # a plain job has no counter to advance
    B = sc.make_job(tmp_path / "b", device=CPU, n_clients=10)
    B.train(copy.copy(empty))
    assert not hasattr(B, "_compress_ctr")


@pytest.mark.parametrize("kind,nbits", [("topk", 8), ("quant", 4),
                                        ("topk_quant", 4)])
def test_stats_and_wire_fraction_are_logged(tmp_path, kind, nbits):
    """compress_stats() against the hand loop is checked every round of
    fljob_against_hand_loop; here the logged fractions follow from the
    same counters."""
    A, _, _ = qc.fljob_against_hand_loop(tmp_path, CPU, 1, kind, 1,
                                         nbits=nbits) \
        if kind != "topk" else (sc.make_job(
            tmp_path, device=CPU, n_clients=10, upload_compress="topk",
            compress_ratio=0.1), None, None)
    seen = {}
    A.logger.log = lambda d, step: seen.update(d)
    ci = A.client_sampling(0)
    plan = A.algo.plan(A, 1, ci)
    A.train(plan)
    A.algo.aggregate(A, 1, plan, ci)
    want = A._compress_counts.numpy().copy()         # world 1: not drained
    tr, te = A.client_eval(np.zeros(10, dtype=np.int64))
    A.log_round_stats(1, tr, te)
    K, P = A.n_models, A.n_params
    n = 0
    for m in range(K):
        if want[m, 1] == 0:
            continue
        n += 1
        assert seen[f"Compress/SentFrac-m{m}"] == want[m, 0] / want[m, 1]
        wire = spec.wire_bits(kind, want[m, 0], want[m, 1] // P, P, nbits)
        assert seen[f"Compress/WireFrac-m{m}"] == wire / (32 * want[m, 1])
        assert 0 < seen[f"Compress/WireFrac-m{m}"] < 1
    assert n > 0
    assert np.all(A.compress_stats() == 0)           # drained by the log


def test_none_logs_no_fraction(tmp_path):
    A = sc.make_job(tmp_path, device=CPU, n_clients=10)
    seen = {}
    A.logger.log = lambda d, step: seen.update(d)
    ci = A.client_sampling(0)
    plan = A.algo.plan(A, 0, ci)
    A.train(plan)
    A.algo.aggregate(A, 0, plan, ci)
    tr, te = A.client_eval(np.zeros(10, dtype=np.int64))
    A.log_round_stats(0, tr, te)
    assert not [k for k in seen if k.startswith("Compress/")]
