"""Shared cases for the Multi-Krum aggregation tests (tests/test_krum.py on
the CPU against the specification path of ops/krum_hip.py,
tests/test_gpu_krum.py against the HIP kernels). Every case takes `dev`,
builds its bank on the host, runs krum_hip.aggregate on `dev` and checks
what it gets back against comm.robust's float64 specification.

Bound rule (PARITY.md, "Multi-Krum aggregation"); u53 = 2^-53, u24 = 2^-24.
All bounds are derived, none measured.

  distances  |D - D_spec| <= 2 (P + 2) u53 D_spec: the terms are
             non-negative, difference and square cost at most 2 roundings
             and the sum at most P in any order, once on each side. +Inf
             matches exactly, the diagonal is exactly 0.
  scores     relative error <= 2 (P + q + 2) u53; +Inf matches exactly.
  selection  compared as the CONTENTS of the selected rows in order
             (identical rows are interchangeable).
  near ties  an input is valid only if every pair of distinct adjacent
             sorted float64 scores differs by at least 1000 x the score
             bound, relative; asserted from the specification before the
             device's result is looked at. Exact ties are resolved by ids.
  output     s = 1: the selected row's bits. s > 1, against the float64
             mean of the selected rows: u24 (sum_i |x_i| + 2 |mean|) per
             coordinate (a sequential float32 sum of s terms, the division
             and the store).

Every general check prints its figures as a FIG line before it asserts."""

import numpy as np
import torch

from feddrift_amd.comm import robust as rb
from feddrift_amd.ops import krum_hip

U53 = 2.0 ** -53
U24 = 2.0 ** -24
SENTINEL = np.float32(-123.456)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def normal(n, P, seed, scale=0.1):
    return (np.random.default_rng(seed).standard_normal((n, P)) * scale
            ).astype(np.float32)


def score_bound(P, q):
    return 2.0 * (P + q + 2) * U53


def assert_no_near_tie(case, scores, P, q):
    """The near-tie guard: distinct adjacent sorted scores are at least
    1000 score bounds apart (relative). Exact ties pass."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    s = s[np.isfinite(s)]
    lo, hi = s[:-1], s[1:]
    distinct = hi != lo
    if not distinct.any():
        return
    gap = ((hi - lo) / hi)[distinct]
    assert gap.min() >= 1000.0 * score_bound(P, q), \
        (case, "near tie in the test's own input", float(gap.min()))


def spec_model(values, ids, frac, select):
    """The float64 specification of one model's participants [n, P]."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    n = len(values)
    f, q, s = rb.krum_counts(n, frac, select)
    D = rb.krum_sqdist(values)
    scores = rb.krum_scores(D, f)
    pos = rb.krum_select(scores, ids, s)
    kept = values[pos].astype(np.float64)
    mean = kept.sum(axis=0) / s
    bound = U24 * (np.abs(kept).sum(axis=0) + 2.0 * np.abs(mean))
    return dict(n=n, f=f, q=q, s=s, D=D, scores=scores, pos=pos, mean=mean,
                bound=bound)


def run(dev, bank, rows, models, weights, ids, K, frac, select, out=None,
        scratch_rows=None):
    """krum_hip.aggregate on `dev`. Returns (out [K, P] float32, plan,
    selected ids per model, scores per model); rows the op does not fill
    hold SENTINEL. Asserts the bank kept its bits."""
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    P = bank.shape[1]
    bank_t = torch.from_numpy(bank.copy()).to(dev)
    out_t = torch.full((K, P + 1), float(SENTINEL), device=dev)
    if out is not None:
        out_t[:, :P] = torch.from_numpy(out).to(dev)
    plan = krum_hip.KrumPlan(rows, models, weights, K, frac, select, ids)
    krum_hip.aggregate(bank_t, plan, out_t[:, :P], scratch_rows=scratch_rows)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert np.array_equal(bits(bank_t.cpu().numpy()), bits(bank)), \
        "the op wrote to the bank"
    res = out_t.cpu().numpy()
    assert np.all(res[:, P] == SENTINEL), "the op wrote past column P"
    chosen, scores = krum_hip.last_selection(plan, with_scores=True)
    return res[:, :P], plan, chosen, scores


def check_model(case, values, ids, frac, select, got_out, got_chosen,
                got_scores, got_D=None):
    """One model's results against the rules above. `values`, `ids` are the
    participants in the plan's order."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    n, P = values.shape
    sp = spec_model(values, ids, frac, select)
    q, s = sp["q"], sp["s"]
    assert_no_near_tie(case, sp["scores"], P, q)
    if got_D is not None:
        Ds = sp["D"]
        assert got_D.shape == Ds.shape
        assert np.all(np.diag(got_D) == 0.0), (case, "diagonal")
        assert np.array_equal(bits64(got_D), bits64(got_D.T)), \
            (case, "D[i, j] and D[j, i] differ")
        inf = np.isinf(Ds)
        assert np.array_equal(np.isposinf(got_D), inf), (case, "+Inf")
        err = np.abs(got_D[~inf] - Ds[~inf])
        lim = 2.0 * (P + 2) * U53 * Ds[~inf]
        rel = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.
        print(f"FIG {case} | D n={n} P={P} | err/bound {rel:.3f}")
        assert np.all(err <= lim), (case, "distance", rel)
    got_scores = np.asarray(got_scores, dtype=np.float64)
    inf = np.isinf(sp["scores"])
    assert np.array_equal(np.isposinf(got_scores), inf), (case, "score +Inf")
    err = np.abs(got_scores[~inf] - sp["scores"][~inf])
    lim = score_bound(P, q) * sp["scores"][~inf]
    rel = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print(f"FIG {case} | scores n={n} q={q} | err/bound {rel:.3f}")
    assert np.all(err <= lim), (case, "score", rel)
    # selection: the contents of the selected rows, in order
    assert len(got_chosen) == s, (case, "selection size")
    by_id = {int(i): k for k, i in enumerate(ids)}
    assert len(by_id) == n, (case, "the test's ids are not unique")
    got_pos = np.array([by_id[int(i)] for i in got_chosen], dtype=np.int64)
    assert np.array_equal(bits(values[got_pos]), bits(values[sp["pos"]])), \
        (case, "selection", got_pos, sp["pos"])
    got_out = np.ascontiguousarray(got_out, dtype=np.float32)
    if s == 1:
        assert np.array_equal(bits(got_out), bits(values[sp["pos"][0]])), \
            (case, "s = 1 bits")
    elif np.all(np.isfinite(sp["mean"])):
        err = np.abs(got_out.astype(np.float64) - sp["mean"])
        rel = float((err / np.maximum(sp["bound"], 1e-300)).max())
        print(f"FIG {case} | output s={s} | err/bound {rel:.3f}")
        assert np.all(np.isfinite(got_out)), (case, "result not finite")
        assert np.all(err <= sp["bound"]), (case, "output", rel)
    return sp


def one_model(dev, case, values, frac, select, ids=None, seed=0,
              scratch_rows=None, check_D=True):
    """values [n, P] as the only model's participants, laid out as shuffled
    rows of a bank with holes. Checks everything and returns (out row,
    scores, selected ids, specification dict)."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    n, P = values.shape
    rng = np.random.default_rng(seed)
    R = 2 * n + 3
    rows = rng.choice(R, size=n, replace=False).astype(np.int64)
    bank = (rng.standard_normal((R, P)) * 0.3).astype(np.float32)
    bank[rows] = values
    if ids is None:
        ids = 10 + rng.permutation(n)
    ids = np.asarray(ids, dtype=np.int64)
    out, plan, chosen, scores = run(
        dev, bank, rows, np.zeros(n, np.int64), np.ones(n, np.float32), ids,
        1, frac, select, scratch_rows=scratch_rows)
    assert plan.n[0] == n
    D = None
    if dev.type == "cuda" and check_D and plan._scratch[1] >= n:
        D = krum_hip.last_distances(plan, 0)
    sp = check_model(case, values, ids, frac, select, out[0], chosen[0],
                     scores[0], D)
    assert (plan.f[0], plan.q[0], plan.s[0]) == (sp["f"], sp["q"], sp["s"])
    return out[0], scores[0], chosen[0], sp


# ------------------------------------------------------------- n and P edges

def n_edge_list(tile):
    return [(n, 19, sel) for n in (1, 2, 3, 4, 5, tile - 1, tile, tile + 1,
                                   2 * tile + 1) for sel in (0, 1)]


def p_edge_list(tile, chunk):
    return [(n, P, sel) for n in (5, tile + 1)
            for P in (1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1)
            for sel in (0, 1)]


def case_shape(dev, n, P, select, scale=0.1):
    one_model(dev, f"shape n={n} P={P} select={select}",
              normal(n, P, n * 131 + P, scale), 0.2, select, seed=n + P)


def cnn_p():
    from feddrift_amd.models import zoo
    from feddrift_amd.models.generic_packer import ModulePacker
    return ModulePacker(zoo.CNN_DropOut()).n_params


def case_cnn(dev, select):
    P = cnn_p()
    one_model(dev, f"CNN P={P} n=10 select={select}", normal(10, P, 77),
              0.2, select)


# ---------------------------------------------------------------- slab seams

def case_slab_seams(dev):
    """n = 17 under scratch_rows 1, 5, 16, 17: bit-identical scores,
    selection and output to the unslabbed launch."""
    vals = normal(17, 23, 5)
    ids = 10 + np.random.default_rng(1).permutation(17)
    ref = one_model(dev, "slab whole", vals, 0.2, 0, ids=ids)
    for sr in (1, 5, 16, 17):
        got = one_model(dev, f"slab {sr}", vals, 0.2, 0, ids=ids,
                        scratch_rows=sr)
        assert np.array_equal(bits64(got[1]), bits64(ref[1])), (sr, "scores")
        assert np.array_equal(got[2], ref[2]), (sr, "selection")
        assert np.array_equal(bits(got[0]), bits(ref[0])), (sr, "output")


def case_mutual_nearest_tie(dev, scratch_rows=None):
    """n = 3, f = 0, q = 1: the two mutually nearest rows tie exactly, D
    being symmetric — under scratch_rows = 1 only if D[i, j] and D[j, i],
    computed in different passes, are one value. The lower id wins;
    swapping the ids swaps the winner."""
    vals = normal(3, 19, 11)
    vals[1] = vals[0] + np.float32(0.01) * normal(1, 19, 12)[0]
    vals[2] += np.float32(1.0)
    for ids in ([7, 9, 3], [9, 7, 3]):
        out, scores, chosen, sp = one_model(
            dev, f"tie ids={ids}", vals, 0.2, 1, ids=ids,
            scratch_rows=scratch_rows)
        assert sp["q"] == 1 and sp["s"] == 1
        assert bits64(scores)[0] == bits64(scores)[1], "no exact tie"
        assert scores[2] > scores[0]
        assert int(chosen[0]) == 7
        assert np.array_equal(bits(out), bits(vals[ids.index(7)]))


# ------------------------------------------------------------ several models

def case_three_models(dev, tile=32):
    """Participant counts (tile + 5, 0, 3) in one launch, the bank rows
    permuted, one zero-weight pair per non-empty model (far off: taking it
    in would change the result); the empty model keeps a sentinel's bits."""
    P, K = 19, 3
    ns = [tile + 5, 0, 3]
    vals = [normal(n, P, 40 + i) for i, n in enumerate(ns)]
    extra = np.full((2, P), 50.0, np.float32)
    bank = np.concatenate(vals + [extra])
    U = len(bank)
    rng = np.random.default_rng(0)
    perm = rng.permutation(U)
    inv = np.argsort(perm)                 # pair i lies at bank row inv[i]
    models = np.concatenate([np.full(n, m) for m, n in enumerate(ns)]
                            + [[0, 2]])
    weights = np.concatenate([np.ones(U - 2, np.float32), [0.0, 0.0]])
    ids = 100 + rng.permutation(U)
    order = rng.permutation(U)             # the pair order is shuffled too
    prev = normal(K, P, 9)
    out, plan, chosen, scores = run(
        dev, bank[perm], inv[order], models[order], weights[order],
        ids[order], K, 0.2, 0, out=prev)
    assert list(plan.n) == ns
    assert np.array_equal(bits(out[1]), bits(prev[1]))
    assert len(chosen[1]) == 0
    for m in (0, 2):
        part = (models[order] == m) & (weights[order] > 0)
        v = bank[np.arange(U)[order][part]]
        check_model(f"three models m={m}", v, ids[order][part], 0.2, 0,
                    out[m], chosen[m], scores[m])


# ----------------------------------------------------------- identical rows

def case_duplicate_honest_rows(dev):
    """Two honest rows are duplicated: their scores are bit-equal, and the
    output does not depend on which copy is picked (check_model compares
    contents)."""
    vals = normal(12, 21, 3)
    vals[4] = vals[1]
    vals[9] = vals[6]
    _, scores, _, _ = one_model(dev, "duplicate rows", vals, 0.2, 0)
    assert bits64(scores)[4] == bits64(scores)[1]
    assert bits64(scores)[9] == bits64(scores)[6]
    one_model(dev, "duplicate rows krum", vals, 0.2, 1)


def collusion_rows(n, P, seed=0):
    """8-of-10 style: honest rows 0.1 N(0, 1); f = floor(0.2 n) colluders
    all upload the honest mean + 0.15. Returns (values, honest mask)."""
    f = rb.krum_f(0.2, n)
    rng = np.random.default_rng(seed)
    honest = (0.1 * rng.standard_normal((n - f, P))).astype(np.float32)
    evil = (honest.astype(np.float64).mean(axis=0) + 0.15).astype(np.float32)
    vals = np.concatenate([honest, np.repeat(evil[None], f, axis=0)])
    mask = np.arange(n) < n - f
    perm = rng.permutation(n)
    return vals[perm], mask[perm]


COLLUSION_SHAPES = [(10, 257), (20, 38), (5, 1025)]
# At P = 38 the honest distances (0.02 chi^2_38, spread 23 %) overlap the
# colluders' margin: of the seeds 0..39 the float64 specification separates
# the two sets at 14 (at all 40 for the two longer shapes). The draw is
# chosen where the specification does; what is under test is that the op
# follows the specification there.
COLLUSION_SEED = {(10, 257): 0, (20, 38): 1, (5, 1025): 0}


def case_collusion(dev, n, P):
    """Colluders inside the honest per-coordinate range: Multi-Krum selects
    exactly the honest set and returns its mean; the trimmed mean at 0.2
    keeps them and moves by more than 0.02 per coordinate on average."""
    vals, honest = collusion_rows(n, P, COLLUSION_SEED[(n, P)])
    f = int((~honest).sum())
    assert f == rb.krum_f(0.2, n) and f >= 1
    ids = 10 + np.arange(n)
    out, scores, chosen, sp = one_model(dev, f"collusion n={n} P={P}", vals,
                                        0.2, 0, ids=ids)
    assert sorted(int(i) for i in chosen) == \
        sorted(int(i) for i in ids[honest])
    # identical colluders are at distance 0 of each other, still rejected
    evil = np.nonzero(~honest)[0]
    assert np.all(sp["D"][np.ix_(evil, evil)] == 0.0)
    assert scores[evil].min() > scores[honest].max()
    hmean = vals[honest].astype(np.float64).mean(axis=0)
    kept = np.abs(vals[honest].astype(np.float64)).sum(axis=0)
    assert np.all(np.abs(out.astype(np.float64) - hmean)
                  <= U24 * (kept + 2.0 * np.abs(hmean)))
    trimmed = rb.order_stat_mean(vals, rb.trim_count("trimmed_mean", 0.2, n))
    shift = float((trimmed - hmean).mean())
    print(f"FIG collusion n={n} P={P} | trimmed mean above honest mean by "
          f"{shift:.4f} per coordinate | colluder score "
          f"{scores[evil].min():.2f} | honest max {scores[honest].max():.2f}")
    assert shift > 0.02


# ---------------------------------------------------------- non-finite rows

def case_nonfinite_rows(dev):
    """A NaN row, a +Inf row and a -Inf row among 16: +Inf scores exactly,
    never selected (s = 13 = the finite rows); run() checks the bank."""
    vals = normal(16, 19, 6)
    vals[2, 5] = np.nan
    vals[7, :] = np.inf
    vals[11, 0] = -np.inf
    ids = 10 + np.arange(16)
    for select in (0, 1):
        out, scores, chosen, sp = one_model(dev, "non-finite rows", vals,
                                            0.2, select, ids=ids)
        assert sp["f"] == 3
        assert np.all(np.isposinf(scores[[2, 7, 11]]))
        assert np.isfinite(np.delete(scores, [2, 7, 11])).all()
        assert not {12, 17, 21} & {int(i) for i in chosen}
        assert np.all(np.isfinite(out))


def case_determinism(dev):
    vals = normal(40, 37, 10)
    ids = 10 + np.arange(40)
    a = one_model(dev, "determinism a", vals, 0.2, 0, ids=ids, seed=1)
    b = one_model(dev, "determinism b", vals, 0.2, 0, ids=ids, seed=1)
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert np.array_equal(bits64(a[1]), bits64(b[1]))
    assert np.array_equal(a[2], b[2])


def case_permutation_invariance(dev):
    """The result does not depend on where the rows lie or in which order
    the pairs are listed, when the ids travel with the rows: bit for bit."""
    vals = normal(11, 29, 13)
    ids = 10 + np.random.default_rng(2).permutation(11)
    ref = one_model(dev, "permutation a", vals, 0.2, 0, ids=ids, seed=1)
    perm = np.random.default_rng(3).permutation(11)
    got = one_model(dev, "permutation b", vals[perm], 0.2, 0, ids=ids[perm],
                    seed=2)
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(bits(got[0]), bits(ref[0]))
    assert np.array_equal(bits64(got[1]), bits64(ref[1][perm]))


OP_CASES = [case_slab_seams, case_mutual_nearest_tie, case_three_models,
            case_duplicate_honest_rows, case_nonfinite_rows,
            case_determinism, case_permutation_invariance]


# -------------------------------------------------------------------- FLJob

def job_participants(job, plan):
    """Per model: (replica rows, global worker ids) of the participants in
    the plan's order."""
    K = job.n_models
    sn = np.asarray(plan.sample_num)
    w = sn[plan.rows // K, plan.rows % K]
    own = np.asarray(job.owned_workers, dtype=np.int64)
    part = plan.rows[w > 0]
    return [(part[part % K == m], own[part[part % K == m] // K])
            for m in range(K)]


def job_stat_and_bound(job, plan, frac, select):
    """float64 Multi-Krum [K, P], its per-element output bound, the mask of
    models with participants and the selected worker ids per model, from a
    job's replicas and plan. Asserts the near-tie guard."""
    reps = job.replicas.detach().cpu().numpy()
    K, P = job.n_models, reps.shape[1]
    stat, bound = np.zeros((K, P)), np.zeros((K, P))
    upd = np.zeros(K, dtype=bool)
    kept = []
    for m, (rows, wid) in enumerate(job_participants(job, plan)):
        if len(rows) == 0:
            kept.append(np.zeros(0, dtype=np.int64))
            continue
        sp = spec_model(reps[rows], wid, frac, select)
        assert_no_near_tie(f"fljob m={m}", sp["scores"], P, sp["q"])
        upd[m] = True
        stat[m], bound[m] = sp["mean"], sp["bound"]
        kept.append(wid[sp["pos"]])
    return stat, bound, upd, kept


def fljob_poison(tmp_path, device, use_hip="auto", n_clients=10):
    """K = 2, fnn, one round: after `train`, one participant's replica row
    is overwritten with 1e6 (n = 5 per model, f = 1, s = 4). Multi-Krum
    leaves the victim's worker out, names the others in krum_selection()
    and returns their mean within the output bound; the plain mean of the
    same rows is off by > 1e4. Totals are the weight sums and the replicas
    keep every bit."""
    import secagg_cases as sc
    res = {}
    for agg in ("multi_krum", "mean"):
        job = sc.make_job(tmp_path / agg, device=device, n_clients=n_clients,
                          robust_agg=agg, use_hip_kernels=use_hip)
        ci = job.client_sampling(0)
        plan = job.algo.plan(job, 0, ci)
        job.train(plan)
        sc.torch_sync(job)
        K = job.n_models
        parts = job_participants(job, plan)
        vm = int(np.argmax([len(r) for r, _ in parts]))
        victim, victim_worker = int(parts[vm][0][0]), int(parts[vm][1][0])
        job.replicas[victim] = 1e6
        if agg == "mean":
            job._partial_fused = False     # sum the rows as they are now
        reps = job.replicas.detach().cpu().numpy().copy()
        before = job.global_params.detach().cpu().numpy().copy()
        stat, bound, upd, kept = job_stat_and_bound(job, plan, 0.2, 0)
        totals = job.aggregate(plan)
        sc.torch_sync(job)
        got = job.global_params.detach().cpu().numpy()
        sum_w = np.asarray(plan.sample_num, dtype=np.float64) \
            .reshape(-1, K).sum(axis=0)
        assert np.array_equal(totals.cpu().numpy().astype(np.float64), sum_w)
        assert np.array_equal(bits(job.replicas.cpu().numpy()), bits(reps))
        res[agg] = (got, before)
        if agg == "mean":
            assert all(len(s) == 0 for s in job.krum_selection())
            continue
        picked = job.krum_selection()
        assert upd.any()
        for m in range(K):
            if not upd[m]:
                assert np.array_equal(bits(got[m]), bits(before[m]))
                assert len(picked[m]) == 0
                continue
            assert np.array_equal(picked[m], kept[m]), (m, picked[m], kept[m])
            err = np.abs(got[m].astype(np.float64) - stat[m])
            print(f"FIG fljob multi_krum {device.type} m={m} | err/bound "
                  f"{float((err / bound[m]).max()):.3f}")
            assert np.all(err <= bound[m])
        assert victim_worker not in {int(i) for i in picked[vm]}
        assert len(picked[vm]) == len(parts[vm][0]) - 1
    assert np.abs(res["mean"][0][vm] - res["multi_krum"][0][vm]).max() > 1e4


def cnn_job(tmp_path, device=None, n_clients=4, **cfg_kw):
    """An MNIST-shaped CNN job (secagg_cases.make_job builds the fnn only):
    the module path on a CPU device, the CNN kernel engine on a GPU."""
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_mnist
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    ds = DriftDataset(data_dir="/nonexistent", dataset="MNIST",
                      num_client=n_clients)
    rng = np.random.default_rng(0)
    for c in range(n_clients):
        for t in range(3):
            arr = sample_mnist(40, 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    cfg = Config(model="cnn", dataset="MNIST", data_dir="/nonexistent",
                 client_num_in_total=n_clients,
                 client_num_per_round=n_clients, batch_size=20, epochs=1,
                 comm_round=1, total_train_iteration=2,
                 curr_train_iteration=1, concept_num=2,
                 concept_drift_algo="softcluster",
                 concept_drift_algo_arg="mmacc_06", bench_mode=1,
                 report_client=0, log_dir=str(tmp_path), lr=0.01, **cfg_kw)
    comm = Communicator(device=device) if device is not None \
        else Communicator()
    return FLJob(cfg, comm, MetricLogger(enabled=False, to_file=False),
                 dataset=ds)


def fljob_cnn_round(tmp_path, device=None):
    """One CNN round under multi_krum with a poisoned upload, at 10 clients:
    the smallest fleet at which a model has the 5 participants that
    krum_f needs to leave one out. The updated rows are the mean of the
    kept uploads within the output bound."""
    import secagg_cases as sc
    job = cnn_job(tmp_path, device=device, n_clients=10,
                  robust_agg="multi_krum")
    ci = job.client_sampling(0)
    plan = job.algo.plan(job, 0, ci)
    job.train(plan)
    sc.torch_sync(job)
    parts = job_participants(job, plan)
    vm = int(np.argmax([len(r) for r, _ in parts]))
    assert rb.krum_f(0.2, len(parts[vm][0])) >= 1
    victim_worker = int(parts[vm][1][0])
    job.replicas[int(parts[vm][0][0])] = 1e6
    before = job.global_params.detach().cpu().numpy().copy()
    stat, bound, upd, kept = job_stat_and_bound(job, plan, 0.2, 0)
    job.aggregate(plan)
    sc.torch_sync(job)
    got = job.global_params.detach().cpu().numpy()
    picked = job.krum_selection()
    for m in range(job.n_models):
        if not upd[m]:
            assert np.array_equal(bits(got[m]), bits(before[m]))
            continue
        assert np.array_equal(picked[m], kept[m])
        if len(kept[m]) == 1:
            rows, wid = parts[m]
            row = rows[list(wid).index(int(kept[m][0]))]
            assert np.array_equal(
                bits(got[m]), bits(job.replicas[int(row)].cpu().numpy()))
        else:
            assert np.all(np.abs(got[m].astype(np.float64) - stat[m])
                          <= bound[m])
    assert victim_worker not in {int(i) for i in picked[vm]}
    return job
