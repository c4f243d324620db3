"""Shared cases for upload_compress=topk (tests/test_compress.py on the CPU,
tests/test_gpu_compress.py against the HIP kernels).

Every comparison is bit for bit against the specification
(feddrift_amd/comm/compress.py): replica bits, residual bits and counts.
The specification is float32 with a fixed operation order and the rule has
no index tie-break, so there is no tolerance to work out."""

import math

import numpy as np
import torch

from feddrift_amd.comm import compress as spec
from feddrift_amd.ops import compress_hip

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def f32(*v):
    return np.array(v, dtype=np.float32)


# ------------------------------------------------------- hand-written rows
# (name, theta, g, e or None, k, sent mask). g is zero unless the case is
# about it, so a sent coordinate holds a's own bits (0 + a = a).

def hand_cases():
    z = lambda n: np.zeros(n, np.float32)
    out = []
    # ties at tau with opposite signs: all travel, more than k
    out.append(("ties", f32(3, -3, 1, 3, 0.5), z(5), None, 2,
                [1, 1, 0, 1, 0]))
    out.append(("ties with residual", f32(2, -3, 1, 3, 0.5), z(5),
                f32(1, 0, 0, 0, 0), 2, [1, 1, 0, 1, 0]))
    # fewer non-zeros than k: tau = 0 and zeros (of either sign) stay
    out.append(("fewer non-zeros than k", f32(0, 2, 0, -0.0, 0), z(5),
                z(5), 3, [0, 1, 0, 0, 0]))
    out.append(("all-zero update", f32(1, -2, 3), f32(1, -2, 3), z(3), 2,
                [0, 0, 0]))
    # update and residual cancel: a = 0, nothing travels
    out.append(("residual cancels", f32(1.5, 0, 4), f32(1, 0, 4),
                f32(-0.5, 0, 0), 1, [0, 0, 0]))
    # non-finite values travel first: NaN above +-Inf above every finite
    out.append(("non-finite first k=3", f32(1, NAN, 5, INF, -INF, 2), z(6),
                z(6), 3, [0, 1, 0, 1, 1, 0]))
    out.append(("non-finite first k=1", f32(1, NAN, 5, INF, -INF, 2), z(6),
                z(6), 1, [0, 1, 0, 0, 0, 0]))
    # k = 2 with one NaN: tau is the Inf key and both Infs tie
    out.append(("non-finite first k=2", f32(1, NAN, 5, INF, -INF, 2), z(6),
                None, 2, [0, 1, 0, 1, 1, 0]))
    # more non-finite than k, two NaNs tie at tau, the Infs are held back
    # and must not enter the residual
    out.append(("more non-finite than k", f32(NAN, INF, 7, NAN, -INF, 0.25),
                z(6), f32(0, 0, 1, 0, 0, 0), 1, [1, 0, 0, 1, 0, 0]))
    return out


def check_hand_case(name, theta, g, e, k, sent):
    """The specification on one hand-written row, and the invariant."""
    sent = np.asarray(sent, dtype=bool)
    nt, nr, a, got = spec.topk_rows(theta[None], g[None],
                                    None if e is None else e[None], k)
    assert np.array_equal(got[0], sent), name
    check_invariant(name, a[0], g, nt[0], None if nr is None else nr[0],
                    sent)
    return int(sent.sum())


def check_invariant(name, a, g, new_theta, new_resid, sent):
    """Per coordinate: the replica holds fl32(g + a) where sent and g's bits
    elsewhere; with a residual exactly one of (sent value, residual) carries
    a's bits and the other is +0, except that an unsent non-finite a is
    dropped (both 0)."""
    with np.errstate(all="ignore"):
        want_t = np.where(sent, (g + a).astype(np.float32), g)
    assert np.array_equal(bits(new_theta), bits(want_t)), name
    if new_resid is None:
        return
    travels = np.where(sent, a, np.float32(0))
    ab, tb, rb = bits(a), bits(travels), bits(new_resid)
    finite = np.isfinite(a)
    one = ((tb == ab) & (rb == 0)) | ((tb == 0) & (rb == ab))
    dropped = ~finite & ~sent & (tb == 0) & (rb == 0)
    assert np.all(one | dropped), name
    assert np.all(np.isfinite(new_resid)), name


# ------------------------------------------------------------- op-level run

def normal(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale) \
        .astype(np.float32)


def expected(bank, glob, rows, models, resid, k):
    """The specification applied by hand: (bank, residual, [K, 2] counts)."""
    rows = np.asarray(rows, dtype=np.int64)
    models = np.asarray(models, dtype=np.int64)
    K, P = glob.shape
    bank = bank.copy()
    resid = None if resid is None else resid.copy()
    counts = np.zeros((K, 2), dtype=np.int64)
    if len(rows):
        nt, nr, _, sent = spec.topk_rows(
            bank[rows], glob[models],
            None if resid is None else resid[rows], k)
        bank[rows] = nt
        if resid is not None:
            resid[rows] = nr
        np.add.at(counts[:, 0], models, sent.sum(axis=1))
        np.add.at(counts[:, 1], models, P)
    return bank, resid, counts


def run_op(dev, bank, glob, rows, models, resid, k, plan=None, counts=None,
           **over):
    """One compress_hip.topk call on `dev`; numpy in, numpy out."""
    K = glob.shape[0]
    b = torch.from_numpy(bank.copy()).to(dev)
    g = torch.from_numpy(glob.copy()).to(dev)
    e = None if resid is None else torch.from_numpy(resid.copy()).to(dev)
    if plan is None:
        plan = compress_hip.CompressPlan(rows, models, K)
    c = compress_hip.new_counts(K, dev) if counts is None else counts
    compress_hip.topk(b, plan, g, e, k, c, **over)
    return (b.cpu().numpy(), None if e is None else e.cpu().numpy(),
            c.cpu().numpy())


def check(dev, name, bank, glob, rows, models, resid, k, **over):
    """Run the op and hold it to the specification, unlisted rows included."""
    want = expected(bank, glob, rows, models, resid, k)
    got = run_op(dev, bank, glob, rows, models, resid, k, **over)
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{name}: replicas"
    if resid is not None:
        assert np.array_equal(bits(got[1]), bits(want[1])), \
            f"{name}: residual"
    assert np.array_equal(got[2], want[2]), f"{name}: counts {got[2]}"
    return got


def k_list(P):
    return sorted({1, math.ceil(P / 10), max(1, P - 1), P})


def case_shape(dev, P, n_pairs=3, seed=0, ef=True, ks=None, **over):
    """n_pairs pairs of one model at row length P, every k of k_list."""
    bank = normal((n_pairs + 2, P), seed)
    glob = normal((1, P), seed + 1, 0.5)
    resid = normal((n_pairs + 2, P), seed + 2, 0.05) if ef else None
    rows = np.arange(n_pairs) + 1
    out = []
    for k in ks or k_list(P):
        out.append(check(dev, f"P={P} k={k}", bank, glob, rows,
                         np.zeros(n_pairs, int), resid, k, **over))
    return out


def case_integer_ties(dev, P, **over):
    """Integers-in-float with many equal magnitudes of either sign: the tie
    rule at every k."""
    rng = np.random.default_rng(P)
    bank = rng.integers(-4, 5, size=(3, P)).astype(np.float32)
    glob = np.zeros((1, P), np.float32)
    resid = rng.integers(-1, 2, size=(3, P)).astype(np.float32)
    for k in k_list(P):
        check(dev, f"integer ties P={P} k={k}", bank, glob, np.arange(3),
              np.zeros(3, int), resid, k, **over)


def case_odd_offsets(dev, **over):
    """An odd P puts every other row at an odd dword offset."""
    P = 77
    bank = normal((9, P), 3)
    glob = normal((2, P), 4, 0.5)
    resid = normal((9, P), 5, 0.05)
    rows = np.array([1, 3, 5, 7])
    check(dev, "odd offsets", bank, glob, rows, rows // 2 % 2, resid, 8,
          **over)


def case_shuffled_rows(dev, **over):
    P = 130
    bank = normal((23, P), 6)
    glob = normal((3, P), 7, 0.5)
    resid = normal((23, P), 8, 0.05)
    rng = np.random.default_rng(9)
    rows = rng.choice(23, size=11, replace=False)
    check(dev, "shuffled rows", bank, glob, rows, rng.integers(0, 3, 11),
          resid, 13, **over)


def case_three_models(dev, **over):
    """Pair counts 5, 0 and 2 in one launch."""
    P = 70
    bank = normal((8, P), 10)
    glob = normal((3, P), 11, 0.5)
    resid = normal((8, P), 12, 0.05)
    models = np.array([0, 2, 0, 0, 2, 0, 0])
    got = check(dev, "three models", bank, glob, np.arange(7), models, resid,
                7, **over)
    assert got[2][1].tolist() == [0, 0]


def case_hand_rows(dev, pad=0, **over):
    """The tie, zero and non-finite rows through the op; `pad` zero
    coordinates behind them move the row to another kernel and change
    neither tau nor the sent set."""
    for name, theta, g, e, k, sent in hand_cases():
        z = np.zeros(pad, np.float32)
        theta, g = np.concatenate([theta, z]), np.concatenate([g, z])
        e = None if e is None else np.concatenate([e, z])
        sent = np.concatenate([np.asarray(sent, bool), np.zeros(pad, bool)])
        bank = np.stack([theta, theta])
        resid = None if e is None else np.stack([e, e])
        got = check(dev, f"{name} pad={pad}", bank, g[None], [0, 1], [0, 0],
                    resid, k, **over)
        assert got[2][0, 0] == 2 * int(sent.sum()), name
        with np.errstate(all="ignore"):
            a = (theta - g).astype(np.float32)
            if e is not None:
                a = (a + e).astype(np.float32)
        check_invariant(name, a, g, got[0][0],
                        None if e is None else got[1][0], sent)


def digit_inputs(P=200):
    """Three rows for the 11 + 10 + 10 radix split: the k-th key differs
    from its neighbours only in the top, the middle and the low digit."""
    out = []
    base = np.uint32(0x3F800000)               # 1.0
    for name, step in (("top", 1 << 20), ("middle", 1 << 10), ("low", 1)):
        keys = base + np.uint32(step) * np.arange(P, dtype=np.uint32)
        vals = keys.view(np.float32).copy()
        assert np.all(np.isfinite(vals))
        vals[::3] *= -1                        # the sign is no part of a key
        np.random.default_rng(step).shuffle(vals)
        out.append((name, vals))
    return out


def case_digits(dev, **over):
    for name, vals in digit_inputs():
        P = len(vals)
        bank = np.stack([vals, vals[::-1].copy()])
        glob = np.zeros((1, P), np.float32)
        for k in (1, 2, P // 2, P - 1):
            got = check(dev, f"digit {name} k={k}", bank, glob, [0, 1],
                        [0, 0], None, k, **over)
            assert got[2][0, 0] == 2 * k       # distinct keys: exactly k


def case_two_calls(dev, P, **over):
    """The residual of call 1 feeds call 2, and a repeat of the same inputs
    is bit-equal."""
    K, n = 2, 5
    glob = normal((K, P), 20, 0.5)
    rows, models = np.arange(n), np.arange(n) % K
    k = max(1, P // 10)
    bank1, bank2 = normal((n, P), 21), normal((n, P), 22)
    resid0 = np.zeros((n, P), np.float32)
    b1, e1, c1 = check(dev, "call 1", bank1, glob, rows, models, resid0, k,
                       **over)
    assert np.any(e1 != 0)
    b2, e2, c2 = check(dev, "call 2", bank2, glob, rows, models, e1, k,
                       **over)
    # call 2 without call 1's residual sends something else
    b2z, _, _ = run_op(dev, bank2, glob, rows, models, resid0, k, **over)
    assert not np.array_equal(bits(b2), bits(b2z))
    again = run_op(dev, bank2, glob, rows, models, e1, k, **over)
    assert np.array_equal(bits(again[0]), bits(b2))
    assert np.array_equal(bits(again[1]), bits(e2))
    assert np.array_equal(again[2], c2)


# -------------------------------------------------------------------- FLJob

def fljob_against_hand_loop(tmp_path, device, n_rounds, ef, make=None,
                            n_clients=10, ratio=0.1, **cfg_kw):
    """A topk job against a plain job of the same seeds whose trained rows
    are compressed by hand with the specification; replicas, residual, the
    counts and the aggregated global rows agree bit for bit every round.

    Under robust_fused=1 with the mean the compressed job's weighted sums
    come from the clip pass run with an infinite bound; the by-hand loop
    calls that pass on the rows it compressed."""
    import secagg_cases as sc
    from feddrift_amd.ops import robust_hip
    make = make or sc.make_job
    kw = dict(cfg_kw)
    if device is not None:
        kw["device"] = device
    A = make(tmp_path / "a", n_clients=n_clients, upload_compress="topk",
             compress_ratio=ratio, compress_error_feedback=ef, **kw)
    B = make(tmp_path / "b", n_clients=n_clients, **kw)
    assert B._residual is None and not B._compress
    assert (A._residual is not None) == bool(ef)
    K, P = A.n_models, A.n_params
    k = spec.keep_count(ratio, P)
    assert A._compress_k == k
    fused_mean = cfg_kw.get("robust_fused", 0) == 1 and \
        cfg_kw.get("robust_agg", "mean") == "mean" and \
        cfg_kw.get("secure_agg", 0) != 2
    resid = np.zeros((A.replicas.shape[0], P), np.float32) if ef else None
    ci = A.client_sampling(0)
    carried = False
    for r in range(n_rounds):
        assert np.array_equal(bits(A.global_params), bits(B.global_params))
        pa = A.algo.plan(A, r, ci)
        A.train(pa)
        pb = B.algo.plan(B, r, ci)
        B.train(pb)
        sc.torch_sync(A)
        assert np.array_equal(pa.rows, pb.rows)
        assert np.array_equal(pa.step_off, pb.step_off)
        glob = B.global_params.cpu().numpy()
        if ef and r > 0:
            carried = carried or bool(np.any(resid[pb.rows] != 0))
        reps, resid, counts = expected(
            B.replicas.cpu().numpy(), glob, pb.rows, pb.rows % K, resid, k)
        assert np.array_equal(bits(A.replicas), bits(reps)), f"round {r}"
        if ef:
            assert np.array_equal(bits(A._residual), bits(resid)), \
                f"round {r}"
        assert np.array_equal(A.compress_stats(), counts), f"round {r}"
        B.replicas.copy_(torch.from_numpy(reps))
        B._partial_fused = False
        if fused_mean:
            mo = pb.rows % K
            cp = robust_hip.ClipPlan(pb.rows, mo,
                                     pb.sample_num[pb.rows // K, mo], K)
            B._partial.zero_()
            robust_hip.clip_accumulate(
                B.replicas, cp, B.global_params, float("inf"), B._partial,
                robust_hip.new_counts(K, B.device))
            B._partial_fused = True
            # the infinite bound left every compressed bit
            assert np.array_equal(bits(B.replicas), bits(reps))
            assert np.array_equal(bits(A.replicas), bits(reps))
        A.algo.aggregate(A, r, pa, ci)
        B.algo.aggregate(B, r, pb, ci)
        sc.torch_sync(A)
        assert np.array_equal(bits(A.global_params),
                              bits(B.global_params)), f"round {r}"
    if ef and n_rounds > 1:
        assert carried, "no residual reached a later round"
    assert np.all(A.clip_stats() == 0) or \
        cfg_kw.get("robust_norm_bound", 0) > 0
    return A, B
