"""Shared cases for upload_compress=quant and topk_quant (tests/test_quant.py
on the CPU, tests/test_gpu_quant.py against the HIP kernels).

Every comparison is bit for bit against the specification
(feddrift_amd/comm/compress.py:quant_rows): replica bits, residual bits and
counts. The specification is float32 with a fixed operation order, the scale
is an integer maximum and the draws are a pure function of (key, pass
counter, global worker id, model, coordinate), so there is no tolerance to
work out."""

import numpy as np
import torch

import compress_cases as cc
from feddrift_amd.comm import compress as spec
from feddrift_amd.ops import compress_hip

bits, f32, normal = cc.bits, cc.f32, cc.normal
NAN, INF = cc.NAN, cc.INF
KEY = spec.quant_key(7, 3)
U_TOP = np.float32(1.0) - np.float32(2.0 ** -24)   # the largest draw

# A draw of the stream KEY with every one of its 24 bits set, found by a
# search over pass counters on the CPU: worker 0, model 0, coordinate
# CLAMP_J, pass CLAMP_CTR (above 2^16). clamp_draw() checks it is still one.
CLAMP_CTR, CLAMP_J = 2511787, 1


def clamp_draw():
    u = spec.quant_uniform(KEY, CLAMP_CTR, [0], [0], CLAMP_J + 1)[0, CLAMP_J]
    assert u == U_TOP, "CLAMP_CTR no longer names a top draw: search again"
    return u


def kind_k(kind, P, ratio=0.1):
    return 0 if kind == "quant" else spec.keep_count(ratio, P)


def spec_rows(theta, glob, resid, k, nbits, workers, models, ctr, key=KEY):
    """quant_rows with the draws of (key, ctr, workers, models)."""
    theta = np.atleast_2d(np.asarray(theta, np.float32))
    u = spec.quant_uniform(key, ctr, workers, models, theta.shape[1])
    return spec.quant_rows(theta, np.atleast_2d(glob),
                           None if resid is None else np.atleast_2d(resid),
                           k, nbits, u) + (u,)


# ------------------------------------------------------- hand-written rows
# (name, theta, g, e or None, bits, ctr); g is zero, so a written coordinate
# holds v's own bits. Every row is quantised as a whole (k = 0) and with
# k = 2.

SUB = np.float32(2.0 ** -140)                   # subnormal


def hand_cases():
    z = lambda n: np.zeros(n, np.float32)
    out = []
    out.append(("ternary", f32(1, -1, 0.5, 0, -0.25), z(5), z(5), 2, 0))
    out.append(("non-finite", f32(2, INF, -0.5, NAN, 1, -INF), z(6), z(6),
                4, 1))
    out.append(("all-zero", f32(1, -2, 3, 0), f32(1, -2, 3, 0), z(4), 8, 2))
    out.append(("subnormal scale", np.array([3, -1, 2, 0, -3], np.float32)
                * SUB, z(5), z(5), 4, 3))
    out.append(("near FLT_MAX", f32(3e38, 1e38, -2e38, 1e37), z(4), None,
                8, 4))
    # the clamp: coordinate CLAMP_J is the row maximum and draws U_TOP
    row = f32(0.5, 0.25, -0.125, 0.3)
    row[CLAMP_J] = -1.0
    out.append(("clamp", row, z(4), z(4), 8, CLAMP_CTR))
    return out


def check_hand_case(name, theta, g, e, nbits, ctr, got=None, k=0):
    """The properties the row was written for, on the specification's
    result or on `got` = (new theta, new residual) of a kernel."""
    L = spec.levels(nbits)
    nt, nr, a, travel, q, written, s, u = spec_rows(
        theta, g, e, k, nbits, [0], [0], ctr)
    if got is not None:
        assert np.array_equal(bits(got[0]), bits(nt[0])), name
        if e is not None:
            assert np.array_equal(bits(got[1]), bits(nr[0])), name
        nt = got[0][None]
        nr = None if e is None else got[1][None]
    nt, a, q, travel = nt[0], a[0], q[0], travel[0]
    nr = None if nr is None else nr[0]
    if name == "ternary":
        assert L == 1 and s[0] == 1.0
        assert nt[0] == 1.0 and nt[1] == -1.0       # always exactly +-1
        assert not travel[3] and nt[3] == 0.0
        if k == 0:
            assert set(q[[2, 4]]) <= {0.0, 1.0}
            assert set(np.abs(nt[[2, 4]])) <= {0.0, 1.0}
    elif name == "non-finite":
        assert s[0] == 2.0                          # from the finite entries
        assert np.isposinf(nt[1]) and np.isnan(nt[3]) and np.isneginf(nt[5])
        assert np.all(nr[[1, 3, 5]] == 0) and np.all(np.isfinite(nr))
        if k == 0:
            assert nt[0] == 2.0
    elif name == "all-zero":
        assert s[0] == 0.0 and not travel.any()
        assert np.array_equal(bits(nt), bits(g))
        assert np.all(bits(nr) == 0)
    elif name == "subnormal scale":
        assert 0 < s[0] < np.finfo(np.float32).tiny
        assert bits(nt[0]) == bits(theta[0]) and bits(nt[4]) == bits(theta[4])
        if k == 0:
            assert q[1] in (2.0, 3.0) and q[2] in (4.0, 5.0)
    elif name == "near FLT_MAX":
        assert s[0] == np.float32(3e38) and nt[0] == np.float32(3e38)
        assert np.all(np.isfinite(nt))
        # 1e38 against s = 3e38: about L / 3, not L
        assert abs(q[2] - 2 * L / 3) < 1
        if k == 0:
            assert abs(q[1] - L / 3) < 1
            assert abs(float(nt[1]) - 1e38) <= 3e38 / L
    elif name == "clamp":
        j = CLAMP_J
        assert u[0, j] == clamp_draw()
        x = np.float32(np.float32(abs(a[j]) / s[0]) * np.float32(L))
        assert x == L
        assert np.floor(np.float32(x + u[0, j])) == L + 1   # reachable
        assert q[j] == L and bits(nt[j]) == bits(a[j])
        assert nr[j] == 0.0
    else:
        raise AssertionError(name)


def check_invariants(name, theta, g, e, k, nbits, out):
    """Per coordinate of quant_rows' result `out` (with u appended)."""
    nt, nr, a, travel, q, written, s, u = out
    L = np.float32(spec.levels(nbits))
    key = spec.magnitude_key(a)
    finite = key < spec.INF_KEY
    tf = travel & finite
    assert np.all((q >= 0) & (q <= L)) and np.all(q == np.floor(q)), name
    assert np.all(q[~tf] == 0), name
    with np.errstate(all="ignore"):
        x = ((np.abs(a) / s[:, None]).astype(np.float32) * L) \
            .astype(np.float32)
        assert np.all((np.abs(q - x) < 1)[tf] | (q == L)[tf]), name
        v = np.copysign(((q / L).astype(np.float32) * s[:, None])
                        .astype(np.float32), a)
        assert np.array_equal(bits(nt[q == 0]),
                              bits(np.broadcast_to(g, nt.shape)[q == 0])), name
        assert np.array_equal(bits(nt[tf & (q > 0)]),
                              bits((g + v).astype(np.float32)[tf & (q > 0)]))
        if nr is not None:
            assert np.array_equal(bits(nr[tf]),
                                  bits((a - v).astype(np.float32)[tf])), name
    assert np.array_equal(written, tf & (q > 0)), name   # the rows are finite
    if k:
        tk = spec.topk_rows(theta, g, e, k)
        assert np.array_equal(travel, tk[3]), name
        assert np.array_equal(bits(nt[~travel]), bits(tk[0][~travel])), name
        if nr is not None:
            assert np.array_equal(bits(nr[~travel]),
                                  bits(tk[1][~travel])), name
    else:
        assert np.array_equal(travel, key > 0), name


# ------------------------------------------------------------- op-level run

def expected(bank, glob, rows, models, workers, resid, k, nbits, ctr,
             key=KEY):
    """The specification applied by hand: (bank, residual, [K, 2] counts)."""
    rows = np.asarray(rows, dtype=np.int64)
    models = np.asarray(models, dtype=np.int64)
    K, P = glob.shape
    bank = bank.copy()
    resid = None if resid is None else resid.copy()
    counts = np.zeros((K, 2), dtype=np.int64)
    if len(rows):
        out = spec_rows(bank[rows], glob[models],
                        None if resid is None else resid[rows], k, nbits,
                        workers, models, ctr, key)
        bank[rows] = out[0]
        if resid is not None:
            resid[rows] = out[1]
        np.add.at(counts[:, 0], models, out[5].sum(axis=1))
        np.add.at(counts[:, 1], models, P)
    return bank, resid, counts


def run_op(dev, bank, glob, rows, models, workers, resid, k, nbits, ctr,
           key=KEY, plan=None, counts=None, **over):
    """One compress_hip.quant call on `dev`; numpy in, numpy out."""
    K = glob.shape[0]
    b = torch.from_numpy(bank.copy()).to(dev)
    g = torch.from_numpy(glob.copy()).to(dev)
    e = None if resid is None else torch.from_numpy(resid.copy()).to(dev)
    if plan is None:
        plan = compress_hip.CompressPlan(rows, models, K, workers)
    c = compress_hip.new_counts(K, dev) if counts is None else counts
    compress_hip.quant(b, plan, g, e, k, nbits, key, ctr, c, **over)
    return (b.cpu().numpy(), None if e is None else e.cpu().numpy(),
            c.cpu().numpy())


def check(dev, name, bank, glob, rows, models, workers, resid, k, nbits, ctr,
          **over):
    """Run the op and hold it to the specification, unlisted rows included."""
    want = expected(bank, glob, rows, models, workers, resid, k, nbits, ctr)
    got = run_op(dev, bank, glob, rows, models, workers, resid, k, nbits,
                 ctr, **over)
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{name}: replicas"
    if resid is not None:
        assert np.array_equal(bits(got[1]), bits(want[1])), \
            f"{name}: residual"
    assert np.array_equal(got[2], want[2]), f"{name}: counts {got[2]}"
    return got


def case_shape(dev, P, kind, nbits, n_pairs=3, seed=0, ef=True, ctr=5,
               **over):
    """n_pairs pairs on 2 models at row length P: shuffled rows of a larger
    bank (odd offsets at an odd P), worker ids that are not the pair index."""
    rng = np.random.default_rng(seed + 100)
    n_rows = n_pairs + 4
    bank = normal((n_rows, P), seed)
    glob = normal((2, P), seed + 1, 0.5)
    resid = normal((n_rows, P), seed + 2, 0.05) if ef else None
    rows = rng.choice(n_rows, size=n_pairs, replace=False)
    models = np.arange(n_pairs) % 2
    workers = 7 + 3 * np.arange(n_pairs)
    return check(dev, f"{kind} P={P} b={nbits}", bank, glob, rows, models,
                 workers, resid, kind_k(kind, P), nbits, ctr, **over)


def case_hand_rows(dev, pad=0, **over):
    """The hand rows through the op, as quant and with k = 2; `pad` zero
    coordinates behind them move the row to another kernel and change
    neither the scale, tau nor the draws of the first coordinates."""
    for name, theta, g, e, nbits, ctr in hand_cases():
        z = np.zeros(pad, np.float32)
        theta, g = np.concatenate([theta, z]), np.concatenate([g, z])
        e = None if e is None else np.concatenate([e, z])
        for k in (0, 2):
            got = check(dev, f"{name} pad={pad} k={k}", theta[None], g[None],
                        [0], [0], [0], None if e is None else e[None], k,
                        nbits, ctr, **over)
            check_hand_case(name, theta, g, e, nbits, ctr, k=k,
                            got=(got[0][0],
                                 None if e is None else got[1][0]))


def case_two_calls(dev, P, kind, nbits=4, **over):
    """Two passes on the same bank: the residual of pass c feeds pass c + 1,
    whose draws differ; then a pass at a counter above 2^16."""
    K, n = 2, 5
    glob = normal((K, P), 20, 0.5)
    rows, models, workers = np.arange(n), np.arange(n) % K, np.arange(n) + 2
    k = kind_k(kind, P)
    bank1, bank2 = normal((n, P), 21), normal((n, P), 22)
    resid0 = np.zeros((n, P), np.float32)
    _, e1, _ = check(dev, "pass 0", bank1, glob, rows, models, workers,
                     resid0, k, nbits, 0, **over)
    assert np.any(e1 != 0)
    b2, _, _ = check(dev, "pass 1", bank2, glob, rows, models, workers, e1,
                     k, nbits, 1, **over)
    # the same inputs at pass 0's counter, or without its residual, send
    # something else
    same, _, _ = run_op(dev, bank2, glob, rows, models, workers, e1, k,
                        nbits, 0, **over)
    assert not np.array_equal(bits(b2), bits(same))
    b2z, _, _ = run_op(dev, bank2, glob, rows, models, workers, resid0, k,
                       nbits, 1, **over)
    assert not np.array_equal(bits(b2), bits(b2z))
    big = (1 << 16) + 12345
    hi, _, _ = check(dev, "pass above 2^16", bank2, glob, rows, models,
                     workers, e1, k, nbits, big, **over)
    low, _, _ = run_op(dev, bank2, glob, rows, models, workers, e1, k, nbits,
                       big & 0xFFFF, **over)
    assert not np.array_equal(bits(hi), bits(low))


# -------------------------------------------------------------------- FLJob

def fljob_against_hand_loop(tmp_path, device, n_rounds, kind, ef, nbits=4,
                            make=None, n_clients=10, ratio=0.1, **cfg_kw):
    """A quantising job against a plain job of the same seeds whose trained
    rows are compressed by hand with the specification; replicas, residual,
    the counts and the aggregated global rows agree bit for bit every
    round (compress_cases.fljob_against_hand_loop for these kinds)."""
    import secagg_cases as sc
    from feddrift_amd.ops import robust_hip
    make = make or sc.make_job
    kw = dict(cfg_kw)
    if device is not None:
        kw["device"] = device
    A = make(tmp_path / "a", n_clients=n_clients, upload_compress=kind,
             compress_ratio=ratio, compress_error_feedback=ef,
             compress_bits=nbits, **kw)
    B = make(tmp_path / "b", n_clients=n_clients, **kw)
    assert B._residual is None and not B._compress
    assert (A._residual is not None) == bool(ef)
    K, P = A.n_models, A.n_params
    k = kind_k(kind, P, ratio)
    assert A._compress_k == k
    key = spec.quant_key(A.cfg.dummy_arg, A.curr_iter)
    assert A._quant_key == key
    fused_mean = cfg_kw.get("robust_fused", 0) == 1 and \
        cfg_kw.get("robust_agg", "mean") == "mean" and \
        cfg_kw.get("secure_agg", 0) != 2
    resid = np.zeros((A.replicas.shape[0], P), np.float32) if ef else None
    own = np.asarray(A.owned_workers, dtype=np.int64)
    ci = A.client_sampling(0)
    carried = False
    for r in range(n_rounds):
        assert np.array_equal(bits(A.global_params), bits(B.global_params))
        assert A._compress_ctr == r
        pa = A.algo.plan(A, r, ci)
        A.train(pa)
        pb = B.algo.plan(B, r, ci)
        B.train(pb)
        sc.torch_sync(A)
        assert np.array_equal(pa.rows, pb.rows)
        glob = B.global_params.cpu().numpy()
        if ef and r > 0:
            carried = carried or bool(np.any(resid[pb.rows] != 0))
        reps, resid, counts = expected(
            B.replicas.cpu().numpy(), glob, pb.rows, pb.rows % K,
            own[pb.rows // K], resid, k, nbits, r, key)
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
            assert np.array_equal(bits(A.replicas), bits(reps))
        A.algo.aggregate(A, r, pa, ci)
        B.algo.aggregate(B, r, pb, ci)
        sc.torch_sync(A)
        assert np.array_equal(bits(A.global_params),
                              bits(B.global_params)), f"round {r}"
    if ef and n_rounds > 1:
        assert carried, "no residual reached a later round"
    return A, B, counts
