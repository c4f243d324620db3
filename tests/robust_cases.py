"""Shared cases for the defended-aggregation tests (tests/test_robust_fused.py
on the CPU, tests/test_gpu_robust.py against the HIP kernels): a replica
bank whose pair rows are unsorted with holes and whose update norms are
chosen (0, 0.999 x bound, 100 x bound, ordinary), float64 references built
from norm_diff_clipping + einsum and from ServerOptimizer, and the bound
rule.

Bound rule (PARITY.md, "Defended aggregation"): a bound is 4 x err32, where
err32 is the error of the float32 SPECIFICATION (comm/robust.py on float32
tensors) against float64 on the same inputs — never the kernel's own error.
Where the float32 specification happens to land on the float64 value the
rule would give 0, so every bound has the floor of one float32 rounding of
the compared value, 2^-23 |value| + 1e-38: two correct float32
implementations may differ by that much. Every check prints its figures as
a FIG line before it asserts."""

import numpy as np
import torch

from feddrift_amd.comm import robust as rb
from feddrift_amd.comm.robust import norm_diff_clipping
from feddrift_amd.engine.server_opt import ServerOptimizer

U23 = 2.0 ** -23
FIGURES = []


def fig(case, qty, err32, kerr, bound):
    FIGURES.append((case, qty, err32, kerr, bound))
    print(f"FIG {case} | {qty} | err32={err32:.3e} | kernel={kerr:.3e} | "
          f"bound={bound:.3e}", flush=True)


def bound_from(spec32, ref64):
    """Per-element bound: max(4 x max err32 over the tensor, one float32
    rounding of the reference). Returns (bound array, max err32)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    err32 = float(np.abs(np.asarray(spec32, dtype=np.float64) - ref64).max()) \
        if ref64.size else 0.0
    return np.maximum(4.0 * err32, U23 * np.abs(ref64) + 1e-38), err32


def check(case, qty, got, spec32, ref64):
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    bound, err32 = bound_from(spec32, ref64)
    kerr = np.abs(got - ref64)
    worst = float(kerr.max()) if kerr.size else 0.0
    fig(case, qty, err32, worst, float(bound.max()) if bound.size else 0.0)
    assert np.all(kerr <= bound), (case, qty, worst)
    return err32, worst


# ----------------------------------------------------------------- clipping

class ClipCase:
    """pairs: list of (model, weight, kind); kind is 'zero' (the row equals
    its global row), 'near' (0.999 x bound), 'far' (100 x bound) or 'rand'
    (ordinary, norm about 3 x bound or bound / 3 by turns). Rows are a
    random subset of a bank with holes; the pair order is shuffled."""

    def __init__(self, P, K, pairs, bound=0.05, seed=0):
        rng = np.random.default_rng(seed)
        self.P, self.K, self.bound = P, K, bound
        pairs = list(pairs)
        order = rng.permutation(len(pairs))
        pairs = [pairs[i] for i in order]
        U = len(pairs)
        R = 2 * U + 3
        self.rows = rng.choice(R, size=U, replace=False).astype(np.int64)
        self.models = np.array([p[0] for p in pairs], dtype=np.int64)
        self.weights = np.array([p[1] for p in pairs], dtype=np.float32)
        self.kinds = [p[2] for p in pairs]
        self.glob = (rng.standard_normal((K, P)) * 0.3).astype(np.float32)
        self.bank = (rng.standard_normal((R, P)) * 0.3).astype(np.float32)
        for i, (m, _, kind) in enumerate(pairs):
            d = rng.standard_normal(P)
            d /= np.linalg.norm(d)
            r = {"zero": 0.0, "near": 0.999 * bound, "far": 100.0 * bound,
                 "rand": bound * (3.0 if i % 2 else 1.0 / 3.0)}[kind]
            self.bank[self.rows[i]] = (self.glob[m].astype(np.float64)
                                       + r * d).astype(np.float32)

    def hand_counts(self):
        """(clipped, seen) per model from the construction alone."""
        clipped = np.zeros(self.K, dtype=np.int64)
        seen = np.zeros(self.K, dtype=np.int64)
        for i, kind in enumerate(self.kinds):
            m = self.models[i]
            seen[m] += 1
            if kind == "far" or (kind == "rand" and i % 2):
                clipped[m] += 1
        return clipped, seen

    def reference(self, dtype):
        """norm_diff_clipping + einsum in `dtype`: (bank, partial [K, P+1])."""
        bank = torch.from_numpy(self.bank).to(dtype).clone()
        glob = torch.from_numpy(self.glob).to(dtype)
        rows = torch.from_numpy(self.rows)
        mo = torch.from_numpy(self.models)
        bank[rows] = norm_diff_clipping(bank[rows], glob[mo], self.bound)
        w = torch.from_numpy(self.weights).to(dtype)
        onehot = torch.zeros(len(rows), self.K, dtype=dtype)
        onehot[torch.arange(len(rows)), mo] = w
        partial = torch.zeros(self.K, self.P + 1, dtype=dtype)
        partial[:, :self.P] = torch.einsum("uk,up->kp", onehot, bank[rows])
        partial[:, self.P] = onehot.sum(0)
        return bank.numpy(), partial.numpy()

    def spec(self, dtype, with_partial=True):
        """comm.robust.clip_and_accumulate in `dtype`."""
        bank = torch.from_numpy(self.bank).to(dtype).clone()
        glob = torch.from_numpy(self.glob).to(dtype)
        partial = torch.zeros(self.K, self.P + 1, dtype=dtype) \
            if with_partial else None
        c, s = rb.clip_and_accumulate(bank, self.rows, self.models,
                                      self.weights, glob, self.bound, partial)
        return bank.numpy(), (partial.numpy() if with_partial else None), c, s

    def partial_bound(self, bank64):
        """mean_and_bound_atomic's rule on the sums themselves: one
        rounding per product and per running sum, 2 n 2^-24 sum |w x|, plus
        the rounding of the result."""
        mag = np.zeros((self.K, self.P + 1))
        n = np.zeros(self.K)
        for i, r in enumerate(self.rows):
            w = float(self.weights[i])
            if w > 0:
                m = self.models[i]
                mag[m, :self.P] += np.abs(w * bank64[r])
                mag[m, self.P] += w
                n[m] += 1
        return 2.0 * np.maximum(n, 1)[:, None] * 2.0 ** -24 * mag


def five_norm_pairs():
    """The CPU clip case: norm 0, 0.999 x bound, 100 x bound, a zero-weight
    pair (clipped all the same), ordinary pairs; model 1 has no pair."""
    return [(0, 2.5, "zero"), (0, 7.0, "near"), (0, 1.0, "far"),
            (0, 0.0, "far"), (0, 120.0, "rand"), (0, 2.5, "rand"),
            (2, 1.0, "rand"), (2, 7.0, "rand"), (2, 0.0, "rand"),
            (2, 2.5, "far")]


def check_clip(case_name, case, got_bank, got_partial, got_counts):
    """A clip result (float32 bank, partial or None, counts [K, 2]) against
    the float64 reference; the bound for rows comes from the float32
    specification, the bound for the sums from the inputs."""
    ref_bank, ref_partial = case.reference(torch.float64)
    s32_bank, s32_partial, _, _ = case.spec(torch.float32)
    untouched = np.ones(len(case.bank), dtype=bool)
    untouched[case.rows] = False
    assert np.array_equal(got_bank[untouched], case.bank[untouched]), \
        (case_name, "a row outside the plan changed")
    for i, kind in enumerate(case.kinds):
        if kind in ("zero", "near"):
            assert np.array_equal(
                got_bank[case.rows[i]].view(np.uint32),
                case.bank[case.rows[i]].view(np.uint32)), (case_name, kind)
    check(case_name, "rows", got_bank[case.rows], s32_bank[case.rows],
          ref_bank[case.rows])
    clipped, seen = case.hand_counts()
    assert np.array_equal(np.asarray(got_counts)[:, 0], clipped), case_name
    assert np.array_equal(np.asarray(got_counts)[:, 1], seen), case_name
    if got_partial is not None:
        bound = case.partial_bound(ref_bank) + U23 * np.abs(ref_partial)
        err32 = np.abs(s32_partial.astype(np.float64) - ref_partial).max()
        kerr = np.abs(got_partial.astype(np.float64) - ref_partial)
        fig(case_name, "partial", float(err32), float(kerr.max()),
            float(bound.max()))
        assert np.all(kerr <= bound), \
            (case_name, float((kerr / np.maximum(bound, 1e-300)).max()))
        # weights are small dyadic numbers: their sums are exact
        assert np.array_equal(got_partial[:, case.P],
                              ref_partial[:, case.P]), case_name


# -------------------------------------------------------------- server step

SERVER_CASES = [("avg", 1.0, 0.0), ("sgd", 1.0, 0.0), ("sgd", 0.5, 0.9),
                ("adam", 0.01, 0.0), ("adagrad", 0.01, 0.0)]


def server_inputs(K, P, steps=3, seed=0):
    """Per step: averaged [K, P] and the updated mask; row K-1 (K > 1) is
    not updated in step 2."""
    rng = np.random.default_rng(seed)
    glob = (rng.standard_normal((K, P)) * 0.3)
    avgs = [glob + rng.standard_normal((K, P)) * 0.05 for _ in range(steps)]
    upds = [np.ones(K, dtype=bool) for _ in range(steps)]
    if K > 1 and steps > 1:
        upds[1][K - 1] = False
    return glob, avgs, upds


def server_reference(kind, lr, momentum, glob, avgs, upds):
    """engine.server_opt.ServerOptimizer on float64: the bank after each
    step. 'avg' is the plain copy of the updated rows."""
    g = torch.from_numpy(np.asarray(glob, dtype=np.float64)).clone()
    out = []
    opt = None
    for avg, upd in zip(avgs, upds):
        a = torch.from_numpy(np.asarray(avg, dtype=np.float64))
        u = torch.from_numpy(upd)
        if kind == "avg":
            g = torch.where(u.unsqueeze(1), a, g)
        else:
            if opt is None:
                kw = {"momentum": momentum} if momentum else {}
                opt = ServerOptimizer(g, kind, lr, **kw)
            opt.step(g, torch.where(u.unsqueeze(1), a, g), u)
        out.append(g.numpy().copy())
    return out


def server_spec(kind, lr, momentum, glob, avgs, upds, dtype):
    g = torch.from_numpy(np.asarray(glob)).to(dtype).clone()
    state = rb.new_server_state(kind)
    out = []
    for avg, upd in zip(avgs, upds):
        rb.server_step(kind, g, torch.from_numpy(np.asarray(avg)).to(dtype),
                       torch.from_numpy(upd), state, lr, momentum)
        out.append(g.numpy().copy())
    return out


# -------------------------------------------------------------------- FLJob

def job_round(job, r, ci, replicas_from=None):
    """plan + train (+ copy another job's trained replicas in) of one
    round; returns the plan."""
    plan = job.algo.plan(job, r, ci)
    job.train(plan)
    if replicas_from is not None:
        job.replicas.copy_(replicas_from.replicas)
    return plan


def update_norms(job, plan, before):
    """L2 distance of every trained replica row from its model's row of
    `before` ([K, P] float64 numpy)."""
    reps = job.replicas.detach().cpu().double().numpy()
    K = job.n_models
    return np.array([np.linalg.norm(reps[r] - before[r % K])
                     for r in plan.rows])
