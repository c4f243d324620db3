"""Secure aggregation via pairwise additive masking.

Counterpart of the reference fedml_api/distributed/turboaggregate (MPC-
style secure aggregation): each client pair (i, j) derives a shared mask
from a common seed; client i adds +mask_ij, client j adds -mask_ij, so the
server-side SUM is exact while every individual upload is information-
theoretically masked. Masks are generated on-device; the engine's fused
aggregation then operates on masked uploads unchanged.
"""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch


def pair_seed(base_seed: int, i: int, j: int) -> int:
    a, b = (i, j) if i < j else (j, i)
    return (base_seed * 1000003 + a * 7919 + b) & 0x7FFFFFFF


def mask_for(client: int, others: Sequence[int], n_params: int,
             base_seed: int, device, scale: float = 1.0) -> torch.Tensor:
    """Sum of signed pairwise masks for `client` against `others`."""
    total = torch.zeros(n_params, device=device)
    for other in others:
        if other == client:
            continue
        g = torch.Generator(device=device)
        g.manual_seed(pair_seed(base_seed, client, other))
        m = torch.randn(n_params, device=device, generator=g) * scale
        total += m if client < other else -m
    return total


def mask_uploads(uploads: torch.Tensor, clients: Sequence[int],
                 base_seed: int, scale: float = 1.0) -> torch.Tensor:
    """uploads [n, P] -> masked copies; sum over rows is preserved."""
    out = uploads.clone()
    for row, c in enumerate(clients):
        out[row] += mask_for(c, clients, uploads.shape[1], base_seed,
                             uploads.device, scale)
    return out


# ---------------------------------------------------------------------------
# secure_agg=2: exact ring arithmetic
#
# Uploads are quantised to fixed point (2^-F) and live in the ring Z_{2^M};
# pairwise masks are uniform ring elements from Philox4x32-10, so the ring
# sum of the masked contributions equals the ring sum of the plain uploads
# bit for bit, whatever the summation order. Everything below is the numpy
# SPECIFICATION; ops/hip/secagg_kernels.hip matches it bit for bit.
#
# Pair keys are derived from values every rank knows (job seed, iteration,
# aggregation counter): this reproduces the protocol's arithmetic and cost,
# not its privacy guarantee. Key agreement and dropout recovery are out of
# scope.
# ---------------------------------------------------------------------------

RING_BITS = 56
RING_MASK = (1 << RING_BITS) - 1
MAX_WORLD = 128      # int64 sum of <=128 values in [0, 2^56) cannot overflow

_PHILOX_M0 = np.uint64(0xD2511F53)
_PHILOX_M1 = np.uint64(0xCD9E8D57)
_PHILOX_W0 = 0x9E3779B9
_PHILOX_W1 = 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(ctr, key) -> np.ndarray:
    """Philox4x32-10. ctr [..., 4], key [..., 2] (uint32 values, broadcast
    against each other) -> [..., 4] uint32."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for r in range(10):
        p0 = _PHILOX_M0 * c0          # 32x32 -> 64, exact in uint64
        p1 = _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0, p1 & _U32,
                          (p0 >> _S32) ^ c3 ^ k1, p0 & _U32)
        if r < 9:
            k0 = (k0 + np.uint64(_PHILOX_W0)) & _U32
            k1 = (k1 + np.uint64(_PHILOX_W1)) & _U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3),
                    axis=-1).astype(np.uint32)


def _mix64(z: np.ndarray) -> np.ndarray:
    """splitmix64 step + finaliser on a uint64 array (wrapping)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u64(x) -> np.ndarray:
    x = np.asarray(x)
    return x if x.dtype == np.uint64 else x.astype(np.int64).astype(np.uint64)


def job_key(seed: int, curr_iter: int) -> int:
    """Per-job 64-bit key prefix: mix(mix(seed) ^ iteration)."""
    h = _mix64(_u64([seed]))
    return int(_mix64(h ^ _u64([curr_iter]))[0])


def pair_keys(base: int, agg_ctr, m, lo, hi) -> np.ndarray:
    """64-bit key of the worker pair {lo, hi} (lo < hi) for model m in
    aggregation number agg_ctr of the job whose prefix is `base`
    (job_key). All arguments broadcast; keys of two aggregations differ
    because the counter enters the mix."""
    h = _mix64(np.asarray([base], dtype=np.uint64) ^ _u64(agg_ctr))
    h = _mix64(h ^ _u64(m))
    h = _mix64(h ^ _u64(lo))
    return _mix64(h ^ _u64(hi))


def ring_mask(key: int, length: int) -> np.ndarray:
    """`length` ring elements (uint64 in [0, 2^M)) of one pair key:
    counter (j,0,0,0) yields elements 2j and 2j+1."""
    nj = (length + 1) // 2
    ctr = np.zeros((nj, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nj, dtype=np.uint64)
    k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    x = philox4x32(ctr, k).astype(np.uint64)
    out = np.empty(2 * nj, dtype=np.uint64)
    out[0::2] = (x[:, 0] | (x[:, 1] << _S32)) & np.uint64(RING_MASK)
    out[1::2] = (x[:, 2] | (x[:, 3] << _S32)) & np.uint64(RING_MASK)
    return out[:length]


def guard_limit(frac_bits: int, n_workers: int) -> float:
    """Largest admissible |n*theta| * 2^F (exclusive): with every one of
    n_workers uploads below it the true sum stays inside the signed ring."""
    return float(2.0 ** (RING_BITS - 1) / max(int(n_workers), 1))


def quantise_upload(n, theta: np.ndarray, frac_bits: int, n_workers: int):
    """Upload [n*theta_0 .. n*theta_{P-1}, n] -> (ring elements uint64
    [P+1], violated). n*theta is ONE fp32 multiply; the product is scaled
    in double and rounded to nearest even. Out-of-range / non-finite
    elements quantise to 0 and set `violated`."""
    n32 = np.float32(n)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.empty(theta.shape[0] + 1, dtype=np.float32)
        v[:-1] = np.asarray(theta, dtype=np.float32) * n32
        v[-1] = n32
        s = v.astype(np.float64) * (2.0 ** frac_bits)
        ok = np.abs(s) < guard_limit(frac_bits, n_workers)   # NaN -> False
        q = np.rint(np.where(ok, s, 0.0)).astype(np.int64)
    return q.astype(np.uint64) & np.uint64(RING_MASK), bool((~ok).any())


def dequantise(ring: np.ndarray, frac_bits: int) -> np.ndarray:
    """int64/uint64 ring sums -> float32: reduce mod 2^M, sign-extend from
    M bits, divide by 2^F in double, round to fp32."""
    r = np.asarray(ring).astype(np.uint64) & np.uint64(RING_MASK)
    s = r.astype(np.int64)
    s = np.where(s >= (1 << (RING_BITS - 1)), s - (1 << RING_BITS), s)
    return (s.astype(np.float64) / (2.0 ** frac_bits)).astype(np.float32)


class MaskGraph:
    """Who masks against whom, per model, for one (iteration, active set).

    active[m]: sorted global worker ids with a positive weight on model m.
    nbr[m]:    None for the complete graph over active[m], else a dict
               worker -> sorted array of its d neighbours.
    A model with fewer than two active workers has no edges."""

    def __init__(self, active, nbr):
        self.active = active
        self.nbr = nbr

    def neighbours(self, m: int, w: int) -> np.ndarray:
        a = self.active[m]
        if len(a) < 2:
            return a[:0]
        if self.nbr[m] is None:
            return a[a != w]
        return self.nbr[m][int(w)]


def build_mask_graph(act: np.ndarray, degree: int, seed: int,
                     curr_iter: int) -> MaskGraph:
    """act [W, K] bool. degree 0: complete graph. degree d (even): each
    worker of a model with A >= d+2 active workers masks against the
    workers at cyclic positions +-1..+-d/2 of a permutation seeded by
    (seed, iteration, m, active set) — identical on every rank; smaller
    active sets use the complete graph."""
    if degree < 0 or degree % 2:
        raise ValueError(f"secure_agg_degree must be even and >= 0, "
                         f"got {degree}")
    active, nbr = [], []
    for m in range(act.shape[1]):
        a = np.nonzero(act[:, m])[0].astype(np.int64)
        active.append(a)
        A = len(a)
        if degree == 0 or A < degree + 2:
            nbr.append(None)
            continue
        rng = np.random.default_rng(
            [int(seed) & 0xFFFFFFFF, int(curr_iter), m] + a.tolist())
        order = a[rng.permutation(A)]
        cols = [np.roll(order, -s) for s in range(1, degree // 2 + 1)] + \
               [np.roll(order, s) for s in range(1, degree // 2 + 1)]
        nb = np.sort(np.stack(cols, axis=1), axis=1)
        nbr.append({int(w): nb[i] for i, w in enumerate(order)})
    return MaskGraph(active, nbr)


def ring_contribution(replicas: np.ndarray, rows: np.ndarray,
                      workers: np.ndarray, models: np.ndarray,
                      weights: np.ndarray, n_models: int, graph: MaskGraph,
                      base: int, agg_ctr: int, frac_bits: int,
                      n_workers: int, rank: int = 0, world: int = 1,
                      skip_intra: bool = True, masked: bool = True):
    """One rank's contribution [K, P+1] (int64 in [0, 2^M)) and the range-
    guard flag. Upload i is (replica row rows[i], global worker
    workers[i], model models[i], weight weights[i]). Worker w adds the
    mask of pair {w, o} when w < o and subtracts it when w > o; with
    skip_intra, pairs whose two ends live on this rank (o % world == rank)
    are skipped — they cancel inside the contribution anyway.
    masked=False gives the plain quantised sum."""
    P = replicas.shape[1]
    L = P + 1
    out = np.zeros((n_models, L), dtype=np.uint64)
    flag = False
    pair_mask = {}               # both ends of an intra-rank pair share it
    with np.errstate(over="ignore"):
        for row, w, m, n in zip(rows, workers, models, weights):
            q, bad = quantise_upload(n, replicas[int(row)], frac_bits,
                                     n_workers)
            flag |= bad
            out[m] += q
            if not masked:
                continue
            for o in graph.neighbours(int(m), int(w)):
                o = int(o)
                if skip_intra and o % world == rank:
                    continue
                lo, hi = (w, o) if w < o else (o, w)
                r = pair_mask.get((m, lo, hi))
                if r is None:
                    r = pair_mask[(m, lo, hi)] = ring_mask(
                        int(pair_keys(base, agg_ctr, m, lo, hi)[0]), L)
                out[m] = out[m] + r if w < o else out[m] - r
    return (out & np.uint64(RING_MASK)).astype(np.int64), flag


def guard_error(frac_bits: int) -> RuntimeError:
    return RuntimeError(
        "secure aggregation range guard: an upload element is not finite "
        "or |n*theta| * 2^secure_agg_frac_bits reaches 2^55 / n_workers "
        f"(secure_agg_frac_bits={frac_bits}); lower secure_agg_frac_bits")
