"""Upload compression with error-feedback memory: the specification of
top-k sparsification and of stochastic uniform quantisation (QSGD, Alistarh
et al. 2017; ternary at 2 bits as TernGrad, Wen et al. 2017; after top-k as
Qsparse-local-SGD, Basu et al. 2019).

Every step is float32 numpy in a fixed order, so the HIP kernels
(ops/hip/compress_kernels.hip) match it bit for bit. For the pair (replica
row r, model m) and coordinate j:

  a_j   = fl32(fl32(theta_rj - g_mj) + e_rj)     (the add skipped without
                                                   error feedback)
  key_j = bits(a_j) & 0x7fffffff                 unsigned magnitude order,
                                                   +Inf and then NaN on top
  tau   = the k-th largest key of the row
  sent  = key_j >= tau and key_j > 0             ties at tau all travel;
                                                   zeros never do
  theta_rj <- fl32(g_mj + a_j) if sent else g_mj
  e_rj     <- 0 if sent else a_j                  (0 for a non-finite a_j)

The rule has no index tie-break, so it does not depend on how a row is cut
into blocks or on the world size.

Quantisation (quant, topk_quant) to `bits` bits per coordinate, sign
included, L = 2^(bits-1) - 1 magnitude levels; w is the pair's GLOBAL worker
id and c the job's compress-pass counter:

  travel_j = key_j > 0 (quant) | sent_j of the rule above (topk_quant)
  S     = the largest key_j < INF_KEY of the row (an integer max: no order);
          s = the float32 with S's bits
  u_j   = fl32(x >> 8) * 2^-24 in [0, 1), x = word j % 4 of Philox4x32-10
          at counter (j // 4, w, m, c) under the two halves of quant_key
  for a travelling finite a_j:
    x_j = fl32(fl32(|a_j| / s) * L)               the ratio first: |a_j| * L
                                                   overflows near FLT_MAX
    q_j = min(L, floor(fl32(x_j + u_j)))           fl32(L + (1 - 2^-24)) is
                                                   L + 1: the clamp is live
    v_j = copysign(fl32(fl32(q_j / L) * s), a_j)
    theta_rj <- fl32(g_mj + v_j) if q_j > 0 else g_mj
    e_rj     <- fl32(a_j - v_j)
  a travelling non-finite a_j: theta_rj <- fl32(g_mj + a_j), e_rj <- 0
  otherwise:                   theta_rj <- g_mj, e_rj <- a_j (0 if non-finite)

The counts take the coordinates written from g + ...: q_j > 0, or travelling
and non-finite.
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

KINDS = ("none", "topk", "quant", "topk_quant")
MAG_MASK = np.uint32(0x7FFFFFFF)
INF_KEY = np.uint32(0x7F800000)


def keep_count(ratio: float, P: int) -> int:
    """min(P, max(1, ceil(ratio * P))): coordinates of a row that travel."""
    return int(min(P, max(1, math.ceil(ratio * P))))


def magnitude_key(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.uint32) & MAG_MASK


def topk_rows(theta, glob, resid, k: int):
    """The rule on [n, P] arrays: every row of `theta` against the same row
    of `glob` (and of `resid`, or None). Returns (new theta, new residual or
    None, a, sent mask); nothing is edited in place."""
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    glob = np.ascontiguousarray(glob, dtype=np.float32)
    n, P = theta.shape
    assert 1 <= k <= P, (k, P)
    with np.errstate(all="ignore"):
        a = (theta - glob).astype(np.float32)
        if resid is not None:
            a = (a + np.ascontiguousarray(resid, dtype=np.float32)) \
                .astype(np.float32)
        key = magnitude_key(a)
        tau = np.partition(key, P - k, axis=1)[:, P - k]
        sent = (key >= tau[:, None]) & (key > 0)
        new_theta = np.where(sent, (glob + a).astype(np.float32), glob)
    new_resid = None
    if resid is not None:
        keep = ~sent & (key < INF_KEY)
        new_resid = np.where(keep, a, np.float32(0.0))
    return new_theta, new_resid, a, sent


# splitmix64 tag of the quantiser's Philox key ("QUANTISE" in ASCII): the
# stream is not the aggregation noise's, which uses the bare job key
QUANT_TAG = 0x5155414E54495345


def quant_key(dummy_arg: int, curr_iter: int) -> int:
    """The 64-bit Philox key of a job's quantiser:
    mix(secure_agg.job_key ^ QUANT_TAG)."""
    from .secure_agg import _mix64, job_key
    base = np.asarray([job_key(dummy_arg, curr_iter)], dtype=np.uint64)
    return int(_mix64(base ^ np.uint64(QUANT_TAG))[0])


def levels(bits: int) -> int:
    """L = 2^(bits - 1) - 1 magnitude levels of a `bits`-bit coordinate."""
    assert 2 <= int(bits) <= 16, bits
    return (1 << (int(bits) - 1)) - 1


def quant_uniform(key: int, ctr: int, workers, models, P: int) -> np.ndarray:
    """u [n, P] float32 in [0, 1): row i is the draw of the pair (global
    worker workers[i], model models[i]) in compress pass `ctr`."""
    from .secure_agg import philox4x32
    workers = np.asarray(workers, dtype=np.uint64).reshape(-1)
    models = np.asarray(models, dtype=np.uint64).reshape(-1)
    n, nj = len(workers), (P + 3) // 4
    ctrs = np.zeros((n, nj, 4), dtype=np.uint64)
    ctrs[:, :, 0] = np.arange(nj, dtype=np.uint64)[None]
    ctrs[:, :, 1] = workers[:, None] & np.uint64(0xFFFFFFFF)
    ctrs[:, :, 2] = models[:, None]
    ctrs[:, :, 3] = np.uint64(int(ctr) & 0xFFFFFFFF)
    k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF],
                 dtype=np.uint64)
    x = philox4x32(ctrs, k).reshape(n, nj * 4)[:, :P]
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def quant_rows(theta, glob, resid, k: int, bits: int, u):
    """The quantisation rule on [n, P] arrays with the draws u [n, P];
    k = 0 is quant, k >= 1 topk_quant keeping k. Returns (new theta, new
    residual or None, a, travelling mask, q, written mask, s [n]); q is 0
    off the travelling finite coordinates."""
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    glob = np.ascontiguousarray(glob, dtype=np.float32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    n, P = theta.shape
    assert 0 <= k <= P and u.shape == (n, P), (k, P, u.shape)
    L = np.float32(levels(bits))
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        if k:
            _, _, a, travel = topk_rows(theta, glob, resid, k)
        else:
            a = (theta - glob).astype(np.float32)
            if resid is not None:
                a = (a + np.ascontiguousarray(resid, dtype=np.float32)) \
                    .astype(np.float32)
            travel = magnitude_key(a) > 0
        key = magnitude_key(a)
        finite = key < INF_KEY
        S = np.where(finite, key, np.uint32(0)).max(axis=1) if P else \
            np.zeros(n, np.uint32)
        s = np.ascontiguousarray(S, dtype=np.uint32).view(np.float32)
        sc = s[:, None]
        tf = travel & finite                     # key > 0, hence s > 0
        ratio = np.where(tf, (np.abs(a) / sc).astype(np.float32), zero)
        x = (ratio * L).astype(np.float32)
        q = np.minimum(L, np.floor((x + u).astype(np.float32)))
        q = np.where(tf, q, zero).astype(np.float32)
        v = np.copysign(((q / L).astype(np.float32) * sc).astype(np.float32),
                        a)
        raw = travel & ~finite
        written = (tf & (q > 0)) | raw
        add = np.where(raw, a, v)
        new_theta = np.where(written, (glob + add).astype(np.float32), glob)
        new_resid = None
        if resid is not None:
            new_resid = np.where(tf, (a - v).astype(np.float32),
                                 np.where(finite, a, zero))
    return new_theta, new_resid, a, travel, q, written, s


def wire_bits(kind: str, sent: int, pairs: int, P: int, bits: int) -> int:
    """Bits on the wire of `pairs` rows of P coordinates of which `sent`
    were written: a float32 per value (topk) or per row scale (the
    quantised kinds), ceil(log2 P) bits per index of a sparse row."""
    idx = max(0, int(P) - 1).bit_length()
    sent, pairs, P, bits = int(sent), int(pairs), int(P), int(bits)
    if kind == "topk":
        return sent * (32 + idx)
    if kind == "quant":
        return pairs * (32 + P * bits)
    if kind == "topk_quant":
        return pairs * 32 + sent * (bits + idx)
    raise ValueError(f"no wire format for upload_compress='{kind}'")


def quant_compress(replicas: torch.Tensor, rows, model_of, workers,
                   global_params: torch.Tensor,
                   residual: Optional[torch.Tensor], k: int, bits: int,
                   key: int, ctr: int,
                   counts: Optional[torch.Tensor] = None) -> np.ndarray:
    """topk_compress for the quantised kinds (k = 0: quant); `workers` are
    the pairs' global worker ids. Returns the per-pair written counts."""
    K, P = global_params.shape
    rows = np.asarray(rows, dtype=np.int64)
    mo = np.asarray(model_of, dtype=np.int64)
    if rows.size == 0:
        return np.zeros(0, dtype=np.int64)
    rt, mt = torch.as_tensor(rows), torch.as_tensor(mo)
    u = quant_uniform(key, ctr, workers, mo, P)
    out = quant_rows(replicas[rt].numpy(), global_params[mt].numpy(),
                     None if residual is None else residual[rt].numpy(),
                     k, bits, u)
    replicas[rt] = torch.from_numpy(out[0])
    if residual is not None:
        residual[rt] = torch.from_numpy(out[1])
    per_pair = out[5].sum(axis=1).astype(np.int64)
    if counts is not None:
        add = np.zeros((K, 2), dtype=np.int64)
        np.add.at(add[:, 0], mo, per_pair)
        np.add.at(add[:, 1], mo, P)
        counts += torch.from_numpy(add).to(counts.dtype)
    return per_pair


def topk_compress(replicas: torch.Tensor, rows, model_of,
                  global_params: torch.Tensor,
                  residual: Optional[torch.Tensor], k: int,
                  counts: Optional[torch.Tensor] = None) -> np.ndarray:
    """Compress the listed replica rows IN PLACE around their model's global
    row; `residual` (the replicas' shape, or None) is read and rewritten on
    the same rows. `counts` [K, 2] int64 gains (sent coordinates, pairs * P)
    per model. Returns the per-pair sent counts."""
    K, P = global_params.shape
    rows = np.asarray(rows, dtype=np.int64)
    mo = np.asarray(model_of, dtype=np.int64)
    if rows.size == 0:
        return np.zeros(0, dtype=np.int64)
    rt, mt = torch.as_tensor(rows), torch.as_tensor(mo)
    new_theta, new_resid, _, sent = topk_rows(
        replicas[rt].numpy(), global_params[mt].numpy(),
        None if residual is None else residual[rt].numpy(), k)
    replicas[rt] = torch.from_numpy(new_theta)
    if residual is not None:
        residual[rt] = torch.from_numpy(new_resid)
    per_pair = sent.sum(axis=1).astype(np.int64)
    if counts is not None:
        add = np.zeros((K, 2), dtype=np.int64)
        np.add.at(add[:, 0], mo, per_pair)
        np.add.at(add[:, 1], mo, P)
        counts += torch.from_numpy(add).to(counts.dtype)
    return per_pair
