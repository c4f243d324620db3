"""Top-k upload sparsification with error-feedback memory: the specification.

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
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

KINDS = ("none", "topk")
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
