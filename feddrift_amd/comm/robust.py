"""Robust aggregation defenses: update-norm clipping + Gaussian noise.

Counterpart of the reference fedml_core/distributed/robustness/
robust_aggregation.py (RobustAggregator.norm_diff_clipping :38,
add_noise :51) and the fedavg_robust package, re-expressed on flat
parameter vectors so it composes with the engine's fused aggregation:
each client update is clipped to `norm_bound` around the previous global
model BEFORE the weighted average, and stddev-sigma noise is added AFTER.
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch


def norm_diff_clipping(local_flat: torch.Tensor, global_flat: torch.Tensor,
                       norm_bound: float) -> torch.Tensor:
    """Clip (local - global) to an L2 ball of radius norm_bound."""
    diff = local_flat - global_flat
    norm = torch.linalg.vector_norm(diff, dim=-1, keepdim=True)
    scale = torch.clamp(norm_bound / (norm + 1e-12), max=1.0)
    return global_flat + diff * scale


def add_noise(flat: torch.Tensor, stddev: float,
              generator: Optional[torch.Generator] = None) -> torch.Tensor:
    noise = torch.randn(flat.shape, device=flat.device, generator=generator)
    return flat + stddev * noise


def robustify_replicas(replicas: torch.Tensor, global_params: torch.Tensor,
                       rows: torch.Tensor, model_of: torch.Tensor,
                       norm_bound: float) -> None:
    """In-place clipping of trained replica rows around their global model
    row (engine hook: called between local training and aggregation)."""
    if rows.numel() == 0:
        return
    local = replicas[rows]
    glob = global_params[model_of.long()]
    replicas[rows] = norm_diff_clipping(local, glob, norm_bound)


# ---------------------------------------------------------------------------
# robust_fused=1: the SPECIFICATION of the fused clip / noise / server-step
# path. These functions define the arithmetic (and run as the CPU path);
# ops/hip/robust_kernels.hip follows them in fp32.
# ---------------------------------------------------------------------------

SERVER_KINDS = ("avg", "sgd", "adam", "adagrad")
# torch's defaults, which engine/server_opt.py constructs
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8
ADAGRAD_EPS = 1e-10


def clip_scale(norm, bound: float):
    """min(1, bound / (norm + 1e-12)) — norm_diff_clipping's factor."""
    if isinstance(norm, torch.Tensor):
        return torch.clamp(bound / (norm + 1e-12), max=1.0)
    return np.minimum(1.0, bound / (np.asarray(norm) + 1e-12))


def clip_and_accumulate(replicas: torch.Tensor, rows, model_of, weights,
                        global_params: torch.Tensor, bound: float,
                        partial: Optional[torch.Tensor] = None):
    """Clip the listed replica rows IN PLACE to an L2 ball of radius `bound`
    around their model's global row, and (with `partial` [K, P+1]) add
    w * clipped into partial[model, :P] and w into partial[model, P] for
    every pair with w > 0. A row whose factor is 1 keeps its bits; a row
    with w == 0 is still clipped but adds nothing. Returns the per-model
    counts (clipped, seen) as int64 arrays [K]."""
    K, P = global_params.shape
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    mo = torch.as_tensor(np.asarray(model_of, dtype=np.int64))
    w = torch.as_tensor(np.asarray(weights)).to(replicas.dtype)
    clipped_n = np.zeros(K, dtype=np.int64)
    seen_n = np.zeros(K, dtype=np.int64)
    if rows.numel() == 0:
        return clipped_n, seen_n
    local = replicas[rows]
    glob = global_params[mo]
    diff = local - glob
    norm = torch.linalg.vector_norm(diff, dim=1)
    scale = clip_scale(norm, bound)
    hit = scale < 1.0
    out = torch.where(hit.unsqueeze(1), glob + diff * scale.unsqueeze(1),
                      local)
    replicas[rows[hit]] = out[hit]
    if partial is not None:
        sel = w > 0
        ws = w[sel].unsqueeze(1)
        partial.index_add_(0, mo[sel], torch.cat([ws * out[sel], ws], dim=1))
    np.add.at(seen_n, mo.numpy(), 1)
    np.add.at(clipped_n, mo.numpy()[hit.numpy()], 1)
    return clipped_n, seen_n


def noise_key(dummy_arg: int, curr_iter: int) -> int:
    """The 64-bit Philox key of a job's noise: secure_agg.job_key."""
    from .secure_agg import job_key
    return job_key(dummy_arg, curr_iter)


def gaussian_noise(key: int, ctr: int, K: int, P: int, dtype=np.float64,
                   models=None, p0: int = 0, p1: Optional[int] = None
                   ) -> np.ndarray:
    """Standard normals [K, P] (or the block models x [p0, p1) of them): a
    pure function of (key, ctr, m, p). Philox4x32-10 with counter
    (p // 4, m, ctr & 0xffffffff, ctr >> 32) and the two halves of `key`;
    outputs (x0, x1) give p = 4j, 4j+1 and (x2, x3) give 4j+2, 4j+3 by
    Box-Muller on u = (x + 0.5) * 2^-32: r = sqrt(-2 ln u_a),
    z_even = r cos(2 pi u_b), z_odd = r sin(2 pi u_b). Every step is done
    in `dtype` (float64: the yardstick; float32: what fp32 code gives)."""
    from .secure_agg import philox4x32
    dt = np.dtype(dtype).type
    models = np.arange(K) if models is None else np.asarray(models)
    p1 = P if p1 is None else p1
    j0, j1 = p0 // 4, (max(p1, p0 + 1) + 3) // 4
    nj = j1 - j0
    ctrs = np.zeros((len(models), nj, 4), dtype=np.uint64)
    ctrs[:, :, 0] = np.arange(j0, j1, dtype=np.uint64)[None, :]
    ctrs[:, :, 1] = models.astype(np.uint64)[:, None]
    ctrs[:, :, 2] = np.uint64(int(ctr) & 0xFFFFFFFF)
    ctrs[:, :, 3] = np.uint64((int(ctr) >> 32) & 0xFFFFFFFF)
    k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF],
                 dtype=np.uint64)
    x = philox4x32(ctrs, k)                              # [M, nj, 4] uint32
    u = (x.astype(dt) + dt(0.5)) * dt(2.0 ** -32)
    out = np.empty((len(models), nj, 4), dtype=dt)
    two_pi = dt(2.0 * np.pi)
    for a in (0, 2):
        r = np.sqrt(dt(-2.0) * np.log(u[:, :, a]))
        ang = two_pi * u[:, :, a + 1]
        out[:, :, a] = r * np.cos(ang)
        out[:, :, a + 1] = r * np.sin(ang)
    flat = out.reshape(len(models), nj * 4)
    return np.ascontiguousarray(flat[:, p0 - 4 * j0:p1 - 4 * j0])


# ---------------------------------------------------------------------------
# robust_agg = trimmed_mean | median: the SPECIFICATION of the order-
# statistic aggregation (numpy). ops/hip/orderstat_kernels.hip follows it.
# The statistic is unweighted over a model's participants (its pairs with an
# aggregation weight > 0): a client can lie about its sample count as easily
# as about its parameters, so the weight only decides participation.
# ---------------------------------------------------------------------------

ORDER_KINDS = ("mean", "trimmed_mean", "median")


def ordered_key(x) -> np.ndarray:
    """uint32 keys of float32 values whose unsigned order is the total order
    -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN: ~u under a set sign
    bit, u | 0x80000000 otherwise. Agrees with np.sort on finite values."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u,
                    u | np.uint32(0x80000000)).astype(np.uint32)


def trim_count(kind: str, frac: float, n: int) -> int:
    """Rows dropped at either end of every coordinate's sorted column. At
    least one value always survives."""
    n = int(n)
    most = max(n - 1, 0) // 2
    if kind == "median":
        return most
    if kind == "trimmed_mean":
        return min(int(np.floor(frac * n + 1e-9)), most)
    raise ValueError(f"'{kind}' is not an order statistic "
                     f"({list(ORDER_KINDS[1:])})")


def order_stat_mean(values, k: int, dtype=np.float64) -> np.ndarray:
    """Per column of values [n, P] (float32): sort by ordered_key, keep
    sorted positions k .. n-k-1, sum these s = n - 2k survivors in sorted
    order in `dtype`, divide by s. s = 1 returns the selected element
    itself (no arithmetic: its bits survive), s = 2 returns (a + b) * 0.5."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    n = v.shape[0]
    k = int(k)
    s = n - 2 * k
    assert k >= 0 and s >= 1, (n, k)
    dt = np.dtype(dtype).type
    order = np.argsort(ordered_key(v), axis=0, kind="stable")
    srt = np.take_along_axis(v, order, axis=0)[k:n - k]
    with np.errstate(all="ignore"):
        if s == 1:
            return srt[0].astype(dt)
        if s == 2:
            return (srt[0].astype(dt) + srt[1].astype(dt)) * dt(0.5)
        acc = srt[0].astype(dt)
        for i in range(1, s):
            acc = acc + srt[i].astype(dt)
        return acc / dt(s)


def order_stat_aggregate(replicas, rows, model_of, weights, K: int,
                         kind: str, frac: float, out, dtype=np.float32):
    """out[m] <- order_stat_mean of model m's participant rows (the listed
    pairs with weight > 0), for every model with a participant; other rows
    of `out` ([K, P], numpy or a CPU tensor, written through a view) keep
    their bits, and `replicas` is only read. Returns (n [K], k [K])."""
    bank = replicas.detach().numpy() if isinstance(replicas, torch.Tensor) \
        else np.asarray(replicas)
    dst = out.detach().numpy() if isinstance(out, torch.Tensor) else out
    rows = np.asarray(rows, dtype=np.int64)
    mo = np.asarray(model_of, dtype=np.int64)
    sel = np.asarray(weights) > 0
    n_out = np.zeros(K, dtype=np.int64)
    k_out = np.zeros(K, dtype=np.int64)
    for m in range(K):
        r = rows[sel & (mo == m)]
        n_out[m] = len(r)
        if len(r) == 0:
            continue
        k_out[m] = trim_count(kind, frac, len(r))
        dst[m] = order_stat_mean(bank[r], k_out[m], dtype)
    return n_out, k_out


# ---------------------------------------------------------------------------
# robust_agg = multi_krum: the SPECIFICATION of Krum / Multi-Krum (Blanchard
# et al., NeurIPS 2017) in numpy float64. ops/hip/krum_kernels.hip follows
# it. A whole upload is judged by its squared L2 distances to the other
# uploads of its model, which catches what the coordinate-wise rules above
# cannot: colluders that stay inside the honest range of every coordinate.
# Unweighted over a model's participants, for the reason given above.
#
# The rule's limit: it leaves out n - s rows. If more rows than that are
# non-finite, a non-finite row is selected and the output row is non-finite.
# ---------------------------------------------------------------------------

def krum_f(frac: float, n: int) -> int:
    """Byzantine uploads assumed among n: floor(frac n), capped so that
    Krum's condition n >= 2f + 3 holds wherever it can (f = 0 below 3)."""
    n = int(n)
    return min(int(np.floor(frac * n + 1e-9)), max((n - 3) // 2, 0))


def krum_sqdist(values) -> np.ndarray:
    """D[i, j] = sum_p (double(x_ip) - double(x_jp))^2 of values [n, P]:
    direct differences (uploads are the global row plus a small update, and
    the Gram form |x|^2 + |y|^2 - 2 x.y cancels exactly there). The diagonal
    is 0; a non-finite result (a NaN or Inf coordinate) is +Inf."""
    v = np.ascontiguousarray(values, dtype=np.float32).astype(np.float64)
    n = v.shape[0]
    D = np.empty((n, n), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = v - v[i]
            D[i] = (d * d).sum(axis=1)
    D[~np.isfinite(D)] = np.inf
    D[np.arange(n), np.arange(n)] = 0.0
    return D


def krum_scores(D, f: int) -> np.ndarray:
    """score_i = the sum of the q = max(n - f - 2, 1) smallest D[i, j],
    j != i, added in ascending order; 0 for n = 1."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    if n == 1:
        return np.zeros(1, dtype=np.float64)
    q = max(n - int(f) - 2, 1)
    off = D[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    with np.errstate(all="ignore"):
        return np.cumsum(np.sort(off, axis=1)[:, :q], axis=1)[:, q - 1]


def krum_select(scores, ids, s: int) -> np.ndarray:
    """Positions of the s participants of lowest (score, id), in that
    order. Exact score ties are structural (with q = 1 two mutually nearest
    rows always tie, D being symmetric): `ids` decides them."""
    scores = np.asarray(scores, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    return np.lexsort((ids, scores))[:int(s)]


def krum_counts(n: int, frac: float, select: int):
    """(f, q, s) of a model with n >= 1 participants: s = n - f rows are
    kept (at most `select` of them when select > 0)."""
    f = krum_f(frac, n)
    q = max(n - f - 2, 1) if n >= 2 else 0
    s = n - f if select == 0 else min(int(select), n - f)
    return f, q, s


def multi_krum_aggregate(replicas, rows, model_of, weights, ids, K: int,
                         frac: float, select: int, out, dtype=np.float32):
    """out[m] <- Multi-Krum over model m's participant rows (the listed
    pairs with weight > 0; ids[i] is pair i's tie-break key), for every
    model with a participant: s = 1 stores the selected row's bits (classic
    Krum), otherwise the selected rows are added in selection order in
    `dtype` and divided by s. Other rows of `out` and `replicas` keep every
    bit. Returns (n [K], f [K], s [K], selected ids per model, scores per
    model in the pairs' order)."""
    bank = replicas.detach().numpy() if isinstance(replicas, torch.Tensor) \
        else np.asarray(replicas)
    dst = out.detach().numpy() if isinstance(out, torch.Tensor) else out
    rows = np.asarray(rows, dtype=np.int64)
    mo = np.asarray(model_of, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    sel = np.asarray(weights) > 0
    dt = np.dtype(dtype).type
    n_out = np.zeros(K, dtype=np.int64)
    f_out = np.zeros(K, dtype=np.int64)
    s_out = np.zeros(K, dtype=np.int64)
    chosen = [np.zeros(0, dtype=np.int64) for _ in range(K)]
    scores = [np.zeros(0, dtype=np.float64) for _ in range(K)]
    for m in range(K):
        pick = sel & (mo == m)
        r = rows[pick]
        n = len(r)
        n_out[m] = n
        if n == 0:
            continue
        f, _, s = krum_counts(n, frac, select)
        f_out[m], s_out[m] = f, s
        scores[m] = krum_scores(krum_sqdist(bank[r]), f)
        pos = krum_select(scores[m], ids[pick], s)
        chosen[m] = ids[pick][pos]
        if s == 1:
            dst[m] = bank[r[pos[0]]]
            continue
        with np.errstate(all="ignore"):
            acc = bank[r[pos[0]]].astype(dt)
            for i in pos[1:]:
                acc = acc + bank[r[i]].astype(dt)
            dst[m] = acc / dt(s)
    return n_out, f_out, s_out, chosen, scores


def new_server_state(kind: str) -> dict:
    if kind not in SERVER_KINDS:
        raise ValueError(f"server optimizer '{kind}' is not one of "
                         f"{list(SERVER_KINDS)}")
    return {"kind": kind, "step": 0}


@torch.no_grad()
def server_step(kind: str, global_params: torch.Tensor,
                averaged: torch.Tensor, upd: torch.Tensor, state: dict,
                lr: float = 1.0, momentum: float = 0.0) -> None:
    """global <- one server-optimizer step toward `averaged` (in place), as
    engine/server_opt.py does it with torch.optim at default hyper-
    parameters: the pseudo-gradient is global - averaged on updated rows and
    zero elsewhere, ONE step count is shared by the bank, and every row is
    stepped on every call (so Adam / momentum state of a non-updated row
    still decays and moves it). 'avg' copies the updated rows."""
    if kind not in SERVER_KINDS:
        raise ValueError(f"server optimizer '{kind}' is not one of "
                         f"{list(SERVER_KINDS)}")
    u = upd.unsqueeze(1)
    if kind == "avg":
        global_params.copy_(torch.where(u, averaged, global_params))
        return
    g = torch.where(u, global_params - averaged,
                    torch.zeros_like(global_params))
    state["step"] = t = state.get("step", 0) + 1
    if kind == "sgd":
        if momentum != 0:
            if "buf" not in state:
                state["buf"] = g.clone()
            else:
                state["buf"].mul_(momentum).add_(g)
            g = state["buf"]
        global_params.add_(g, alpha=-lr)
    elif kind == "adam":
        if "m" not in state:
            state["m"] = torch.zeros_like(global_params)
            state["v"] = torch.zeros_like(global_params)
        m, v = state["m"], state["v"]
        m.add_((g - m) * (1.0 - ADAM_B1))
        v.mul_(ADAM_B2).add_(g * g * (1.0 - ADAM_B2))
        step_size = lr / (1.0 - ADAM_B1 ** t)
        denom = v.sqrt() / ((1.0 - ADAM_B2 ** t) ** 0.5) + ADAM_EPS
        global_params.add_(m / denom, alpha=-step_size)
    else:                                                    # adagrad
        if "sum" not in state:
            state["sum"] = torch.zeros_like(global_params)
        state["sum"].add_(g * g)
        global_params.add_(g / (state["sum"].sqrt() + ADAGRAD_EPS),
                           alpha=-lr)
