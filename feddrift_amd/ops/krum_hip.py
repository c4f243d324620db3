"""Multi-Krum aggregation op (robust_agg = multi_krum): per model, the
participants whose uploads lie closest to the others' are kept and averaged.

HIP kernels (ops/hip/krum_kernels.hip) on a CUDA device, the specification
(comm/robust.py, float32 mean) on CPU — so the option also runs under gloo.

A KrumPlan is robust_hip.ParticipantPlan (ClipPlan's pairs-by-model CSR
restricted to the participants, aggregation weight > 0) plus every
participant's tie-break id and the per-model counts f, q, s, computed on the
host. On a GPU nothing
is copied back in a steady-state aggregation: scores and the selection stay
on the device until last_selection() asks for them.
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..comm import robust as spec
from . import hip_loader
from .robust_hip import ParticipantPlan


def tile() -> int:
    """Rows of either tile of the distance kernel."""
    return int(hip_loader.load().krum_tile())


def chunk() -> int:
    """Coordinates one block of the distance kernel covers; a longer vector
    is split and its partial distances are added in chunk order."""
    return int(hip_loader.load().krum_chunk())


def score_lds() -> int:
    """Entries of a distance row the score kernel keeps in LDS; the rest of
    a longer row streams from global memory on every pass."""
    return int(hip_loader.load().krum_score_lds())


def scratch_rows() -> int:
    """Default bound on the distance rows of one model held at once."""
    return int(hip_loader.load().krum_scratch_rows())


def scratch_layout(n, n_split: int, rows_bound: int, budget: int):
    """(slab, d_off [K], need): the largest slab <= rows_bound such that the
    per-model [n_split, min(slab, n), n] blocks of doubles fit `budget`
    elements together; d_off is every model's first element."""
    n = np.asarray(n, dtype=np.int64)
    n_max = int(n.max(initial=0))
    if n_max == 0:
        return 1, np.zeros(len(n), dtype=np.int64), 0

    def total(slab):
        return int(n_split) * int((np.minimum(slab, n) * n).sum())

    slab = max(1, min(int(rows_bound), n_max, 65535))
    if total(slab) > budget:
        lo, hi = 1, slab                 # total() is monotone in slab
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if total(mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        slab = lo
    if total(slab) > budget:
        raise ValueError(
            f"multi_krum: one distance row of every model needs "
            f"{total(1)} doubles, more than the scratch bound {budget}")
    sizes = int(n_split) * np.minimum(slab, n) * n
    d_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return slab, d_off, int(sizes.sum())


class KrumPlan(ParticipantPlan):
    def __init__(self, rows, models, weights, n_models: int, frac: float,
                 select: int = 0, ids=None):
        """Pair i = (bank row rows[i], model models[i], weight weights[i],
        tie-break key ids[i]); any order. Pairs with weight <= 0 do not
        participate. ids default to the pairs' positions."""
        rows = np.asarray(rows, dtype=np.int64)
        ids = np.arange(len(rows), dtype=np.int64) if ids is None \
            else np.asarray(ids, dtype=np.int64)
        assert ids.shape == rows.shape
        super().__init__(rows, models, weights, n_models)
        self.ids = ids[self.order]   # ids follow the grouping by model
        self.frac, self.select = float(frac), int(select)
        cnt = [spec.krum_counts(n, frac, select) if n else (0, 0, 0)
               for n in self.n]
        self.f = np.array([c[0] for c in cnt], dtype=np.int32)
        self.q = np.array([c[1] for c in cnt], dtype=np.int32)
        self.s = np.array([c[2] for c in cnt], dtype=np.int32)
        self._krum_dev = None
        self._layouts = {}
        self._scratch = None         # (tensor, slab, d_off): the last launch
        self._spec_result = None     # CPU path: (selected ids, scores)

    def device_tensors(self, device, n_rows: int):
        first = self._dev is None
        mod_off, rows, _, _ = super().device_tensors(device, n_rows)
        if first:
            live = self.n > 0
            assert int(self.mod_off[-1]) == len(self.rows)
            assert np.all((self.q >= 0) & ((self.q < self.n) | ~live))
            assert np.all(((self.s >= 1) & (self.s <= self.n)) | ~live)
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a),
                                          device=device)
            U = len(self.rows)
            self._krum_dev = (
                t(self.ids), t(self.q), t(self.s),
                torch.zeros(U, dtype=torch.float64, device=device),
                torch.zeros(U, dtype=torch.int32, device=device))
        return (mod_off, rows) + self._krum_dev

    def layout(self, device, P: int, rows_bound: int):
        """The cached scratch layout of vectors of length P under
        `rows_bound`: (slab, d_off on the host, d_off on the device, need)."""
        key = (int(P), int(rows_bound))
        hit = self._layouts.get(key)
        if hit is None:
            mod = hip_loader.load()
            n_split = max(1, -(-int(P) // int(mod.krum_chunk())))
            slab, d_off, need = scratch_layout(
                self.n, n_split, rows_bound, int(mod.krum_scratch_elems()))
            hit = (slab, d_off, torch.as_tensor(d_off, device=device), need)
            self._layouts[key] = hit
        return hit


_scratch_cache = {}


def _scratch(device, need: int) -> torch.Tensor:
    """One growing float64 buffer per device, shared by every plan."""
    buf = _scratch_cache.get(device)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, 1), dtype=torch.float64, device=device)
        _scratch_cache[device] = buf
    return buf


def aggregate(bank: torch.Tensor, plan: KrumPlan, out: torch.Tensor,
              scratch_rows: Optional[int] = None) -> None:
    """out[m] <- Multi-Krum over model m's participant rows of `bank`
    ([R, P]), for every model with a participant; the other rows of `out`
    ([K, P], unit column stride) and the bank keep every bit. At most
    `scratch_rows` distance rows of a model are held at once (default:
    krum_scratch_rows(), and never more than 1 GiB of scratch); the result
    does not depend on it."""
    assert out.shape == (plan.n_models, bank.shape[1])
    if bank.device.type != "cuda":
        _, _, _, chosen, scores = spec.multi_krum_aggregate(
            bank, plan.rows, plan.models, plan.weights, plan.ids,
            plan.n_models, plan.frac, plan.select, out, dtype=np.float32)
        plan._spec_result = (chosen, scores)
        return
    if scratch_rows is not None and scratch_rows < 1:
        raise ValueError(f"scratch_rows must be >= 1, got {scratch_rows}")
    mod = hip_loader.load()
    mod_off, rows, ids, q, s, scores, sel = plan.device_tensors(
        bank.device, bank.shape[0])
    if len(plan.rows) == 0:
        return
    bound = int(scratch_rows or mod.krum_scratch_rows())
    slab, d_off_host, d_off, need = plan.layout(bank.device, bank.shape[1],
                                                bound)
    buf = _scratch(bank.device, need)
    plan._scratch = (buf, slab, d_off_host)
    mod.krum(bank, mod_off, rows, ids, q, s, d_off, buf, scores, sel, out,
             int(plan.n.max()), int(slab), int(need))


def last_selection(plan: KrumPlan, with_scores: bool = False):
    """Per model, the ids kept by the last aggregate() on this plan, in
    (score, id) order; with_scores adds every participant's score per model
    (in the plan's participant order). On a GPU this synchronises and
    copies; nothing else in the op does."""
    K = plan.n_models
    if plan._spec_result is not None:
        chosen, scores = plan._spec_result
    elif plan._krum_dev is not None:
        _, _, _, sc_t, sel_t = plan._krum_dev
        sel, sc = sel_t.cpu().numpy(), sc_t.cpu().numpy()
        off = plan.mod_off
        chosen = [plan.ids[sel[off[m]:off[m] + plan.s[m]]] if plan.n[m]
                  else np.zeros(0, dtype=np.int64) for m in range(K)]
        scores = [sc[off[m]:off[m + 1]] for m in range(K)]
    else:
        raise RuntimeError("last_selection: the plan has not aggregated yet")
    return (chosen, scores) if with_scores else chosen


def last_distances(plan: KrumPlan, m: int) -> np.ndarray:
    """Test accessor: model m's [n, n] distance matrix as the last GPU
    aggregate() left it in the scratch. Whole only when the launch held the
    model in one slab and nothing has reused the scratch since."""
    buf, slab, d_off = plan._scratch
    n = int(plan.n[m])
    assert slab >= n, "the last launch held this model in row slabs"
    return buf[int(d_off[m]):int(d_off[m]) + n * n].cpu().numpy() \
        .reshape(n, n)
