"""Upload compression op (upload_compress = topk): every trained replica row
keeps the k largest-magnitude coordinates of its update (plus the pair's
error-feedback residual) and falls back to the global row elsewhere. Under
quant / topk_quant what travels (every non-zero coordinate / the top k) is
stochastically rounded to `bits` bits against the row's largest magnitude.

HIP kernels (ops/hip/compress_kernels.hip) on a CUDA device, the
specification (comm/compress.py) on CPU — so the option also runs under gloo.

A CompressPlan is the per-plan-template structure: the trained pairs' replica
rows, models and (for the quantiser's draws) global worker ids, uploaded once
and reused every round. On a GPU a
steady-state call enqueues kernels only.
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..comm import compress as spec
from . import hip_loader


def wave_max() -> int:
    """Row length up to which one wave takes a pair (four pairs a block)."""
    return int(hip_loader.load().compress_wave_max())


def row_max() -> int:
    """The switch length: rows up to it take a row kernel (one block per
    pair at most), longer rows the radix path."""
    return int(hip_loader.load().compress_row_max())


def chunk() -> int:
    """Coordinates one block of the long path covers."""
    return int(hip_loader.load().compress_chunk())


def slab_rows() -> int:
    """Default bound on the pairs the long path holds histograms for."""
    return int(hip_loader.load().compress_slab_rows())


class CompressPlan:
    def __init__(self, rows, models, n_models: int, workers=None):
        """Pair i = (replica row rows[i], model models[i]); any order, every
        row at most once. workers[i] is the pair's global worker id, which
        the quantised kinds need."""
        self.rows = np.asarray(rows, dtype=np.int64)
        self.models = np.asarray(models, dtype=np.int64)
        assert self.rows.shape == self.models.shape
        self.workers = None
        if workers is not None:
            self.workers = np.asarray(workers, dtype=np.int64)
            assert self.workers.shape == self.rows.shape
            assert self.workers.size == 0 or \
                (0 <= self.workers.min() and self.workers.max() < 2 ** 31)
        self._dev_workers = None
        assert len(np.unique(self.rows)) == len(self.rows), \
            "a replica row is listed twice"
        self.n_models = int(n_models)
        self.n = np.bincount(self.models, minlength=n_models).astype(np.int64)
        self._dev = None
        self._totals = {}

    def device_tensors(self, device, n_rows: int):
        if self._dev is None:
            if len(self.rows):
                assert 0 <= self.rows.min() and self.rows.max() < n_rows, \
                    "pair row outside the replica bank"
                assert 0 <= self.models.min() and \
                    self.models.max() < self.n_models
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a),
                                          device=device)
            self._dev = (t(self.rows), t(self.models.astype(np.int32)))
        return self._dev

    def device_workers(self, device) -> torch.Tensor:
        assert self.workers is not None, \
            "the plan was built without global worker ids"
        if self._dev_workers is None:
            self._dev_workers = torch.as_tensor(
                np.ascontiguousarray(self.workers.astype(np.int32)),
                device=device)
        return self._dev_workers

    def totals(self, device, P: int) -> torch.Tensor:
        """[K, 2] int64 (0, pairs * P): what one pass adds to slot 1."""
        hit = self._totals.get(int(P))
        if hit is None:
            add = np.zeros((self.n_models, 2), dtype=np.int64)
            add[:, 1] = self.n * int(P)
            hit = torch.as_tensor(add, device=device)
            self._totals[int(P)] = hit
        return hit


def new_counts(n_models: int, device) -> torch.Tensor:
    """[K, 2] (sent coordinates, pairs * P), accumulated by topk."""
    return torch.zeros(n_models, 2, dtype=torch.int64, device=device)


_scratch_cache = {}


def _scratch(device, slab: int):
    """Histograms, thresholds and wanted ranks of one slab; one growing set
    per device, shared by every plan."""
    hit = _scratch_cache.get(device)
    if hit is None or hit[1].numel() < slab:
        bins = int(hip_loader.load().compress_bins())
        hit = (torch.zeros(slab * bins, dtype=torch.int32, device=device),
               torch.zeros(slab, dtype=torch.int32, device=device),
               torch.zeros(slab, dtype=torch.int32, device=device))
        _scratch_cache[device] = hit
    return hit


_scale_cache = {}


def _scale_scratch(device, slab: int) -> torch.Tensor:
    """The long path's per-pair scale slots of one slab."""
    hit = _scale_cache.get(device)
    if hit is None or hit.numel() < slab:
        hit = torch.zeros(slab, dtype=torch.int32, device=device)
        _scale_cache[device] = hit
    return hit


def _dispatch(mod, replicas, plan, P, switch, slab):
    """(switch length, slab, hist, tau, krem) of one call."""
    most = int(mod.compress_row_max())
    sw = most if switch is None else int(switch)
    if not 0 <= sw <= most:
        raise ValueError(f"switch must lie in [0, {most}], got {switch}")
    n_slab = int(mod.compress_slab_rows()) if slab is None else int(slab)
    if n_slab < 1:
        raise ValueError(f"slab must be >= 1, got {slab}")
    n_slab = min(n_slab, len(plan.rows), 65535)
    if P > sw:
        hist, tau, krem = _scratch(replicas.device, n_slab)
    else:
        hist = tau = krem = _scratch(replicas.device, 1)[1]
    return sw, n_slab, hist, tau, krem


def topk(replicas: torch.Tensor, plan: CompressPlan,
         global_params: torch.Tensor, residual: Optional[torch.Tensor],
         k: int, counts: torch.Tensor, switch: Optional[int] = None,
         slab: Optional[int] = None) -> None:
    """Compress plan's replica rows in place around their global rows,
    keeping the k coordinates of largest magnitude (ties included);
    `residual` (the replicas' shape, or None for no error feedback) is added
    to the update first and takes what was held back. `counts` [K, 2] int64
    accumulates (sent, pairs * P). `switch` lowers the row length above
    which the long path runs and `slab` bounds its pairs per pass (tests
    drive the long path at tiny P with them); the result depends on
    neither."""
    P = replicas.shape[1]
    if not 1 <= int(k) <= P:
        raise ValueError(f"k must lie in [1, {P}], got {k}")
    if residual is not None:
        assert residual.shape == replicas.shape
    assert global_params.shape == (plan.n_models, P)
    assert counts.shape == (plan.n_models, 2)
    if replicas.device.type != "cuda":
        spec.topk_compress(replicas, plan.rows, plan.models, global_params,
                           residual, int(k), counts)
        return
    mod = hip_loader.load()
    rows, models = plan.device_tensors(replicas.device, replicas.shape[0])
    if len(plan.rows) == 0:
        return
    sw, n_slab, hist, tau, krem = _dispatch(mod, replicas, plan, P, switch,
                                            slab)
    mod.compress_topk(replicas, global_params, residual, rows, models,
                      counts, int(k), sw, hist, tau, krem, n_slab)
    counts.add_(plan.totals(replicas.device, P))


def quant(replicas: torch.Tensor, plan: CompressPlan,
          global_params: torch.Tensor, residual: Optional[torch.Tensor],
          k: int, bits: int, key: int, ctr: int, counts: torch.Tensor,
          switch: Optional[int] = None, slab: Optional[int] = None) -> None:
    """topk() with stochastic quantisation of what travels to `bits` bits
    per coordinate (comm/compress.py:quant_rows): k = 0 quantises every
    non-zero coordinate (quant), k >= 1 the k of largest magnitude
    (topk_quant). `key` is the job's quant_key and `ctr` its compress-pass
    counter; the plan carries the pairs' global worker ids. The residual
    takes the quantisation error as well. `counts` slot 0 gains the
    coordinates written from g + ... ."""
    P = replicas.shape[1]
    if not 0 <= int(k) <= P:
        raise ValueError(f"k must lie in [0, {P}], got {k}")
    L = spec.levels(bits)                        # asserts the range
    if residual is not None:
        assert residual.shape == replicas.shape
    assert global_params.shape == (plan.n_models, P)
    assert counts.shape == (plan.n_models, 2)
    assert plan.workers is not None, \
        "the plan was built without global worker ids"
    assert L >= 1 and 0 <= int(key) < 2 ** 64 and int(ctr) >= 0
    if replicas.device.type != "cuda":
        spec.quant_compress(replicas, plan.rows, plan.models, plan.workers,
                            global_params, residual, int(k), int(bits),
                            int(key), int(ctr), counts)
        return
    mod = hip_loader.load()
    rows, models = plan.device_tensors(replicas.device, replicas.shape[0])
    if len(plan.rows) == 0:
        return
    workers = plan.device_workers(replicas.device)
    sw, n_slab, hist, tau, krem = _dispatch(mod, replicas, plan, P, switch,
                                            slab)
    smax = _scale_scratch(replicas.device, n_slab if P > sw else 1)
    mod.compress_quant(replicas, global_params, residual, rows, models,
                       workers, counts, int(k), int(bits), int(key),
                       int(ctr) & 0xFFFFFFFF, sw, hist, tau, krem, smax,
                       n_slab)
    counts.add_(plan.totals(replicas.device, P))
