"""Defended-aggregation ops (robust_fused=1): update-norm clipping with the
weighted sums, and the apply pass (average + Gaussian noise + server
optimizer step).

HIP kernels (ops/hip/robust_kernels.hip) on a CUDA device, the
specification (comm/robust.py) on CPU — so the option also runs under gloo.

A ClipPlan is the per-plan-template structure: the trained pairs grouped by
model (a CSR), uploaded once and reused every round. ServerState owns the
optimizer state ([K, P] tensors + the shared step count) across rounds.
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..comm import robust as spec
from . import hip_loader

# pairs one slice of the accumulate kernel sums at least, and the block
# count above which further slices stop paying (see hip/README.md)
PAIRS_PER_SLICE = 8
TARGET_BLOCKS = 2048
_THREADS, _ELEMS = 256, 4

_KIND = {"avg": 0, "sgd": 1, "adam": 2, "adagrad": 3}


def span() -> int:
    """Elements one block row of the accumulate kernel covers at large P."""
    return int(hip_loader.load().robust_span())


def _signed(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


class ClipPlan:
    def __init__(self, rows, models, weights, n_models: int):
        """Pair i = (replica row rows[i], model models[i], aggregation
        weight weights[i]); any order."""
        rows = np.asarray(rows, dtype=np.int64)
        models = np.asarray(models, dtype=np.int64)
        weights = np.asarray(weights, dtype=np.float32)
        order = np.argsort(models, kind="stable")
        self.order = order           # plan position -> position as given
        self.n_models = int(n_models)
        self.rows = rows[order]
        self.models = models[order]
        self.weights = weights[order]
        self.mod_off = np.zeros(n_models + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.models, minlength=n_models),
                  out=self.mod_off[1:])
        self._dev = None

    def slices(self, P: int) -> int:
        """Pair slices per model: enough blocks to fill the chip at small
        P, one slice once the element chunks alone do (CNN size)."""
        quads = -(-(P + 1) // _ELEMS)
        tq = 1
        while tq < _THREADS and tq < quads:
            tq *= 2
        chunks = -(-quads // tq)
        ty = _THREADS // tq
        most = int(np.diff(self.mod_off).max(initial=0))
        by_pairs = max(1, -(-most // PAIRS_PER_SLICE))
        by_blocks = max(1, TARGET_BLOCKS * ty // (self.n_models * chunks))
        return int(min(by_pairs, by_blocks))

    def device_tensors(self, device, n_rows: int):
        if self._dev is None:
            if len(self.rows):
                assert 0 <= self.rows.min() and self.rows.max() < n_rows, \
                    "pair row outside the replica bank"
                assert 0 <= self.models.min() and \
                    self.models.max() < self.n_models
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a),
                                          device=device)
            self._dev = (t(self.mod_off), t(self.rows),
                         t(self.models.astype(np.int32)), t(self.weights))
        return self._dev


class ParticipantPlan(ClipPlan):
    """ClipPlan restricted to the participants (aggregation weight > 0):
    what the row-reading aggregations (order statistics, Multi-Krum) share.
    `order` indexes the pairs as given; n[m] counts model m's participants."""

    def __init__(self, rows, models, weights, n_models: int):
        weights = np.asarray(weights, dtype=np.float32)
        keep = np.nonzero(weights > 0)[0]
        super().__init__(np.asarray(rows, dtype=np.int64)[keep],
                         np.asarray(models, dtype=np.int64)[keep],
                         weights[keep], n_models)
        self.order = keep[self.order]
        self.n = np.diff(self.mod_off).astype(np.int64)
        self._has = None

    def has(self, device) -> torch.Tensor:
        """[K] float: 1 for a model with a participant (uploaded once)."""
        if self._has is None:
            self._has = torch.as_tensor((self.n > 0).astype(np.float32),
                                        device=device)
        return self._has


def new_counts(n_models: int, device) -> torch.Tensor:
    """[K, 2] (clipped, seen), accumulated by clip_accumulate."""
    return torch.zeros(n_models, 2, dtype=torch.int32, device=device)


def clip_accumulate(replicas: torch.Tensor, plan: ClipPlan,
                    global_params: torch.Tensor, bound: float,
                    partial: Optional[torch.Tensor],
                    counts: torch.Tensor,
                    slices: Optional[int] = None) -> None:
    """Clip plan's replica rows in place around their global rows; with
    `partial` [K, P+1], add the weighted sums of the clipped rows (and the
    weights, slot P) into it. `counts` accumulates (clipped, seen)."""
    if replicas.device.type != "cuda":
        c, s = spec.clip_and_accumulate(
            replicas, plan.rows, plan.models, plan.weights, global_params,
            bound, partial)
        counts[:, 0] += torch.from_numpy(c).to(counts.dtype)
        counts[:, 1] += torch.from_numpy(s).to(counts.dtype)
        return
    mod_off, rows, models, weights = plan.device_tensors(
        replicas.device, replicas.shape[0])
    hip_loader.load().robust_clip(
        replicas, global_params, mod_off, rows, models, weights, partial,
        counts, float(bound),
        int(slices or plan.slices(replicas.shape[1])))


class ServerState:
    """Server-optimizer state of one job: kind, hyper-parameters, the
    shared step count and the [K, P] state tensors (allocated on first
    use, kept across rounds)."""

    def __init__(self, kind: str, lr: float = 1.0, momentum: float = 0.0):
        if kind not in _KIND:
            raise ValueError(f"server optimizer '{kind}' is not one of "
                             f"{list(spec.SERVER_KINDS)}")
        self.kind, self.lr, self.momentum = kind, float(lr), float(momentum)
        self.step = 0
        self.s0: Optional[torch.Tensor] = None
        self.s1: Optional[torch.Tensor] = None
        self.spec_state = spec.new_server_state(kind)

    def tensors(self, like: torch.Tensor):
        need0 = self.kind in ("adam", "adagrad") or \
            (self.kind == "sgd" and self.momentum != 0)
        if need0 and (self.s0 is None or self.s0.shape != like.shape):
            self.s0 = torch.zeros_like(like)
        if self.kind == "adam" and (self.s1 is None or
                                    self.s1.shape != like.shape):
            self.s1 = torch.zeros_like(like)
        return (self.s0 if need0 else None,
                self.s1 if self.kind == "adam" else None)


def apply(global_params: torch.Tensor, partial: torch.Tensor,
          mask: Optional[torch.Tensor], totals_out: torch.Tensor,
          state: ServerState, noise_std: float = 0.0, key: int = 0,
          ctr: int = 0, slabs: Optional[int] = None) -> torch.Tensor:
    """apply_aggregate's contract — rows with a positive total and a set
    mask become partial / total, `partial` is drained to zero (slot P
    included), totals land in totals_out — plus N(0, noise_std^2) noise on
    the updated rows (a pure function of key, ctr, model, element) and the
    server-optimizer step of `state`. Returns totals_out."""
    K, P = global_params.shape
    if global_params.device.type != "cuda":
        totals = partial[:, P].clone()
        upd = totals > 0
        if mask is not None:
            upd &= mask.bool()
        averaged = torch.where(
            upd.unsqueeze(1),
            partial[:, :P] * (1.0 / totals.clamp(min=1e-30)).unsqueeze(1),
            global_params)
        if noise_std > 0:
            rows = np.nonzero(upd.numpy())[0]
            if len(rows):
                z = spec.gaussian_noise(key, ctr, K, P, dtype=np.float32,
                                        models=rows)
                averaged[torch.as_tensor(rows)] += \
                    noise_std * torch.from_numpy(z).to(averaged.dtype)
        spec.server_step(state.kind, global_params, averaged, upd,
                         state.spec_state, state.lr, state.momentum)
        state.step = state.spec_state["step"]
        partial.zero_()
        totals_out.copy_(totals)
        return totals_out
    if mask is not None and mask.dtype != torch.uint8:
        mask = mask.to(torch.uint8)
    if state.kind != "avg":
        state.step += 1
    s0, s1 = state.tensors(global_params)
    hip_loader.load().robust_apply(
        global_params, partial, mask, totals_out, _KIND[state.kind], s0, s1,
        int(state.step), state.lr, state.momentum, float(noise_std),
        _signed(int(key)), _signed(int(ctr)), int(slabs or 0))
    return totals_out
