"""Ring-arithmetic secure aggregation ops (secure_agg=2).

HIP kernels (ops/hip/secagg_kernels.hip) on a CUDA device, the numpy
specification (comm/secure_agg.py) on CPU — so the mode also runs under
gloo. Both produce identical bits.

A SecaggPlan is the per-(iteration, active set) structure: this rank's
uploads grouped by model, plus the mask graph as a CSR edge list. It is
built once on the host, uploaded once, and reused every round; the pair
keys are derived on the device from (job key, aggregation counter, model,
pair), so a steady-state round uploads nothing.
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..comm import secure_agg as sa
from . import hip_loader

# uploads one slice of the mask kernel sums at least (see hip/README.md)
UPLOADS_PER_SLICE = 8
MAX_SLICES = 1024


def span() -> int:
    """Elements one block row of the mask kernel covers at large P."""
    return int(hip_loader.load().secagg_span())


class SecaggPlan:
    def __init__(self, rows, workers, models, weights, n_models: int,
                 graph: sa.MaskGraph):
        """Upload i = (replica row rows[i], global worker workers[i], model
        models[i], weight weights[i]); any order."""
        rows = np.asarray(rows, dtype=np.int64)
        workers = np.asarray(workers, dtype=np.int64)
        models = np.asarray(models, dtype=np.int64)
        weights = np.asarray(weights, dtype=np.float32)
        order = np.argsort(models, kind="stable")
        self.n_models = int(n_models)
        self.graph = graph
        self.rows = rows[order]
        self.workers = workers[order]
        self.models = models[order]
        self.weights = weights[order]
        self.mod_off = np.zeros(n_models + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.models, minlength=n_models),
                  out=self.mod_off[1:])
        # CSR edges. A complete-graph model stores its active list ONCE and
        # every upload of it points there (the kernel skips the upload's own
        # worker); a degree-d model stores d neighbours per upload.
        es = np.zeros(len(rows), dtype=np.int32)
        ec = np.zeros(len(rows), dtype=np.int32)
        edges = []
        n_edges = 0
        for m in range(n_models):
            lo, hi = self.mod_off[m], self.mod_off[m + 1]
            act = graph.active[m]
            if hi == lo or len(act) < 2:
                continue
            if graph.nbr[m] is None:
                es[lo:hi] = n_edges
                ec[lo:hi] = len(act)
                edges.append(act)
                n_edges += len(act)
            else:
                nb = np.stack([graph.nbr[m][int(w)]
                               for w in self.workers[lo:hi]])
                d = nb.shape[1]
                es[lo:hi] = n_edges + d * np.arange(hi - lo)
                ec[lo:hi] = d
                edges.append(nb.reshape(-1))
                n_edges += nb.size
        self.up_es, self.up_ec = es, ec
        self.edge_other = (np.concatenate(edges) if edges
                           else np.zeros(0, np.int64)).astype(np.int32)
        counts = np.diff(self.mod_off)
        self.slices = int(min(MAX_SLICES, max(
            1, -(-int(counts.max(initial=0)) // UPLOADS_PER_SLICE))))
        self._dev = None

    def device_tensors(self, device, n_rows: int):
        if self._dev is None:
            if len(self.rows):
                assert 0 <= self.rows.min() and self.rows.max() < n_rows, \
                    "upload row outside the replica bank"
                assert int((self.up_es + self.up_ec).max()) <= \
                    len(self.edge_other)
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a),
                                          device=device)
            self._dev = (t(self.mod_off), t(self.rows),
                         t(self.workers.astype(np.int32)), t(self.weights),
                         t(self.up_es), t(self.up_ec), t(self.edge_other))
        return self._dev


def _signed(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def new_flag(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def contribution(replicas: torch.Tensor, plan: SecaggPlan, base: int,
                 agg_ctr: int, frac_bits: int, n_workers: int,
                 rank: int = 0, world: int = 1, skip_intra: bool = True,
                 flag: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """This rank's [K, P+1] int64 contribution in [0, 2^56) and the sticky
    range-guard flag (int32[1], nonzero once any element violated)."""
    if flag is None:
        flag = new_flag(replicas.device)
    if replicas.device.type != "cuda":
        out, bad = sa.ring_contribution(
            replicas.numpy(), plan.rows, plan.workers, plan.models,
            plan.weights, plan.n_models, plan.graph, base, agg_ctr,
            frac_bits, n_workers, rank, world, skip_intra)
        if bad:
            flag.fill_(1)
        return torch.from_numpy(out), flag
    mod_off, rows, workers, weights, es, ec, edges = plan.device_tensors(
        replicas.device, replicas.shape[0])
    out = hip_loader.load().secagg_mask(
        replicas, mod_off, rows, workers, weights, es, ec, edges, flag,
        _signed(base), int(agg_ctr), int(frac_bits), int(n_workers),
        int(rank), int(world), bool(skip_intra), plan.slices)
    return out, flag


def dequantise(ring: torch.Tensor, out: torch.Tensor, frac_bits: int) -> None:
    """All-reduced ring sums [K, P+1] int64 -> float32 `out` (same shape)."""
    if ring.device.type != "cuda":
        out.copy_(torch.from_numpy(
            sa.dequantise(ring.numpy(), frac_bits)).reshape(out.shape))
        return
    hip_loader.load().secagg_dequant(ring, out, int(frac_bits))


def check_flag(flag: torch.Tensor, frac_bits: int) -> None:
    """Raise if the range guard fired (synchronises on a CUDA device)."""
    if int(flag.item()) != 0:
        raise sa.guard_error(frac_bits)
