"""Order-statistic aggregation op (robust_agg = trimmed_mean | median): the
coordinate-wise trimmed mean of every model's participant rows.

HIP kernel (ops/hip/orderstat_kernels.hip) on a CUDA device, the
specification (comm/robust.py, float32) on CPU — so the option also runs
under gloo.

An OrderStatPlan is robust_hip.ParticipantPlan (ClipPlan's pairs-by-model
CSR restricted to the participants, aggregation weight > 0) plus the
per-model trim count k, computed on the host.
"""

from __future__ import annotations

import numpy as np
import torch

from ..comm import robust as spec
from . import hip_loader
from .robust_hip import ParticipantPlan


def tile() -> int:
    """Coordinates one block of the kernel covers (TP)."""
    return int(hip_loader.load().orderstat_tp())


def lds_rows() -> int:
    """Participants of one model up to which the kernel keeps the model's
    key tile in LDS; above it every pass streams from global memory."""
    return int(hip_loader.load().orderstat_lds_rows())


def small_rows() -> int:
    """Participants of one model up to which the one-thread-per-coordinate
    rank kernel takes it (a CNN fleet); above, the block-per-tile kernel."""
    return int(hip_loader.load().orderstat_small_rows())


class OrderStatPlan(ParticipantPlan):
    def __init__(self, rows, models, weights, n_models: int, kind: str,
                 frac: float = 0.0):
        """Pair i = (bank row rows[i], model models[i], weight weights[i]);
        any order. Pairs with weight <= 0 do not participate."""
        if kind not in spec.ORDER_KINDS[1:]:
            raise ValueError(f"'{kind}' is not an order statistic")
        super().__init__(rows, models, weights, n_models)
        self.kind, self.frac = kind, float(frac)
        self.k = np.array([spec.trim_count(kind, frac, n) for n in self.n],
                          dtype=np.int32)
        self._k_dev = None
        self._which = None           # (a small model, a large model)

    def device_tensors(self, device, n_rows: int):
        first = self._dev is None
        mod_off, rows, _, _ = super().device_tensors(device, n_rows)
        if first:
            assert int(self.mod_off[-1]) == len(self.rows)
            assert np.all(self.k >= 0) and \
                np.all((2 * self.k < self.n) | (self.n == 0)), \
                "trim count leaves no survivor"
            self._k_dev = torch.as_tensor(self.k, device=device)
        return mod_off, rows, self._k_dev


def aggregate(bank: torch.Tensor, plan: OrderStatPlan,
              out: torch.Tensor) -> None:
    """out[m] <- the plan's order statistic over model m's participant rows
    of `bank` ([R, P]), for every model with a participant; the other rows
    of `out` ([K, P], unit column stride) and the bank keep every bit."""
    assert out.shape == (plan.n_models, bank.shape[1])
    if bank.device.type != "cuda":
        spec.order_stat_aggregate(bank, plan.rows, plan.models, plan.weights,
                                  plan.n_models, plan.kind, plan.frac, out,
                                  dtype=np.float32)
        return
    mod_off, rows, k = plan.device_tensors(bank.device, bank.shape[0])
    if plan._which is None:
        small = small_rows()
        plan._which = (bool(np.any((plan.n > 0) & (plan.n <= small))),
                       bool(np.any(plan.n > small)))
    hip_loader.load().order_stat(bank, mod_off, rows, k, out, *plan._which)
