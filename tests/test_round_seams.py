"""The seams of a federated round, on the CPU.

The CPU twin of tests/test_gpu_mlp_rounds.py: the same check bodies
(tests/gpu_variant_cases.py) with fp32 mlp_torch standing in for the HIP
kernels. That pins the drivers and their bounds where no GPU is present —
an honest fp32 implementation has to pass them — and holds the unfused
round path of engine/fljob.py (sync_replicas + einsum) to the same float64
references as the fused one. Bounds: PARITY.md, "Round path across
launches".
"""

import pytest
import torch

import gpu_variant_cases as vc
import secagg_cases as sc
from feddrift_amd.ops import mlp_torch


def test_round_bounds_are_the_measured_err32():
    """The frozen table is what measure_round_err32() reports (parts A and
    B, all cases): fp32 torch passes every check body, and its largest
    error is the table's, up to what another CPU's BLAS rounds differently
    (seen: 1 % on m)."""
    worst = vc.measure_round_err32()
    for q, e32 in worst.items():
        assert e32 / 1.25 <= vc.ROUND_TRAIN_ERR32[q] <= 1.25 * e32, (q, e32)
    # no ill-conditioned draw among the seeds
    assert worst["param"] <= 1e-5


@pytest.mark.parametrize("what", ["plain", "special"])
def test_fljob_rounds_unfused_path(tmp_path, what):
    """Part C on device="cpu": backend mlp_torch, replicas synced from the
    global rows, aggregation by einsum; _partial is not drained there."""
    job = sc.make_job(tmp_path, device=torch.device("cpu"), secure_agg=0)
    assert job.backend is mlp_torch and job.device.type == "cpu"
    rounds = ("plan",) * 4 if what == "plain" else vc.JOB_ROUNDS
    figs = vc.drive_fljob_rounds(job, f"fljob cpu {what}", drained=False,
                                 rounds=rounds)
    assert figs["mean/bound"] <= 1.0
