"""The seams of a federated round, on the CPU.

The CPU twin of tests/test_gpu_mlp_rounds.py: the same check bodies
(tests/gpu_variant_cases.py) with fp32 mlp_torch standing in for the HIP
kernels. That pins the drivers and their bounds where no GPU is present —
an honest fp32 implementation has to pass them — and holds the unfused
round path of engine/fljob.py (sync_replicas + einsum) to the same float64
references as the fused one. Bounds: PARITY.md, "Round path across
launches".
"""

import dataclasses

import numpy as np
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


def test_template_cache_follows_sample_num(tmp_path):
    """Every per-template constant is keyed on the identity of the plan's
    sample_num: a plan that keeps its template and carries a new weight
    array gets every slot rebuilt from the new weights, and a plan without
    a template stores nothing."""
    def weights_of(name, val):
        if name == "pairs":
            return val[2]
        if name == "train":
            return val[2].numpy()
        if name in ("orderstat", "krum"):
            return val[0].weights
        return getattr(val, "weights", None)         # compress: none

    options = [
        (dict(robust_fused=1, robust_norm_bound=0.5, upload_compress="topk"),
         {"pairs", "train", "clip", "compress"}),
        (dict(robust_agg="median"), {"pairs", "train", "orderstat"}),
        (dict(robust_agg="multi_krum"), {"pairs", "train", "krum"}),
        (dict(secure_agg=2), {"pairs", "train", "secagg"}),
    ]
    for kw, want in options:
        job = sc.make_job(tmp_path, device=torch.device("cpu"), **kw)
        ci = job.client_sampling(0)

        def round_(plan):
            job.train(plan)
            # the staged launch's constants: the HIP path builds them
            job.cached(plan, "train", lambda: job._train_constants(plan))
            job.aggregate(plan)

        plan = job.algo.plan(job, 0, ci)
        tmpl = plan.template
        round_(plan)
        slots = {s for s in tmpl.cache if not isinstance(s, tuple)}
        assert slots == want, (kw, slots)
        first = {s: tmpl.cache[s] for s in slots}
        round_(job.algo.plan(job, 1, ci))                 # same array: hits
        assert all(tmpl.cache[s] is first[s] for s in slots), kw

        doubled = dataclasses.replace(
            job.algo.plan(job, 2, ci),
            sample_num=np.asarray(plan.sample_num) * 2)
        assert doubled.template is tmpl
        round_(doubled)
        for s in slots:
            key, val = tmpl.cache[s]
            assert key is doubled.sample_num, (kw, s)
            assert val is not first[s][1], (kw, s)
            w0, w1 = weights_of(s, first[s][1]), weights_of(s, val)
            if w0 is not None:
                assert len(w0) and np.array_equal(w1, 2 * w0), (kw, s)

        kept = dict(tmpl.cache)
        bare = dataclasses.replace(job.algo.plan(job, 3, ci), template=None,
                                   sample_num=np.asarray(plan.sample_num) * 3)
        round_(bare)
        assert tmpl.cache.keys() == kept.keys(), kw
        assert all(tmpl.cache[s] is kept[s] for s in kept), kw
