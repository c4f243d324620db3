"""The MLP round path across launches, against float64 on the CPU.

tests/test_gpu_mlp_edges.py holds every MLP kernel to float64 for ONE launch
from a zero optimizer state. The benchmark times steady-state rounds, where
each launch starts from what the previous one left: here the train kernels
load a non-zero Adam state with a rate and a step count per row (A), the
small kernel's fused broadcast / aggregation partial feeds
apply_aggregate_kernel and the next launch adds into the buffer that apply
drained (B), and FLJob runs rounds by hand on the default aggregation path
with a second plan template, a masked model and an empty plan (C). Check
bodies and bounds: tests/gpu_variant_cases.py; PARITY.md, "Round path
across launches". The 256-thread build of the small kernel runs the same
bodies in a child process (tests/test_gpu_cnn_edges.py, VARIANTS).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import gpu_variant_cases as vc  # noqa: E402
import secagg_cases as sc  # noqa: E402
from feddrift_amd.ops import mlp_hip  # noqa: E402

DEV = torch.device("cuda:0")

CARRIED = list(vc.carried_cases(small=True)) \
    + list(vc.carried_cases(small=False))
FUSED = list(vc.fused_cases())


@pytest.mark.parametrize("case,kind,d,o,lens,seed,optname", CARRIED,
                         ids=[c[0].replace(" ", "-") for c in CARRIED])
def test_carried_state_three_launches(case, kind, d, o, lens, seed, optname):
    """A: seeded m / v / vmax / t, lr per row, three launches on the same
    params and opt with a fresh permuted row subset each."""
    vc.check_carried(case, vc.carried_inputs(kind, d, o, lens, seed),
                     optname, mlp_hip, DEV)


@pytest.mark.parametrize("case,kind,d,o,masked,seed", FUSED,
                         ids=[c[0].replace(" ", "-") for c in FUSED])
def test_small_fused_partial_apply_chain(case, kind, d, o, masked, seed):
    """B: 100 pairs add into each of 3 model rows (a 4th has no pair), into
    a pre-filled partial; then train / apply (one model masked) / train into
    the drained buffer / apply."""
    vc.check_fused_chain(case, vc.fused_inputs(kind, d, o, masked, seed),
                         mlp_hip, DEV)


def test_fljob_rounds_default_path(tmp_path):
    """C: nine rounds by hand on the fused default path."""
    job = sc.make_job(tmp_path, secure_agg=0, use_hip_kernels="always")
    assert job.device.type == "cuda" and job.backend is mlp_hip
    figs = vc.drive_fljob_rounds(job, "fljob hip", drained=True)
    assert figs["mean/bound"] <= 1.0
    # the rounds went through the per-template staging and constant cache
    tmpl = job.algo._tmpl
    stage = tmpl.cache["stage", job.cfg.epochs][1]
    train = tmpl.cache["train"][1]
    assert stage["buf"].shape[1] == len(tmpl.rows)
    assert train[0].numel() == len(tmpl.rows)
