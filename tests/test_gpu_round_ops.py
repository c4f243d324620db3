"""The small-fleet round's step windows in the train launch's arguments, on
the GPU (bodies and their reasoning: tests/round_ops_cases.py)."""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import round_ops_cases as rc  # noqa: E402
import train_chain_cases as tc  # noqa: E402
from feddrift_amd.ops import hip_loader  # noqa: E402

INLINE = rc.inline_cases(tc.CHAIN_LENS, tc.CHAIN_SEEDS)


def _child(case, env, marker):
    hip_loader.load()                  # the child must find it built
    r = subprocess.run([sys.executable, rc.__file__, case],
                       env=dict(os.environ, **env), timeout=240,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-4000:])
    assert marker in r.stdout


@pytest.mark.parametrize("c", INLINE,
                         ids=[c[0].replace(" ", "-") for c in INLINE])
def test_inline_steps_same_bits(c):
    """G = 6, E = 4, lengths (0, 1, 64, 511, 512, 513, 600): CPU step
    tensors (in the launch arguments) against device step tensors."""
    rc.check_inline_chain(c, tc.CHAIN_LENS)


@pytest.mark.parametrize("G", [64, 65])
def test_inline_steps_at_and_over_the_cap(G):
    rc.check_cap(G)


def test_inline_steps_256_thread_blocks():
    _child("inline_bs256", {"FEDDRIFT_TRAIN_BS64_MIN_G": "1000000"},
           "case inline_bs256 OK")


def test_fljob_rounds_on_both_step_routes(tmp_path):
    """Nine rounds by hand, once with the step windows in the launch
    arguments and once through the pinned upload (FLJob.inline_steps off):
    the per-template staging buffer shows which route ran (a CPU tensor
    that the launch reads, or the device tensor the DMA fills), and both
    keep the rounds' float64 bounds. (Launch-level bit equality of the
    routes: the tests above; here four pairs add into each partial row in
    arrival order, so two jobs need not agree in the last bit.)"""
    import gpu_variant_cases as vc
    import secagg_cases as sc
    from feddrift_amd.ops import mlp_hip
    for inline in (True, False):
        job = sc.make_job(tmp_path / f"inline{int(inline)}", secure_agg=0,
                          use_hip_kernels="always")
        job.inline_steps = inline
        assert job.device.type == "cuda" and job.backend is mlp_hip
        figs = vc.drive_fljob_rounds(job, f"fljob inline={int(inline)}",
                                     drained=True)
        assert figs["mean/bound"] <= 1.0
        tmpl = job.algo._tmpl
        stage = tmpl.cache["stage", job.cfg.epochs][1]
        assert stage["inline"] == inline
        assert stage["buf"].shape[1] == len(tmpl.rows)
        assert stage["buf"].device.type == ("cpu" if inline else "cuda")
