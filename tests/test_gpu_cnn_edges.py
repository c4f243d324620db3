"""CNN kernel pipeline (ops/hip/cnn_kernels.hip) at its tile, chunk and
dispatch edges, against float64 autograd / forward on the CPU.

The existing tests/test_gpu_cnn.py compares fp32 end to end at batch <= 8;
here every layer's gradient is compared on its own, at batches that cross
the 16-row MFMA fragment and the 64-row m-tile, with the conv2-wgrad
pipeline owning more than one tile per block, for O = 62, with input
masks and with live dropout; the eval sweep is checked per sample. Bounds
and their derivation: tests/gpu_variant_cases.py and PARITY.md ("Kernel
edge and variant coverage").
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import gpu_variant_cases as vc  # noqa: E402

DEV = torch.device("cuda:0")


# --------------------------------------------------------------------------
# per-layer gradient parity
# --------------------------------------------------------------------------

def test_cnn_grad_edges_then_shrinking_workspace():
    eng, world = vc.case_cnn_grad_edges()
    # second launch on the SAME engine with a smaller G and B: the reused
    # workspace (and its stored w2ms) is larger than the launch's own sizes
    ws = eng._ws
    plan = vc.cnn_plan([9, 4, 2], seed=3)
    run = vc.cnn_sgd_epoch(eng, world, plan)
    assert eng._ws is ws and ws["G"] == 8 and ws["B"] == 65
    vc.check_cnn_grads("cnn grad reuse G=3 B=9", world, plan, run)


@pytest.mark.parametrize("w2ms", [1, 3])
def test_cnn_grad_w2ms(monkeypatch, w2ms):
    """FEDDRIFT_W2MS=1: one block walks all 9 * 65 = 585 conv2-wgrad tiles
    through the double-buffered pipeline (the fleet-scale path); 3: a
    block's tiles interleave samples. Read when the workspace is made."""
    monkeypatch.setenv("FEDDRIFT_W2MS", str(w2ms))
    eng, _ = vc.case_cnn_grad_edges(case=f"cnn grad B=65 w2ms={w2ms}")
    assert eng._ws["w2ms"] == w2ms


def test_cnn_grad_o62():
    """FEMNIST head: lanes 62/63 dead, dz2 stride 62, and P % 4 == 2 takes
    the scalar tail of cnn_opt_step."""
    world = vc.cnn_world(62, K=2, seed=4)
    assert world["P"] == 1206590 and world["P"] % 4 == 2
    plan = vc.cnn_plan([1, 17, 33], seed=5)
    run = vc.cnn_sgd_epoch(vc.cnn_engine(world), world, plan)
    vc.check_cnn_grads("cnn grad O=62", world, plan, run)


def test_cnn_adam_o62_two_steps():
    """Adam(amsgrad) at O = 62 against _apply_update fed the kernel's own
    gradient bits (wd = 0 for the reason given in
    test_gpu_cnn.test_cnn_adam_math_multi_epoch)."""
    from feddrift_amd.engine.fljob import TrainPlan
    from feddrift_amd.ops.mlp_torch import _apply_update
    world = vc.cnn_world(62, K=2, seed=4)
    eng = vc.cnn_engine(world)
    G, P, K, lr = 3, world["P"], world["K"], 0.03
    x, y = world["x"].to(DEV), world["y"].to(DEV)
    opt = eng.make_opt_state("adam", G, lr, 0.0)
    st = {k: torch.zeros(G, P, device=DEV) for k in ("m", "v", "vmax")}
    st["t"] = torch.zeros(G, dtype=torch.int32, device=DEV)
    lr_t = torch.full((G,), lr, device=DEV)
    cur = world["gp"].to(DEV)
    rows = torch.arange(G, device=DEV)
    for step, lens in enumerate(([1, 17, 33], [16, 5, 9])):
        plan = vc.cnn_plan(lens, seed=6 + step)
        plan = TrainPlan(plan.rows, plan.step_off, plan.step_len,
                         plan.sample_num)
        reps = torch.zeros(G, P, device=DEV)
        eng.train(cur.clone(), reps, plan, opt, x, y, K)
        torch.cuda.synchronize()
        w_ref = cur[rows % K].clone()
        _apply_update("adam", lr_t, 0.0, st, w_ref,
                      eng._ws["grad"][:G].clone())
        err = (reps - w_ref).abs().max().item()
        assert err < 1e-5, (step, err)
        assert torch.equal(opt["t"], st["t"])
        for k in ("m", "v", "vmax"):
            assert (opt[k] - st[k]).abs().max().item() < 1e-5, (step, k)
        cur = reps[:K].clone()


def test_cnn_grad_x_mask():
    """x_mask [G, 784]: conv1 wgrad reads the masked input a second time."""
    world = vc.cnn_world(10, K=2)
    plan = vc.cnn_plan([5, 16, 17, 20], seed=7)
    g = torch.Generator().manual_seed(8)
    xmask = (torch.rand(4, 784, generator=g) > 0.3).float()
    run = vc.cnn_sgd_epoch(vc.cnn_engine(world), world, plan, xmask)
    vc.check_cnn_grads("cnn grad x_mask", world, plan, run, xmask=xmask)


# --------------------------------------------------------------------------
# dropout: backward must recompute the mask the forward used
# --------------------------------------------------------------------------

def test_cnn_dropout_forward_backward_consistency():
    """Recover the forward keep-scales from the workspace, then run float64
    autograd with them as fixed multipliers: the gradients match only if
    cnn_pool_bwd / cnn_fc2_dgrad hash the ids cnn_pool_fwd / cnn_fc1_act
    hashed."""
    world = vc.cnn_world(10, K=2)
    lens = [8, 16, 20]
    plan = vc.cnn_plan(lens, seed=9)
    eng = vc.cnn_engine(world, dropout=True)       # p = 0.25 / 0.5 live
    p1, p2 = eng._dropout_ps()
    assert (p1, p2) == (0.25, 0.5)
    run = vc.cnn_sgd_epoch(eng, world, plan)
    scales, kept1, seen1, kept2, seen2 = [], 0, 0, 0, 0
    for g, n in enumerate(lens):
        a2, z1, a1 = run["a2"][g, :n], run["z1"][g, :n], run["a1"][g, :n]
        # a2 / pooled64 is 0 where dropped and 1/(1-p1) where kept: kept is
        # a2 != 0 (pooled64 is never 0), and check_cnn_grads below holds a2
        # to pooled64 * s1 within the pooled bound
        ka = a2 != 0
        # a1 / relu(z1) where z1 > 0, both from the workspace: one rounding
        pos = z1 > 0
        kb = (a1 != 0) & pos
        full = z1.double() / (1 - p2)
        assert ((a1.double() - full).abs() * kb
                <= 2.0 ** -23 * full.abs()).all(), g
        assert (a1[~pos] == 0).all(), g
        scales.append((ka.double() / (1 - p1), kb.double() / (1 - p2)))
        kept1 += int(ka.sum())
        seen1 += ka.numel()
        kept2 += int(kb.sum())
        seen2 += int(pos.sum())          # a draw shows only where z1 > 0
    # keep rate within 5 binomial standard deviations of 1 - p
    for kept, seen, p in ((kept1, seen1, p1), (kept2, seen2, p2)):
        assert abs(kept / seen - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / seen), \
            (kept, seen, p)
    vc.check_cnn_grads("cnn grad dropout", world, plan, run, scales=scales)


# --------------------------------------------------------------------------
# eval sweep
# --------------------------------------------------------------------------

def test_cnn_eval_blocks_and_row_runs():
    eng, world = vc.case_cnn_eval_dump()
    wins = vc.cnn_eval_inputs(world)
    tr, _, _, ln = wins
    order = torch.argsort(tr, stable=True)
    slot = torch.cumsum(ln[order], 0) - ln[order]
    _, _, blk_len = eng._fc1_blocks(tr[order], ln[order], slot)
    assert blk_len.tolist() == [63, 64, 64, 64, 2]
    # a chunk boundary inside a row run
    eng.EVAL_SLOT_BUDGET = 100
    vc.check_cnn_eval("cnn eval budget=100", world, eng, wins)


@pytest.mark.parametrize("form", ["1d", "per_window"])
def test_cnn_eval_x_mask(form):
    world = vc.cnn_world(10, K=3, seed=2)
    wins = vc.cnn_eval_inputs(world)
    g = torch.Generator().manual_seed(10)
    shape = (784,) if form == "1d" else (len(vc.EVAL_WINDOWS), 784)
    xmask = (torch.rand(*shape, generator=g) > 0.3).float()
    vc.check_cnn_eval(f"cnn eval mask {form}", world, vc.cnn_engine(world),
                      wins, xmask)


def test_cnn_eval_o62():
    vc.case_cnn_eval_dump(case="cnn eval O=62", O=62)


# --------------------------------------------------------------------------
# process-latched variants: one fresh child per variant
# --------------------------------------------------------------------------

VARIANTS = [
    ({"FEDDRIFT_CONV2FWD": "2"}, "cnn_grad_edges"),
    ({"FEDDRIFT_CONV2FWD": "2"}, "cnn_eval_dump"),
    ({"FEDDRIFT_DGRAD": "1"}, "cnn_grad_edges"),
    ({"FEDDRIFT_DGRAD": "2"}, "cnn_grad_edges"),
    ({"FEDDRIFT_TRAIN_BS64_MIN_G": "1000000"}, "small_train"),
    # tests/test_gpu_mlp_rounds.py, parts A and B, on the 256-thread build
    ({"FEDDRIFT_TRAIN_BS64_MIN_G": "1000000"}, "rounds_small_train"),
    ({"FEDDRIFT_TRAIN_BS64_MIN_G": "1000000"}, "rounds_small_fused"),
]
# import torch + the extension, a handful of launches, float64 references
CHILD_TIMEOUT_S = 240
_card_suspect = False


@pytest.mark.parametrize(
    "env,case", VARIANTS,
    ids=[f"{'-'.join(f'{k}={v}' for k, v in e.items())}-{c}"
         for e, c in VARIANTS])
def test_variant_in_child_process(env, case):
    global _card_suspect
    if _card_suspect:
        pytest.skip("an earlier variant child was killed or aborted")
    from feddrift_amd.ops import hip_loader
    hip_loader.load()                  # the child must find it built
    child_env = dict(os.environ)
    child_env.update(env)
    try:
        r = subprocess.run([sys.executable, vc.__file__, case],
                           env=child_env, timeout=CHILD_TIMEOUT_S,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _card_suspect = True
        pytest.fail(f"{env} {case}: child exceeded {CHILD_TIMEOUT_S}s")
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (134, 139):
        _card_suspect = True
    assert r.returncode == 0, (env, case, r.returncode, r.stdout[-2000:],
                               r.stderr[-4000:])
