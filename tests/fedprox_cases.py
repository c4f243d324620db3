"""Check bodies shared by tests/test_fedprox.py (CPU) and
tests/test_gpu_fedprox.py (HIP kernels), and the child process of the
256-thread small train kernel (not collected: no test_ prefix).

FedProx local training hands the optimizer grad + mu * (w - w0) at every
executed step; the specification is ops/mlp_torch.train_fused. Everything
here compares against float64 on the CPU. The bound is the project's rule
min(4 x err32, 5e-5), err32 being fp32 mlp_torch against float64 mlp_torch
on the same inputs WITH THE SAME mu (`measure_prox_err32()`, CPU only; table
in PARITY.md, "Proximal local training"). The helpers extend those of
tests/gpu_variant_cases.py by a `mu` argument: mu=None leaves the key out
of the optimizer state altogether.

`python tests/fedprox_cases.py CASE` runs one named case in a fresh process
(FEDDRIFT_TRAIN_BS64_MIN_G is latched once per process by the C++ dispatch).
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

import gpu_variant_cases as vc  # noqa: E402
from feddrift_amd.ops import mlp_torch  # noqa: E402

MU = 1.0                 # the GPU cases' coefficient
MUS = (0.0, 0.1, 1.0, 10.0)

# Largest err32 at mu = 1.0 over the small cases (seeds 100..104), the
# generic cases (vc.GENERIC_SEEDS) and the fused case (vc.FUSED_SEED), each
# with sgd and adam, with and without x_mask: measure_prox_err32().
PROX_TRAIN_ERR32 = {"param": 1.47e-6, "m": 1.21e-5, "v": 1.47e-6,
                    "vmax": 1.47e-6}
PROX_TRAIN_TOL = {k: min(4 * e, 5e-5) for k, e in PROX_TRAIN_ERR32.items()}
# a kernel that ignores mu must not pass: max|p64(mu) - p64(0)| is at least
# this many times the parameter bound in every case
EFFECT_FACTOR = 10


# --------------------------------------------------------------------------
# MLP training with mu
# --------------------------------------------------------------------------

def prox_opt(optname, R, P, dev, dtype, mu):
    opt = mlp_torch.make_opt_state(optname, R, P, vc.MLP_LR, vc.MLP_WD, dev,
                                   dtype=dtype)
    opt.pop("mu", None)
    if mu is not None:
        opt["mu"] = mu
    return opt


def mlp_train_ref(inp, optname, dtype, mu):
    """vc.mlp_train_ref with mu; inp["bcast"] = (glob, model_of) broadcasts
    the global rows first (they are then the anchor, as the rows at entry)."""
    spec = inp["spec"]
    p = inp["params"].to(dtype).clone()
    if inp.get("bcast") is not None:
        glob, model_of = inp["bcast"]
        p[inp["rows"]] = glob.to(dtype)[model_of]
    opt = prox_opt(optname, inp["R"], spec.n_params, "cpu", dtype, mu)
    mask = inp["mask"].to(dtype) if inp["mask"] is not None else None
    mlp_torch.train_fused(spec, p, inp["rows"], inp["x"].to(dtype), inp["y"],
                          inp["off"], inp["ln"], opt, x_mask=mask)
    return p, opt


def mlp_train_hip(inp, optname, mu, **fused):
    from feddrift_amd.ops import mlp_hip
    dev = vc._dev()
    spec = inp["spec"]
    p = inp["params"].clone().to(dev)
    opt = prox_opt(optname, inp["R"], spec.n_params, dev, torch.float32, mu)
    mask = inp["mask"].to(dev) if inp["mask"] is not None else None
    mlp_hip.train_fused(spec, p, inp["rows"].to(dev), inp["x"].to(dev),
                        inp["y"].to(dev), inp["off"].to(dev),
                        inp["ln"].to(dev), opt, x_mask=mask, **fused)
    torch.cuda.synchronize()
    return p.cpu(), {k: (v.cpu() if torch.is_tensor(v) else v)
                     for k, v in opt.items()}


def mlp_train_figures(inp, optname, mu, got=None):
    """{quantity: (err32, kernel error or None)} against float64 at mu, the
    float64 optimizer state and the float64 parameters."""
    p64, o64 = mlp_train_ref(inp, optname, torch.float64, mu)
    p32, o32 = mlp_train_ref(inp, optname, torch.float32, mu)
    qs = {"param": (p64, p32, got[0] if got else None)}
    if optname == "adam":
        for k in ("m", "v", "vmax"):
            qs[k] = (o64[k], o32[k], got[1][k] if got else None)
    figs = {}
    for k, (r64, r32, rk) in qs.items():
        e32 = (r32.double() - r64).abs().max().item()
        ke = (rk.double() - r64).abs().max().item() if rk is not None \
            else None
        figs[k] = (e32, ke)
    return figs, o64, p64


def effect(inp, optname, mu):
    """max|p64(mu) - p64(0)| over the trained rows."""
    a, _ = mlp_train_ref(inp, optname, torch.float64, mu)
    b, _ = mlp_train_ref(inp, optname, torch.float64, 0.0)
    return (a - b).abs().max().item()


def assert_same_bits(case, a, b):
    """Parameters and Adam state of two runs (params, opt) are equal."""
    assert torch.equal(a[0], b[0]), (case, "param")
    for k in ("m", "v", "vmax", "t"):
        if k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), (case, k)


def check_prox_train(case, inp, optname, mu=MU, **fused):
    """One launch at `mu` against float64 at the same mu, the effect guard,
    and mu = 0.0 against the call without the key (equal bits)."""
    got = mlp_train_hip(inp, optname, mu, **fused)
    figs, o64, _ = mlp_train_figures(inp, optname, mu, got)
    eff = effect(inp, optname, mu)
    for k, (e32, ke) in figs.items():
        vc.record(case, k, e32, ke, PROX_TRAIN_TOL[k])
    vc.record(case, "effect of mu", None, eff,
              EFFECT_FACTOR * PROX_TRAIN_TOL["param"])
    assert eff >= EFFECT_FACTOR * PROX_TRAIN_TOL["param"], (case, eff)
    rest = torch.ones(inp["R"], dtype=torch.bool)
    rest[inp["rows"]] = False
    assert torch.equal(got[0][rest], inp["params"][rest]), case
    if optname == "adam":
        # the zero-length step skips without advancing t, pull or no pull
        assert torch.equal(got[1]["t"], o64["t"]), (case, got[1]["t"])
    for k, (e32, ke) in figs.items():
        assert ke <= PROX_TRAIN_TOL[k], (case, k, ke, PROX_TRAIN_TOL[k])
    zero = mlp_train_hip(inp, optname, 0.0, **clone_fused(fused))
    absent = mlp_train_hip(inp, optname, None, **clone_fused(fused))
    assert_same_bits((case, "mu=0 vs no key"), zero, absent)
    return got


def clone_fused(fused):
    """A launch adds into `partial`: every launch gets its own copy."""
    return {k: (v.clone() if k == "partial" else v) for k, v in fused.items()}


def small_cases():
    for i, (kind, d, o) in enumerate(vc.SMALL_SHAPES):
        for optname in ("sgd", "adam"):
            for masked in (False, True):
                yield (f"prox small {kind}({d},{o}) {optname} "
                       f"mask={int(masked)}", kind, d, o, optname, masked,
                       100 + i)


def generic_cases():
    for i, (kind, d, o) in enumerate(vc.GENERIC_SHAPES):
        for optname in ("sgd", "adam"):
            yield (f"prox generic {kind}({d},{o}) {optname}", kind, d, o,
                   optname, vc.GENERIC_SEEDS[i])


def case_small_bs256():
    """fnn(3,2), sgd and adam, no mask and x_mask, on whatever block size
    the process was started for (the child sets FEDDRIFT_TRAIN_BS64_MIN_G
    huge: 256-thread blocks)."""
    for case, kind, d, o, optname, masked, seed in small_cases():
        if (kind, d, o) != ("fnn", 3, 2):
            continue
        inp = vc.mlp_train_inputs(kind, d, o, vc.SMALL_LENS, masked, seed)
        check_prox_train(case + " bs256", inp, optname)


FUSED_K = 5
FUSED_MODEL_OF = (0, 1, 2, 3, 0, 1, 2, 0, 3)      # model 4: no pair


def fused_inputs():
    """The set-up of test_gpu_mlp_edges.py::test_fused_broadcast_and_partial:
    K = 5, G = 9, replica rows pre-set to 0, two sample_w = 0, model 4
    without a pair. inp["params"] holds the zeroed rows the launch gets;
    inp["bcast"] tells the reference to broadcast first."""
    inp = vc.mlp_train_inputs("fnn", 12, 4, vc.GENERIC_LENS, False,
                              seed=vc.FUSED_SEED, G=9)
    P = inp["spec"].n_params
    g = torch.Generator().manual_seed(301)
    glob = torch.randn(FUSED_K, P, generator=g) * 0.4
    model_of = torch.tensor(FUSED_MODEL_OF)
    sample_w = torch.rand(9, generator=g) + 0.5
    sample_w[[1, 4]] = 0.0
    start = inp["params"].clone()
    start[inp["rows"]] = 0.0
    return dict(inp, params=start, bcast=(glob, model_of), glob=glob,
                model_of=model_of, sample_w=sample_w)


def measure_prox_err32(mus=(0.1, 1.0)):
    """err32 per mu: {mu: {quantity: largest err32}} over every small and
    generic case and the fused case. CPU only."""
    out = {}
    for mu in mus:
        worst = {"param": 0.0, "m": 0.0, "v": 0.0, "vmax": 0.0}

        def fold(name, inp, optname):
            for k, (e32, _) in mlp_train_figures(inp, optname, mu)[0].items():
                print(f"mu={mu} {name} {k} err32={e32:.3e}")
                worst[k] = max(worst[k], e32)
        for case, kind, d, o, optname, masked, seed in small_cases():
            fold(case, vc.mlp_train_inputs(kind, d, o, vc.SMALL_LENS, masked,
                                           seed), optname)
        for i, (kind, d, o) in enumerate(vc.GENERIC_SHAPES):
            for optname in ("sgd", "adam"):
                for masked in (False, True):
                    fold(f"prox generic {kind}({d},{o}) {optname} "
                         f"mask={int(masked)}",
                         vc.mlp_train_inputs(kind, d, o, vc.GENERIC_LENS,
                                             masked, vc.GENERIC_SEEDS[i]),
                         optname)
        fold("prox fused fnn(12,4) adam", fused_inputs(), "adam")
        out[mu] = worst
    return out


# --------------------------------------------------------------------------
# FLJob rounds with mu, each held to the float64 replay of the specification
# --------------------------------------------------------------------------

def plan_windows(plan):
    # the template's scratch arrays are overwritten by the next draw
    return dict(rows=torch.from_numpy(np.array(plan.rows, copy=True)),
                off=torch.from_numpy(np.array(plan.step_off, copy=True)),
                ln=torch.from_numpy(np.array(plan.step_len, copy=True)))


def prox_round(job, case, r, ci, clip_bound=0.0):
    """Plan and train round r of an MLP job; the trained replicas and the
    carried optimizer state against the float64 replay `broadcast the
    pre-round global rows, train_fused with the job's mu (then clip to
    clip_bound)`, under vc.ROUND_TRAIN_TOL. Returns (plan, float64 replica
    table, worst figures)."""
    from feddrift_amd.comm import robust as rb
    from secagg_cases import torch_sync
    spec, K = job.spec, job.n_models
    x64, y = job.arena.x.cpu().double(), job.arena.y.cpu()
    plan = job.algo.plan(job, r, ci)
    L = plan_windows(plan)
    rows = L["rows"]
    assert len(rows)
    glob0 = job.global_params.detach().cpu().clone()
    o64 = vc.opt_to(job.opt, "cpu", torch.float64)
    assert o64["mu"] == job.cfg.fedprox_mu
    # what the float64 replay gives without the pull: figs["effect"]
    o64_0 = dict(vc.opt_to(job.opt, "cpu", torch.float64), mu=0.0)
    p64_0 = torch.zeros(job.replicas.shape, dtype=torch.float64)
    p64_0[rows] = glob0.double()[rows % K]
    vc.launch(mlp_torch, spec, p64_0, o64_0, x64, y, L)
    job.train(plan)
    torch_sync(job)
    after = vc.snapshot(job.replicas, job.opt)
    p64 = torch.zeros(job.replicas.shape, dtype=torch.float64)
    p64[rows] = glob0.double()[rows % K]
    vc.launch(mlp_torch, spec, p64, o64, x64, y, L)
    if clip_bound > 0:
        rb.clip_and_accumulate(p64, rows.numpy(), (rows % K).numpy(),
                               np.ones(len(rows)), glob0.double(),
                               clip_bound)
    s64 = vc.snapshot(p64, o64)
    figs = {}
    eff = (p64[rows] - p64_0[rows]).abs().max().item() \
        if clip_bound <= 0 else None
    for q in vc.ROUND_QS:
        if q in s64:
            figs[q] = (after[q][rows].double() - s64[q][rows]).abs().max() \
                .item()
            vc.record(f"{case} r{r}", q, None, figs[q], vc.ROUND_TRAIN_TOL[q])
    for q, ke in figs.items():
        assert ke <= vc.ROUND_TRAIN_TOL[q], (case, r, q, ke)
    if "t" in s64:
        assert torch.equal(after["t"], s64["t"]), (case, r)
    if eff is not None:
        figs["effect"] = eff
        vc.record(f"{case} r{r}", "effect of mu", None, eff,
                  EFFECT_FACTOR * vc.ROUND_TRAIN_TOL["param"])
    return plan, p64, figs


# --------------------------------------------------------------------------
# module models: the eager float64 oracle of one round of local training
# --------------------------------------------------------------------------

def eager_prox_round(make_module, packer, glob, plan, x, y, K, optname, lr,
                     wd, mu, dtype=torch.float64, x_mask=None):
    """Per pair: load the global row, minimise CE + mu/2 |p - p0|^2 over the
    TRAINABLE parameters by autograd with torch.optim, one step per
    non-empty window. Fresh optimizer per pair (a round from a zero state).
    Returns the replica rows [G, P] (buffers included)."""
    out = torch.zeros(len(plan.rows), packer.n_params, dtype=dtype)
    for gi, row in enumerate(plan.rows):
        mod = make_module().to(dtype)
        packer.load_into(mod, glob[int(row) % K].to(dtype))
        mod.train()
        params = [p for p in mod.parameters()]
        p0 = [p.detach().clone() for p in params]
        if optname == "adam":
            opt = torch.optim.Adam(params, lr=lr, weight_decay=wd,
                                   amsgrad=True)
        else:
            opt = torch.optim.SGD(params, lr=lr)
        for e in range(plan.step_off.shape[1]):
            n, off = int(plan.step_len[gi, e]), int(plan.step_off[gi, e])
            if n == 0:
                continue
            xs = x[off:off + n].to(dtype)
            if x_mask is not None:
                xs = xs * x_mask[gi].to(dtype)
            opt.zero_grad()
            loss = F.cross_entropy(mod(xs), y[off:off + n])
            loss = loss + 0.5 * mu * sum(((p - q) ** 2).sum()
                                         for p, q in zip(params, p0))
            loss.backward()
            opt.step()
        sd = mod.state_dict()       # (packer.dump_from rounds to fp32)
        out[gi] = torch.cat([sd[k].reshape(-1).to(dtype)
                             for k in packer.keys])
    return out


CASES = {"small_bs256": case_small_bs256}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print(f"usage: {argv[0]} {{{'|'.join(CASES)}}}")
        return 2
    CASES[argv[1]]()
    print(f"case {argv[1]} OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
