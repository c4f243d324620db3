"""Check bodies shared by tests/test_gpu_mlp_edges.py, tests/test_gpu_cnn_edges.py,
tests/test_gpu_mlp_rounds.py with its CPU twin tests/test_round_seams.py,
and the per-variant child processes (not collected: no test_ prefix).

Every comparison here is against float64 on the CPU. The bounds are the
named constants below; each derives from `err32`, the error of an honest
fp32 torch implementation against the same float64 value on the same
inputs (table: PARITY.md, "Kernel edge and variant coverage"), by the
margins stated next to it. err32 needs no GPU: `measure_mlp_train_err32()`
prints the MLP train column, and every check prints its own err32 (or the
constant it uses), the kernel's error and the bound as a `FIG` line
before it asserts (`pytest -s`).

Some kernel variants are selected by environment variables that the C++
dispatch latches once per process (FEDDRIFT_CONV2FWD, FEDDRIFT_DGRAD,
FEDDRIFT_TRAIN_BS64_MIN_G), so `python tests/gpu_variant_cases.py CASE`
runs one named case in a fresh process and exits non-zero when it fails.
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__),
                                                "..")))

from feddrift_amd.models.packed import spec_for  # noqa: E402
from feddrift_amd.ops import mlp_torch  # noqa: E402

# --------------------------------------------------------------------------
# bounds (PARITY.md, "Kernel edge and variant coverage")
# --------------------------------------------------------------------------

# MLP parameters / Adam state after E steps: 4 x the largest err32 over the
# train cases, capped at the 5e-5 absolute of tests/test_gpu_ops.py.
MLP_TRAIN_ERR32 = {"param": 2.36e-6, "m": 1.32e-5, "v": 1.53e-6,
                   "vmax": 1.53e-6}
MLP_TRAIN_TOL = {k: min(4 * e, 5e-5) for k, e in MLP_TRAIN_ERR32.items()}

# CNN per-layer gradient, metric max|g - g64| / max|g64|: 4 x the largest
# err32 of that layer over the gradient cases (state_dict order: conv1 w/b,
# conv2 w/b, fc1 w/b, fc2 w/b).
CNN_GRAD_ERR32 = [2.14e-6, 2.86e-6, 9.42e-7, 9.33e-7,
                  5.79e-7, 3.43e-7, 5.98e-7, 2.85e-7]
CNN_GRAD_TOL = [4 * e for e in CNN_GRAD_ERR32]

# CNN per-sample outputs: 8 x the largest per-sample err32 (the kernels use
# __expf where torch uses an accurate exp); sums scale by the sample count.
CNN_PROB_ERR32 = 7.97e-8
CNN_LOSS_ERR32 = 4.89e-7
CNN_MSE_ERR32 = 9.53e-8
CNN_PROB_TOL = 8 * CNN_PROB_ERR32
CNN_LOSS_TOL = 8 * CNN_LOSS_ERR32
CNN_MSE_TOL = 8 * CNN_MSE_ERR32
# pooled activations (conv1 -> conv2 -> max-pool): 4 x err32, absolute
CNN_POOL_ERR32 = 4.07e-7
CNN_POOL_TOL = 4 * CNN_POOL_ERR32
# two pool inputs that are each within CNN_POOL_TOL of float64 can swap
# order when they are closer than this: such windows are tied
POOL_TIE = 2 * CNN_POOL_TOL
POOL_TIE_MAX_SHARE = 1e-4    # measured 2.4e-5 of all windows

NEAR_TIE_MLP = 1e-4      # top-two gap of float64 logits
NEAR_TIE_CNN = 1e-5      # top-two gap of float64 probabilities
NEAR_TIE_MAX_SHARE = 0.02

FIGURES = []             # (case, quantity, err32 or None, kernel error, bound)


def record(case, qty, err32, kerr, bound):
    FIGURES.append((case, qty, err32, kerr, bound))
    e32 = "-" if err32 is None else f"{err32:.3e}"
    k = "-" if kerr is None else f"{kerr:.3e}"
    b = "-" if bound is None else f"{bound:.3e}"
    print(f"FIG {case} | {qty} | err32={e32} | kernel={k} | bound={b}",
          flush=True)


def _dev():
    return torch.device("cuda:0")


# --------------------------------------------------------------------------
# MLP training
# --------------------------------------------------------------------------

MLP_N = 4000
SMALL_SHAPES = [("fnn", 3, 2), ("fnn", 2, 2), ("fnn", 4, 2),
                ("lr", 3, 2), ("lr", 2, 2)]
SMALL_LENS = (1, 63, 64, 65, 200)          # one-wave stride edges
GENERIC_SHAPES = [("fnn", 12, 4), ("fnn", 8, 5), ("lr", 4, 2)]
GENERIC_LENS = (1, 511, 512, 513, 1100)    # 1, 2 and 3 trips of the BC loop
# Input seeds per generic shape (and for the fused case). Adam's step
# g / (sqrt(vmax) + eps) is ill-conditioned where a length-1 step meets a
# saturated softmax (|g| ~ eps = 1e-8): on such draws fp32 torch itself is
# off by up to lr / 2 from float64 (err32 5e-3, seen at 1 seed in 6), and no
# fp32 implementation can be told right from wrong. These seeds are draws
# that fp32 torch resolves (err32 <= 1e-5); nothing else selects them.
GENERIC_SEEDS = (102, 109, 100)
FUSED_SEED = 307
MLP_LR, MLP_WD = 0.01, 1e-3


def mlp_arena(d, o, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(MLP_N, d, generator=g) * 10
    y = torch.randint(0, o, (MLP_N,), generator=g)
    return x, y, g


def mlp_train_inputs(kind, d, o, lens, masked, seed, G=6, E=4):
    """rows is a permutation subset of a larger replica table; every length
    of `lens` occurs, one step has length 0."""
    spec = spec_for(kind, d, o)
    x, y, g = mlp_arena(d, o, seed)
    R = G + 3
    params = torch.randn(R, spec.n_params, generator=g) * 0.4
    rows = torch.randperm(R, generator=g)[:G]
    choice = torch.tensor(lens)
    ln = choice[torch.randint(0, len(lens), (G, E), generator=g)]
    zero_at = 2 * E + 1
    perm = torch.randperm(G * E, generator=g)
    ln.view(-1)[perm[perm != zero_at][:len(lens)]] = choice
    ln.view(-1)[zero_at] = 0
    off = (torch.rand(G, E, generator=g) * (MLP_N - max(lens))).long()
    mask = ((torch.rand(G, d, generator=g) > 0.4).float()
            if masked else None)
    return dict(spec=spec, x=x, y=y, params=params, rows=rows, off=off,
                ln=ln, mask=mask, R=R)


def mlp_train_ref(inp, optname, dtype):
    spec = inp["spec"]
    p = inp["params"].to(dtype).clone()
    opt = mlp_torch.make_opt_state(optname, inp["R"], spec.n_params, MLP_LR,
                                   MLP_WD, "cpu", dtype=dtype)
    mask = inp["mask"].to(dtype) if inp["mask"] is not None else None
    mlp_torch.train_fused(spec, p, inp["rows"], inp["x"].to(dtype), inp["y"],
                          inp["off"], inp["ln"], opt, x_mask=mask)
    return p, opt


def mlp_train_hip(inp, optname, **fused):
    from feddrift_amd.ops import mlp_hip
    dev = _dev()
    spec = inp["spec"]
    p = inp["params"].clone().to(dev)
    opt = mlp_torch.make_opt_state(optname, inp["R"], spec.n_params, MLP_LR,
                                   MLP_WD, dev)
    mask = inp["mask"].to(dev) if inp["mask"] is not None else None
    mlp_hip.train_fused(spec, p, inp["rows"].to(dev), inp["x"].to(dev),
                        inp["y"].to(dev), inp["off"].to(dev),
                        inp["ln"].to(dev), opt, x_mask=mask, **fused)
    torch.cuda.synchronize()
    return p.cpu(), {k: (v.cpu() if torch.is_tensor(v) else v)
                     for k, v in opt.items()}


def mlp_train_figures(inp, optname, got=None):
    """{quantity: (err32, kernel error or None)} against float64."""
    p64, o64 = mlp_train_ref(inp, optname, torch.float64)
    p32, o32 = mlp_train_ref(inp, optname, torch.float32)
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
    return figs, o64


def check_mlp_train(case, inp, optname):
    got = mlp_train_hip(inp, optname)
    figs, o64 = mlp_train_figures(inp, optname, got)
    for k, (e32, ke) in figs.items():
        record(case, k, e32, ke, MLP_TRAIN_TOL[k])
    # rows outside `rows` are not touched at all
    rest = torch.ones(inp["R"], dtype=torch.bool)
    rest[inp["rows"]] = False
    assert torch.equal(got[0][rest], inp["params"][rest]), case
    if optname == "adam":
        # the zero-length step skips without advancing t
        assert torch.equal(got[1]["t"], o64["t"]), (case, got[1]["t"])
        assert int(o64["t"][inp["rows"][2]]) == inp["ln"].shape[1] - 1
    for k, (e32, ke) in figs.items():
        assert ke <= MLP_TRAIN_TOL[k], (case, k, ke, MLP_TRAIN_TOL[k])


def case_small_train():
    """The register-resident small train kernel, all five template shapes,
    {sgd, adam} x {no mask, x_mask}."""
    for i, (kind, d, o) in enumerate(SMALL_SHAPES):
        for optname in ("sgd", "adam"):
            for masked in (False, True):
                inp = mlp_train_inputs(kind, d, o, SMALL_LENS, masked,
                                       seed=100 + i)
                check_mlp_train(f"small {kind}({d},{o}) {optname} "
                                f"mask={int(masked)}", inp, optname)


# --------------------------------------------------------------------------
# the MLP round path across launches (PARITY.md, "Round path across
# launches"): carried optimizer state, fused broadcast / partial / apply
# chains, FLJob rounds. Every check takes the op module under test, so the
# same body runs with fp32 mlp_torch on the CPU (tests/test_round_seams.py),
# where the "kernel" error is err32 itself.
# --------------------------------------------------------------------------

# 4 x the largest err32 over the new train cases (parts A and B, every
# launch; measure_round_err32()), capped at 5e-5
ROUND_TRAIN_ERR32 = {"param": 3.38e-6, "m": 2.22e-5, "v": 3.24e-6,
                     "vmax": 3.24e-6}
ROUND_TRAIN_TOL = {k: min(4 * e, 5e-5) for k, e in ROUND_TRAIN_ERR32.items()}

ROUND_R, ROUND_G, ROUND_E = 9, 6, 4
ROUND_T0 = (0, 1, 7, 999, 1000, 20000, 3, 50, 123456)
# Shape i of its list takes seed 500 + i % 3. fnn(12,4) is the exception:
# on its seed 500 fp32 torch itself is 1.4e-5 off float64 on `param` and
# 1.8e-4 on `m` (a hidden unit within rounding of the ReLU kink, where the
# gradient jumps), above the 1e-5 at which a draw counts as ill-conditioned
# (see GENERIC_SEEDS), and 503 (1.1e-5) is too; 504 is the next seed.
# Nothing else selects seeds.
ROUND_SMALL_SEEDS = (500, 501, 502, 500, 501)
ROUND_GENERIC_SEEDS = (504, 501, 502)
ROUND_QS = ("param", "m", "v", "vmax")
U24 = 2.0 ** -24


def seeded_opt_state(optname, R, P, g):
    """Optimizer state as a job carries it into a launch: a rate of its own
    per row, first and second moments away from zero, vmax on both sides of
    v (both branches of the amsgrad max), step counts from 0 to 123456."""
    r9 = torch.arange(R) % len(ROUND_T0)
    opt = {"kind": optname, "wd": MLP_WD,
           "lr": 0.002 + 0.002 * r9.float()}
    if optname == "adam":
        opt["m"] = 0.05 * torch.randn(R, P, generator=g)
        opt["v"] = 0.01 * torch.rand(R, P, generator=g)
        opt["vmax"] = opt["v"] * (0.5 + torch.rand(R, P, generator=g))
        opt["t"] = torch.tensor(ROUND_T0, dtype=torch.int32)[r9]
    return opt


def opt_to(opt, dev, dtype):
    out = {}
    for k, v in opt.items():
        if not torch.is_tensor(v):
            out[k] = v
        elif v.is_floating_point():
            out[k] = v.to(dev, dtype).clone()
        else:
            out[k] = v.to(dev).clone()
    return out


def snapshot(params, opt):
    s = {k: v.detach().cpu().clone() for k, v in opt.items()
         if torch.is_tensor(v)}
    s["param"] = params.detach().cpu().clone()
    return s


def draw_windows(g, G, E, lens, dead=None):
    """[G, E] window starts and lengths: every length of `lens` occurs, one
    step has length 0, and so has every step of pair `dead` (if given)."""
    choice = torch.tensor(lens)
    ln = choice[torch.randint(0, len(lens), (G, E), generator=g)]
    zero = torch.zeros(G * E, dtype=torch.bool)
    zero[2 * E + 1] = True
    if dead is not None:
        zero[dead * E:(dead + 1) * E] = True
    perm = torch.randperm(G * E, generator=g)
    ln.view(-1)[perm[~zero[perm]][:len(lens)]] = choice
    ln.view(-1)[zero] = 0
    off = (torch.rand(G, E, generator=g) * (MLP_N - max(lens))).long()
    return off, ln


def launch(ops, spec, params, opt, x, y, L, **fused):
    """One train_fused call of op module `ops` on the tensors' device."""
    dev = params.device
    mask = L.get("mask")
    ops.train_fused(spec, params, L["rows"].to(dev), x, y, L["off"].to(dev),
                    L["ln"].to(dev), opt,
                    x_mask=None if mask is None
                    else mask.to(dev, params.dtype), **fused)
    if dev.type == "cuda":
        torch.cuda.synchronize()


def worst_figures(figs, s64, s32=None, sk=None):
    """Fold one launch's errors against float64 into figs[q] = [err32,
    kernel error]."""
    for q in ROUND_QS:
        if q not in s64:
            continue
        f = figs.setdefault(q, [0.0, 0.0])
        for i, s in enumerate((s32, sk)):
            if s is not None:
                f[i] = max(f[i], (s[q].double() - s64[q]).abs().max().item())


# A hidden pre-activation z1 within RELU_TIE of 0 is tied: the ReLU's
# derivative jumps there, so the whole gradient of that (sample, unit) has
# two right answers, and which one an fp32 implementation takes hangs on
# its last bits. Weights that are err32 (3.4e-6) off float64 move z1 by
# err32 * (1 + sum |x_d|), 5e-5 at the 3 or 4 features of x ~ U(0, 10)
# where the broadcast chains run; the fp32 rounding of the dot product
# itself (1e-6) is well inside that.
RELU_TIE = 5e-5
RELU_TIE_MAX_FORKS = 4


def _pair_run(spec, x64, y, off, ln, mask, p0, o0, force, near):
    """float64 train_fused of ONE pair from weights p0 [P] and its one-row
    optimizer state o0. `force` {(call, sample, unit): sign} fixes the ReLU
    decision of tied pre-activations; `near` collects the tied
    (call, sample, unit) of this run."""
    calls = [0]

    def fwd(spec_, params, x):
        G = params.shape[0]
        w1 = params[:, spec_.off_w1:spec_.off_b1].reshape(G, spec_.h, spec_.d)
        b1 = params[:, spec_.off_b1:spec_.off_w2].reshape(G, 1, spec_.h)
        w2 = params[:, spec_.off_w2:spec_.off_b2].reshape(G, spec_.o, spec_.h)
        b2 = params[:, spec_.off_b2:].reshape(G, 1, spec_.o)
        z1 = torch.baddbmm(b1, x, w1.transpose(1, 2))
        c = calls[0]
        calls[0] += 1
        for i, h in (z1[0].abs() < RELU_TIE).nonzero().tolist():
            near.append((c, i, h))
        for (cc, i, h), sign in force.items():
            if cc == c:
                z1[0, i, h] = sign * 1e-300
        a = torch.relu(z1)
        return z1, a, torch.baddbmm(b2, a, w2.transpose(1, 2))

    p = p0.clone()[None]
    opt = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o0.items()}
    orig = mlp_torch._forward_fnn
    mlp_torch._forward_fnn = fwd
    try:
        mlp_torch.train_fused(spec, p, torch.zeros(1, dtype=torch.long), x64,
                              y, off[None], ln[None], opt,
                              x_mask=None if mask is None else mask[None])
    finally:
        mlp_torch._forward_fnn = orig
    return snapshot(p, opt)


def adopt_relu_ties(case, spec, x64, y, L, start64, before64, s64, sk):
    """Where a pair of the launch is outside ROUND_TRAIN_TOL of the float64
    reference s64, and only there: if that reference passed tied
    pre-activations, rerun the pair in float64 with their ReLU decisions
    forced every way, and let s64 adopt a rerun that the implementation is
    within the bounds of. A pair without tied pre-activations, or that
    matches no rerun, stays as it is and fails its caller's bounds.
    Returns the adopted pairs."""
    import itertools
    if spec.kind != "fnn":
        return []
    rows = L["rows"]
    qs = [q for q in ROUND_QS if q in s64]
    out = torch.zeros(len(rows), dtype=torch.bool)
    for q in qs:
        out |= (sk[q][rows].double() - s64[q][rows]).abs().amax(1) \
            > ROUND_TRAIN_TOL[q]
    adopted = []
    for g in out.nonzero().flatten().tolist():
        row = int(rows[g])
        o0 = {k: (v[row:row + 1].double() if v.is_floating_point()
                  else v[row:row + 1]) for k, v in before64.items()
              if k != "param"}
        o0.update(kind="adam" if "m" in o0 else "sgd", wd=MLP_WD)
        mask = None if L.get("mask") is None else L["mask"][g].double()
        args = (spec, x64, y, L["off"][g], L["ln"][g], mask, start64[row], o0)
        near = []
        _pair_run(*args, {}, near)
        print(f"TIE {case} pair {g}: {len(near)} pre-activations within "
              f"{RELU_TIE:g} of the ReLU kink", flush=True)
        if not 0 < len(near) <= RELU_TIE_MAX_FORKS:
            continue
        for signs in itertools.product((1.0, -1.0), repeat=len(near)):
            alt = _pair_run(*args, dict(zip(near, signs)), [])
            if all((sk[q][row].double() - alt[q][0]).abs().max().item()
                   <= ROUND_TRAIN_TOL[q] for q in qs):
                for q in qs:
                    s64[q][row] = alt[q][0]
                adopted.append(g)
                break
    return adopted


def record_and_assert_train(case, figs):
    for q, (e32, ke) in figs.items():
        record(case, q, e32, ke, ROUND_TRAIN_TOL[q])
    for q, (e32, ke) in figs.items():
        assert ke <= ROUND_TRAIN_TOL[q], (case, q, ke, ROUND_TRAIN_TOL[q])


def assert_rows_identical(case, before, after, sel):
    for q in before:
        assert torch.equal(after[q][sel], before[q][sel]), (case, q)


# -- A: carried optimizer state over three launches ------------------------

def carried_inputs(kind, d, o, lens, seed):
    """R = 9 rows, three launches of a permuted 6-of-9 subset each: two rows
    train in every launch, one in none, four of the other six per launch.
    The second launch has a pair whose steps all have length 0."""
    spec = spec_for(kind, d, o)
    x, y, g = mlp_arena(d, o, seed)
    R, G, E = ROUND_R, ROUND_G, ROUND_E
    params = torch.randn(R, spec.n_params, generator=g) * 0.4
    state = seeded_opt_state("adam", R, spec.n_params, g)
    order = torch.randperm(R, generator=g)
    always, rest, never = order[:2], order[2:8], order[8:]
    launches = []
    for j in range(3):
        pick = rest[torch.randperm(6, generator=g)[:4]]
        rows = torch.cat([always, pick])[torch.randperm(G, generator=g)]
        dead = 4 if j == 1 else None
        off, ln = draw_windows(g, G, E, lens, dead)
        launches.append(dict(rows=rows, off=off, ln=ln, dead=dead))
    return dict(spec=spec, x=x, y=y, params=params, state=state, R=R,
                launches=launches, never=never)


def carried_opt(inp, optname):
    if optname == "adam":
        return inp["state"]
    return {"kind": "sgd", "wd": MLP_WD, "lr": inp["state"]["lr"]}


def carried_run(inp, optname, ops, dev, dtype):
    """The launches on ONE params / opt pair -> snapshot before the first
    and after each."""
    params = inp["params"].to(dev, dtype).clone()
    opt = opt_to(carried_opt(inp, optname), dev, dtype)
    x, y = inp["x"].to(dev, dtype), inp["y"].to(dev)
    snaps = [snapshot(params, opt)]
    for L in inp["launches"]:
        launch(ops, inp["spec"], params, opt, x, y, L)
        snaps.append(snapshot(params, opt))
    return snaps


def check_carried(case, inp, optname, ops, dev):
    s64 = carried_run(inp, optname, mlp_torch, "cpu", torch.float64)
    s32 = carried_run(inp, optname, mlp_torch, "cpu", torch.float32)
    sk = carried_run(inp, optname, ops, dev, torch.float32)
    figs = {}
    for j in range(1, len(sk)):
        worst_figures(figs, s64[j], s32[j], sk[j])
    for q, (e32, ke) in figs.items():
        record(case, q, e32, ke, ROUND_TRAIN_TOL[q])
    trained = torch.zeros(inp["R"], dtype=torch.bool)
    for j, L in enumerate(inp["launches"]):
        rest = torch.ones(inp["R"], dtype=torch.bool)
        rest[L["rows"]] = False
        trained[L["rows"]] = True
        assert int(rest.sum()) == inp["R"] - ROUND_G
        # rows that sit this launch out keep every bit
        assert_rows_identical((case, j, "rest"), sk[j], sk[j + 1], rest)
        if optname == "adam":
            assert torch.equal(sk[j + 1]["t"], s64[j + 1]["t"]), \
                (case, j, sk[j + 1]["t"], s64[j + 1]["t"])
        if L["dead"] is not None:
            assert int(L["ln"][L["dead"]].sum()) == 0
            row = L["rows"][L["dead"]:L["dead"] + 1]
            assert_rows_identical((case, j, "dead"), sk[j], sk[j + 1], row)
    assert int((~trained).sum()) >= 1 and not trained[inp["never"]].any()
    assert_rows_identical((case, "never"), sk[0], sk[-1], ~trained)
    if optname == "adam":
        # the steps counted are the non-empty ones, from each row's own t
        steps = torch.zeros(inp["R"], dtype=torch.int32)
        for L in inp["launches"]:
            steps[L["rows"]] += (L["ln"] > 0).sum(1).to(torch.int32)
        assert torch.equal(sk[-1]["t"], sk[0]["t"] + steps), case
    for q, (e32, ke) in figs.items():
        assert ke <= ROUND_TRAIN_TOL[q], (case, q, ke, ROUND_TRAIN_TOL[q])
    return figs


def carried_cases(small):
    shapes, lens, seeds = (SMALL_SHAPES, SMALL_LENS, ROUND_SMALL_SEEDS) \
        if small else (GENERIC_SHAPES, GENERIC_LENS, ROUND_GENERIC_SEEDS)
    for i, (kind, d, o) in enumerate(shapes):
        for optname in ("sgd", "adam"):
            yield (f"carried {kind}({d},{o}) {optname}", kind, d, o, lens,
                   seeds[i], optname)


def case_rounds_small_train(ops=None, dev=None):
    """Part A on the register-resident small train kernel."""
    if ops is None:
        from feddrift_amd.ops import mlp_hip as ops
        dev = _dev()
    for case, kind, d, o, lens, seed, optname in carried_cases(small=True):
        check_carried(case, carried_inputs(kind, d, o, lens, seed), optname,
                      ops, dev)


# -- B: fused broadcast + partial, apply, the next launch ------------------

FUSED_K, FUSED_G, FUSED_DEAD = 4, 300, 7     # model 3 has no pair
FUSED_TERMS = FUSED_G // 3 + 1               # 100 pairs per row + the start


def fused_inputs(kind, d, o, masked, seed):
    spec = spec_for(kind, d, o)
    x, y, g = mlp_arena(d, o, seed)
    G, E, K, P = FUSED_G, ROUND_E, FUSED_K, spec.n_params
    R = G + 3
    glob = torch.randn(K, P, generator=g) * 0.4
    rows = torch.randperm(R, generator=g)[:G]
    params = torch.randn(R, P, generator=g) * 0.4
    params[rows] = 0.0             # the launch stages from the global bank
    model_of = (torch.arange(G) % 3)[torch.randperm(G, generator=g)]
    sw = torch.randint(0, 501, (G,), generator=g).float()
    zeros = torch.randperm(G, generator=g)[:5]
    sw[zeros] = 0.0
    sw[FUSED_DEAD] = 250.0         # the all-empty pair still contributes
    wild = int(zeros[zeros != FUSED_DEAD][0])
    mask = (torch.rand(G, d, generator=g) > 0.4).float() if masked else None
    launches = []
    for j in range(2):
        dead = FUSED_DEAD if j == 0 else None
        off, ln = draw_windows(g, G, E, SMALL_LENS, dead)
        launches.append(dict(rows=rows, off=off, ln=ln, mask=mask,
                             dead=dead))
    state = seeded_opt_state("adam", R, P, g)
    # the one thing the sw > 0 guard of the fused partial can show: a pair of
    # weight 0 whose replica is not finite (its rate is inf) adds nothing,
    # where 0 * replica would be NaN
    state["lr"][rows[wild]] = float("inf")
    prefill = 0.25 * torch.arange(1, K + 1).float()[:, None] \
        + 0.001 * torch.arange(P + 1).float()[None, :]
    prefill[:, P] = 7.0 * torch.arange(1, K + 1).float()
    return dict(spec=spec, x=x, y=y, glob=glob, rows=rows, params=params,
                model_of=model_of, sw=sw, launches=launches, state=state,
                wild=wild,
                prefill=prefill, R=R, K=K, P=P)


def fused_launch(ops, inp, params, opt, x, y, L, glob, partial):
    """Broadcast from glob, train, add sw * replica into partial."""
    dev = params.device
    mo, sw = inp["model_of"].to(dev), inp["sw"].to(dev)
    if ops is mlp_torch:
        # what the kernel fuses, spelled out in fp32 torch
        rows = L["rows"].to(dev)
        params[rows] = glob[mo]
        launch(ops, inp["spec"], params, opt, x, y, L)
        keep = sw > 0
        partial.index_add_(
            0, mo[keep], torch.cat([sw[keep, None] * params[rows][keep],
                                    sw[keep, None]], 1))
        return
    launch(ops, inp["spec"], params, opt, x, y, L, in_params=glob,
           model_of=mo.to(torch.int32), sample_w=sw, partial=partial)


def apply_aggregate(ops, glob, partial, mask):
    """-> totals; drains partial."""
    if ops is mlp_torch:
        P = glob.shape[1]
        totals = partial[:, P].clone()
        upd = totals > 0
        if mask is not None:
            upd &= mask.bool()
        glob[upd] = partial[upd, :P] * (1.0 / totals[upd, None])
        partial.zero_()
        return totals
    totals = ops.apply_aggregate(glob, partial, mask)
    torch.cuda.synchronize()
    return totals


def fused_train_ref(inp, L, glob, opt, dtype):
    """Broadcast the given global bank, train on the CPU in `dtype`; opt is
    carried in place."""
    p = inp["params"].to(dtype).clone()
    p[L["rows"]] = glob.to(dtype)[inp["model_of"]]
    launch(mlp_torch, inp["spec"], p, opt, inp["x"].to(dtype), inp["y"], L)
    return snapshot(p, opt)


def weighted_sums(inp, reps):
    """float64 sum and sum of magnitudes of sw * replica per model, with the
    weight slot: [K, P + 1] each."""
    sw = inp["sw"].double()[:, None]
    terms = torch.cat([torch.where(sw > 0, sw * reps.double(), 0.0), sw], 1)
    K, P = inp["K"], inp["P"]
    s = torch.zeros(K, P + 1, dtype=torch.float64)
    mag = torch.zeros(K, P + 1, dtype=torch.float64)
    s.index_add_(0, inp["model_of"], terms)
    mag.index_add_(0, inp["model_of"], terms.abs())
    return s, mag


def check_fused_chain(case, inp, ops, dev):
    spec, P, K = inp["spec"], inp["P"], inp["K"]
    rows, mo = inp["rows"], inp["model_of"]
    x, y = inp["x"].to(dev), inp["y"].to(dev)
    rest = torch.ones(inp["R"], dtype=torch.bool)
    rest[rows] = False
    empty = torch.ones(K, dtype=torch.bool)
    empty[mo] = False
    assert empty.tolist() == [False, False, False, True]
    assert int((inp["sw"] == 0).sum()) >= 4
    figs, ties = {}, []

    def train(j, params, opt, glob, partial, o64, o32):
        """Launch j under test and its float64 / fp32 references from the
        same global bank; folds the errors into figs, returns the trained
        replicas [G, P] of the op under test."""
        L = inp["launches"][j]
        before = snapshot(params, opt)
        start = glob.detach().cpu().clone()
        fused_launch(ops, inp, params, opt, x, y, L, glob, partial)
        sk = snapshot(params, opt)
        before64 = snapshot(inp["params"], o64)
        s64 = fused_train_ref(inp, L, start, o64, torch.float64)
        s32 = fused_train_ref(inp, L, start, o32, torch.float32)
        # the pair at rate inf is compared with nothing but itself
        wild = rows[inp["wild"]]
        assert not torch.isfinite(sk["param"][wild]).all(), (case, j)
        for snap in (sk, s64, s32):
            for q in ROUND_QS:
                snap[q][wild] = 0.0
        worst_figures(figs, s64, s32=s32)
        start64 = inp["params"].double()
        start64[rows] = start.double()[mo]
        for g in adopt_relu_ties(case, spec, inp["x"].double(), inp["y"], L,
                                 start64, before64, s64, sk):
            ties.append((j, g))
            for q in ("m", "v", "vmax"):     # the reference carries on from
                o64[q][rows[g]] = s64[q][rows[g]]    # the adopted state
        worst_figures(figs, s64, sk=sk)
        assert torch.equal(sk["t"], s64["t"]), (case, j)
        assert_rows_identical((case, j, "rest"), before, sk, rest)
        if L["dead"] is not None:
            # an all-empty pair still takes the broadcast, and keeps its state
            r = rows[L["dead"]:L["dead"] + 1]
            assert torch.equal(sk["param"][r], start[mo[L["dead"]]][None])
            for q in ("m", "v", "vmax", "t"):
                assert torch.equal(sk[q][r], before[q][r]), (case, j, q)
        return sk["param"][rows]

    def fresh():
        return (inp["params"].to(dev).clone(),
                opt_to(inp["state"], dev, torch.float32),
                opt_to(inp["state"], "cpu", torch.float64),
                opt_to(inp["state"], "cpu", torch.float32))

    # step 1: one launch into a pre-filled partial: the kernel adds
    params, opt, o64, o32 = fresh()
    glob = inp["glob"].to(dev).clone()
    partial = inp["prefill"].to(dev).clone()
    reps = train(0, params, opt, glob, partial, o64, o32)
    assert torch.equal(glob.cpu(), inp["glob"])
    s, mag = weighted_sums(inp, reps)
    pre = inp["prefill"].double()
    part = partial.cpu()
    err = (part.double() - (pre + s)).abs()
    bound = 2 * FUSED_TERMS * U24 * (pre.abs() + mag)
    record(case, "partial/bound", None, (err / bound)[~empty].max().item(),
           1.0)
    assert (err <= bound).all(), (case, (err / bound).max())
    assert torch.equal(part[:, P].double(), (pre + s)[:, P]), case   # exact
    assert torch.equal(part[empty], inp["prefill"][empty]), case

    # step 2: train, apply with model 1 masked, train into the SAME partial
    # with no fill in between, apply: the second apply shows whatever the
    # first left behind
    params, opt, o64, o32 = fresh()
    partial = torch.zeros(K, P + 1, device=dev)
    for j in range(2):
        reps = train(j, params, opt, glob, partial, o64, o32)
        s, mag = weighted_sums(inp, reps)
        tot = s[:, P]
        mask = torch.tensor([1, 0, 1, 1], dtype=torch.uint8) if j == 0 \
            else None
        upd = tot > 0
        if mask is not None:
            upd &= mask.bool()
        assert upd.tolist() == [True, j == 1, True, False]
        before = glob.cpu().clone()
        totals = apply_aggregate(ops, glob, partial,
                                 None if mask is None else mask.to(dev))
        after = glob.cpu()
        mean = s[upd, :P] / tot[upd, None]
        bound = 4 * U24 * mean.abs() \
            + 2 * FUSED_TERMS * U24 * mag[upd, :P] / tot[upd, None]
        err = (after[upd].double() - mean).abs()
        record(case, f"apply {j} mean/bound", None,
               (err / bound).max().item(), 1.0)
        assert (err <= bound).all(), (case, j, (err / bound).max())
        assert torch.equal(after[~upd], before[~upd]), (case, j)
        assert partial.abs().max().item() == 0.0, \
            (case, j, "partial must be drained, masked rows included")
        assert torch.equal(totals.cpu().double(), tot), (case, j)
    # three launches of G pairs; tied pairs (adopt_relu_ties) stay rare
    record(case, "pairs at a ReLU tie", None, len(ties),
           NEAR_TIE_MAX_SHARE * 3 * FUSED_G)
    assert len(ties) <= NEAR_TIE_MAX_SHARE * 3 * FUSED_G, (case, ties)
    record_and_assert_train(case, figs)
    return figs


def fused_cases():
    for i, (kind, d, o) in enumerate(SMALL_SHAPES):
        yield (f"fused chain {kind}({d},{o}) mask={i % 2}", kind, d, o,
               bool(i % 2), 510 + i)


def case_rounds_small_fused(ops=None, dev=None):
    """Part B on the small train kernel and apply_aggregate_kernel."""
    if ops is None:
        from feddrift_amd.ops import mlp_hip as ops
        dev = _dev()
    for case, kind, d, o, masked, seed in fused_cases():
        check_fused_chain(case, fused_inputs(kind, d, o, masked, seed), ops,
                          dev)


# -- C: FLJob rounds on the default aggregation path -----------------------

JOB_ROUNDS = ("plan", "plan", "second", "plan", "masked", "second", "empty",
              "plan", "plan")


def second_template(tmpl):
    """The algorithm's template minus its last pair, and with the
    aggregation weight of another pair of the same model set to 0 (that
    pair still trains). In the two-pairs-per-model job of
    secagg_cases.make_job that model's total is then 0 with a pair
    training, and the other model keeps its full mean."""
    from feddrift_amd.engine.fljob import build_template
    K = tmpl.sample_num.shape[1]
    pairs = []
    for i in range(len(tmpl.rows) - 1):
        a, n = int(tmpl.pool_start[i]), int(tmpl.pool_size[i])
        pairs.append((int(tmpl.rows[i]),
                      list(zip(tmpl.pool_off[a:a + n].tolist(),
                               tmpl.pool_len[a:a + n].tolist()))))
    sample = np.array(tmpl.sample_num, copy=True)
    last = int(tmpl.rows[-1])
    mate = next(int(r) for r in tmpl.rows[:-1] if r % K == last % K)
    for r in (last, mate):
        assert sample[r // K, r % K] > 0
        sample[r // K, r % K] = 0
    return build_template(pairs, sample)


def drive_fljob_rounds(job, case, drained, rounds=JOB_ROUNDS):
    """Rounds by hand, each held to float64: the trained replicas (from the
    pre-round global rows, this round's own windows and the carried
    optimizer state) and the aggregated models. `drained`: the apply kernel
    leaves job._partial at zero (the fused path)."""
    from feddrift_amd.engine.fljob import TrainPlan
    from secagg_cases import mean_and_bound_atomic, torch_sync
    spec, K, E = job.spec, job.n_models, job.cfg.epochs
    ci = job.client_sampling(0)
    x64, y = job.arena.x.cpu().double(), job.arena.y.cpu()
    first = job.algo.plan(job, 0, ci)
    tmpl2 = second_template(first.template)
    populated = int(first.rows[0] % K)
    figs, worst_mean, seen_masked, n_ties = {}, 0.0, False, 0
    for r, what in enumerate(rounds):
        mask = None
        if what in ("plan", "masked"):
            plan = first if r == 0 else job.algo.plan(job, r, ci)
            if what == "masked":
                mask = np.ones(K, dtype=bool)
                mask[populated] = False
        elif what == "second":
            plan = tmpl2.draw(job.pick_rng, E)
        else:
            plan = TrainPlan(np.zeros(0, np.int64), np.zeros((0, E), np.int64),
                             np.zeros((0, E), np.int64),
                             np.zeros_like(first.sample_num))
        # the template's scratch arrays are overwritten by the next draw
        rows = torch.from_numpy(np.array(plan.rows, copy=True))
        L = dict(rows=rows,
                 off=torch.from_numpy(np.array(plan.step_off, copy=True)),
                 ln=torch.from_numpy(np.array(plan.step_len, copy=True)))
        glob0 = job.global_params.detach().cpu().clone()
        before = snapshot(job.replicas, job.opt)
        o64 = opt_to(job.opt, "cpu", torch.float64)

        job.train(plan)
        torch_sync(job)
        after = snapshot(job.replicas, job.opt)
        if len(rows):
            p64 = torch.zeros(job.replicas.shape, dtype=torch.float64)
            p64[rows] = glob0.double()[rows % K]
            before64 = snapshot(p64, o64)
            launch(mlp_torch, spec, p64, o64, x64, y, L)
            s64 = snapshot(p64, o64)
            n_ties += len(adopt_relu_ties(f"{case} r{r}", spec, x64, y, L,
                                          before64["param"], before64, s64,
                                          after))
            kes = {q: (after[q][rows].double() - s64[q][rows]).abs().max()
                   .item() for q in ROUND_QS if q in s64}
            for q, ke in kes.items():
                record(f"{case} r{r} {what}", q, None, ke,
                       ROUND_TRAIN_TOL[q])
                figs[q] = max(figs.get(q, 0.0), ke)
            for q, ke in kes.items():
                assert ke <= ROUND_TRAIN_TOL[q], (case, r, what, q, ke)
            if "t" in s64:
                assert torch.equal(after["t"], s64["t"]), (case, r, what)
        rest = torch.ones(job.replicas.shape[0], dtype=torch.bool)
        rest[rows] = False
        for q in before:
            if q != "param":    # the unfused path re-syncs every replica
                assert torch.equal(after[q][rest], before[q][rest]), \
                    (case, r, q)

        mean, bound, has = mean_and_bound_atomic(job.replicas,
                                                 plan.sample_num, K)
        job.aggregate(plan, mask)
        torch_sync(job)
        gp = job.global_params.detach().cpu()
        upd = has if mask is None else has & mask
        if what == "plan":
            assert upd[populated]
        if what == "masked":
            assert has[populated] and not upd[populated]
            seen_masked = True
        if what == "empty":
            assert not has.any()
        if what == "second":
            # a model whose only weighted pair left the plan stays put
            assert has.any() and not has.all()
        for m in range(K):
            if not upd[m]:
                assert torch.equal(gp[m], glob0[m]), (case, r, what, m)
                continue
            ratio = float((np.abs(gp[m].double().numpy() - mean[m])
                           / bound[m]).max())
            record(f"{case} r{r} {what}", f"model {m} mean/bound", None,
                   ratio, 1.0)
            worst_mean = max(worst_mean, ratio)
            assert ratio <= 1.0, (case, r, what, m, ratio)
        if drained:
            assert job._partial.abs().max().item() == 0.0, (case, r, what)
    assert seen_masked or "masked" not in rounds
    assert n_ties <= 1, (case, n_ties)     # pairs at a ReLU tie stay rare
    figs["mean/bound"] = worst_mean
    return figs


# --------------------------------------------------------------------------
# CNN
# --------------------------------------------------------------------------

CNN_N = 400
NF, NH = 9216, 128
GRAD_LENS = [1, 15, 16, 17, 63, 64, 65, 0]   # B = 65: mtiles = 2
LAYERS = ["conv1.w", "conv1.b", "conv2.w", "conv2.b",
          "fc1.w", "fc1.b", "fc2.w", "fc2.b"]
CNN_LR = 1e-3


def cnn_world(O=10, K=2, seed=0):
    from feddrift_amd.models import zoo
    from feddrift_amd.models.generic_packer import ModulePacker
    proto = zoo.CNN_DropOut(only_digits=(O == 10))
    packer = ModulePacker(proto)
    g = torch.Generator().manual_seed(seed)
    gp = torch.randn(K, packer.n_params, generator=g) * 0.05
    x = torch.randn(CNN_N, 784, generator=g)
    y = torch.randint(0, O, (CNN_N,), generator=g)
    bounds = np.concatenate([[0], np.cumsum(packer.numels)])
    return dict(proto=proto, packer=packer, gp=gp, x=x, y=y, O=O, K=K,
                P=packer.n_params, bounds=bounds)


def cnn_model(world, k, dtype):
    from feddrift_amd.models import zoo
    m = zoo.CNN_DropOut(only_digits=(world["O"] == 10)).to(dtype).eval()
    world["packer"].load_into(m, world["gp"][k].to(dtype))
    return m


def cnn_pool_windows(m, x):
    """conv1 -> conv2 as 2x2 pooling windows [n, 9216, 4]: window order is
    the flatten order [c][py][px], element order dy * 2 + dx."""
    z = m.conv2d_2(m.conv2d_1(x.reshape(-1, 28, 28).unsqueeze(1)))
    n = z.shape[0]
    return z.reshape(n, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5) \
        .reshape(n, NF, 4)


def cnn_pool_select(u, pidx=None):
    """Max-pool of windows u [n, 9216, 4] -> (pooled, argmax, near-tied).

    The pool's argmax routes the whole gradient of its window, so a window
    whose two largest float64 values lie within POOL_TIE has two right
    answers (fp32 torch flips such windows too: one flip in a 5-sample
    step moved conv2's weight gradient by 6e-3 of its maximum). There, and
    only there, the reference adopts the choice `pidx` of the
    implementation under comparison, provided that choice is one of the
    tied maxima; every other window keeps float64's own argmax."""
    top = u.detach().topk(2, dim=2)
    idx = top.indices[..., 0]
    near = (top.values[..., 0] - top.values[..., 1]) < POOL_TIE
    if pidx is not None:
        cand = u.detach().gather(2, pidx.unsqueeze(2))[..., 0] \
            >= top.values[..., 0] - POOL_TIE
        idx = torch.where(near & cand, pidx, idx)
    return u.gather(2, idx.unsqueeze(2))[..., 0], idx, near


def cnn_ref_grad(world, k, off, n, dtype, xmask=None, s1=None, s2=None,
                 pidx=None):
    """Gradient of F.cross_entropy(model(x), y) (the model output is already
    a softmax: the double softmax is the reference's semantics) by plain
    autograd on the CPU, for one (model, window) pair. The forward is the
    module's own layers in the module's order; s1 [n, 9216] / s2 [n, 128]
    are fixed dropout keep-scales (None: dropout off), pidx [n, 9216] is
    the compared implementation's pool argmax (see cnn_pool_select).
    Returns dict(grad [P], pooled [n, 9216], idx, near)."""
    m = cnn_model(world, k, dtype)
    xs = world["x"][off:off + n].to(dtype)
    if xmask is not None:
        xs = xs * xmask.to(dtype)
    ys = world["y"][off:off + n]
    pooled, idx, near = cnn_pool_select(cnn_pool_windows(m, xs), pidx)
    a2 = pooled if s1 is None else pooled * s1.to(dtype)
    a1 = m.relu(m.linear_1(a2))
    if s2 is not None:
        a1 = a1 * s2.to(dtype)
    out = m.softmax(m.linear_2(a1))
    if s1 is None and s2 is None and not bool(near.any()):
        assert torch.equal(out, m(xs))       # it IS the module's forward
    loss = F.cross_entropy(out, ys)
    named = dict(m.named_parameters())
    gs = torch.autograd.grad(loss, [named[k_] for k_ in world["packer"].keys])
    return dict(grad=torch.cat([g.reshape(-1) for g in gs]),
                pooled=pooled.detach(), idx=idx, near=near)


def layer_metric(world, g, g64):
    """max|g - g64| / max|g64| per layer (8 values)."""
    b = world["bounds"]
    out = []
    for i in range(8):
        a, r = g[b[i]:b[i + 1]].double(), g64[b[i]:b[i + 1]]
        out.append(((a - r).abs().max() / r.abs().max()).item())
    return out


def cnn_plan(lens, seed):
    from feddrift_amd.engine.fljob import TrainPlan
    G = len(lens)
    rng = np.random.default_rng(seed)
    off = rng.integers(0, CNN_N - max(lens), (G, 1)).astype(np.int64)
    ln = np.asarray(lens, dtype=np.int64).reshape(G, 1)
    return TrainPlan(np.arange(G, dtype=np.int64), off, ln,
                     np.ones((G, 1), dtype=np.float32))


def cnn_engine(world, dropout=False):
    import copy
    from feddrift_amd.ops.cnn_hip import CnnHipEngine
    eng = CnnHipEngine(copy.deepcopy(world["proto"]), world["packer"], _dev())
    if not dropout:
        eng.dropout_override = (0.0, 0.0)
    return eng


def cnn_sgd_epoch(eng, world, plan, xmask=None):
    """One SGD epoch. Returns the replicas, the gradient the step consumed
    and the forward state left in the workspace ([G, B, .] with the
    launch's own B, whatever the workspace was sized to)."""
    dev = _dev()
    G, B = len(plan.rows), int(plan.step_len.max())
    reps = torch.zeros(G, world["P"], device=dev)
    opt = eng.make_opt_state("sgd", G, CNN_LR, 0.0)
    eng.train(world["gp"].to(dev), reps, plan, opt, world["x"].to(dev),
              world["y"].to(dev), world["K"],
              x_mask=None if xmask is None else xmask.to(dev))
    torch.cuda.synchronize()
    ws = eng._ws
    take = lambda k, w: ws[k][:G * B * w].view(G, B, w).cpu()  # noqa: E731
    return dict(reps=reps.cpu(), grad=ws["grad"][:G].cpu(),
                a2=take("a2", NF), pidx=take("pidx", NF).long(),
                z1=take("z1", NH), a1=take("a1", NH))


def check_cnn_grads(case, world, plan, run, xmask=None, scales=None):
    """Per-layer gradients of every pair against float64 autograd; scales
    [g] = (s1, s2) are recovered dropout keep-scales (None: dropout off)."""
    worst = [0.0] * 8
    scale_max = max(float(s[0].max()) for s in scales) if scales else 1.0
    pool_err, n_near, n_pool = 0.0, 0, 0
    lr = torch.tensor(CNN_LR, dtype=torch.float32).double()
    for g in range(len(plan.rows)):
        n = int(plan.step_len[g, 0])
        w = world["gp"][g % world["K"]]
        if n == 0:
            # a zero-length pair keeps the broadcast model exactly
            assert torch.equal(run["reps"][g], w), (case, g)
            continue
        s1, s2 = scales[g] if scales else (None, None)
        ref = cnn_ref_grad(world, g % world["K"], int(plan.step_off[g, 0]),
                           n, torch.float64,
                           None if xmask is None else xmask[g], s1, s2,
                           run["pidx"][g, :n])
        n_near += int(ref["near"].sum())
        n_pool += ref["near"].numel()
        # a2 is the pooled activation times its keep-scale (0 or 1/(1-p))
        a2_64 = ref["pooled"] if s1 is None else ref["pooled"] * s1
        pool_err = max(pool_err, (run["a2"][g, :n].double() - a2_64)
                       .abs().max().item() / scale_max)
        worst = [max(a, b) for a, b in
                 zip(worst, layer_metric(world, run["grad"][g], ref["grad"]))]
        # replicas == global - lr * grad, to fp32 rounding: one rounding of
        # lr*g and one of the difference (or a single fused one)
        step = lr * run["grad"][g].double()
        want = w.double() - step
        slack = 2.0 ** -23 * (w.double().abs() + step.abs()) + 1e-38
        assert ((run["reps"][g].double() - want).abs() <= slack).all(), \
            (case, g)
    for i, name in enumerate(LAYERS):
        record(case, name, CNN_GRAD_ERR32[i], worst[i], CNN_GRAD_TOL[i])
    record(case, "pooled", CNN_POOL_ERR32, pool_err, CNN_POOL_TOL)
    assert pool_err <= CNN_POOL_TOL, (case, pool_err)
    assert n_near <= POOL_TIE_MAX_SHARE * n_pool, (case, n_near, n_pool)
    for i, name in enumerate(LAYERS):
        assert worst[i] <= CNN_GRAD_TOL[i], \
            (case, name, worst[i], CNN_GRAD_TOL[i])


def case_cnn_grad_edges(case="cnn grad B=65", engine=None):
    """Per-layer gradient parity at [1, 15, 16, 17, 63, 64, 65, 0]: B = 65,
    two 64-row fc1 m-tiles, MFMA fragment edges, a zero-length pair; on a
    fresh workspace sized to exactly this G and B."""
    world = cnn_world(10, K=2)
    plan = cnn_plan(GRAD_LENS, seed=1)
    eng = engine or cnn_engine(world)
    run = cnn_sgd_epoch(eng, world, plan)
    assert eng._ws["G"] == len(GRAD_LENS) and eng._ws["B"] == 65
    check_cnn_grads(case, world, plan, run)
    return eng, world


# -- eval -------------------------------------------------------------------

# (model row, length) per window: the row runs hold 63, 64 and 130 slots, so
# the fc1 blocks come out at 63, 64 and 64/64/2; given in shuffled row order
EVAL_WINDOWS = [(2, 65), (0, 40), (1, 64), (2, 64), (0, 23), (2, 1)]
EVAL_T = 4


def cnn_eval_inputs(world, seed=5):
    rng = np.random.default_rng(seed)
    tr = torch.tensor([r for r, _ in EVAL_WINDOWS])
    ln = torch.tensor([n for _, n in EVAL_WINDOWS])
    ti = torch.from_numpy(rng.integers(0, EVAL_T, len(EVAL_WINDOWS)))
    off = torch.from_numpy(rng.integers(0, CNN_N - 65, len(EVAL_WINDOWS)))
    return tr, ti, off, ln


def cnn_eval_ref(world, wins, dtype, xmask=None):
    """Per window: probabilities, per-sample CE and mse terms, labels."""
    tr, ti, off, ln = wins
    out = []
    models = {}
    with torch.no_grad():
        for w in range(len(tr)):
            k, o, n = int(tr[w]), int(off[w]), int(ln[w])
            if k not in models:
                models[k] = cnn_model(world, k, dtype)
            xs = world["x"][o:o + n].to(dtype)
            if xmask is not None:
                xs = xs * (xmask if xmask.dim() == 1 else xmask[w]).to(dtype)
            ys = world["y"][o:o + n]
            p = models[k](xs)
            ce = F.cross_entropy(p, ys, reduction="none")
            pt = torch.softmax(p, 1).gather(1, ys[:, None])[:, 0]
            out.append(dict(p=p, ce=ce, mse=(1 - pt) ** 2, y=ys))
    return out


def check_cnn_eval(case, world, eng, wins, xmask=None):
    from feddrift_amd.ops.cnn_hip import EV_DUMP
    dev = _dev()
    O, T = world["O"], EVAL_T
    tr, ti, off, ln = wins
    ref = cnn_eval_ref(world, wins, torch.float64, xmask)
    gp, x, y = world["gp"].to(dev), world["x"].to(dev), world["y"].to(dev)
    d = [t.to(dev) for t in wins]
    xm = None if xmask is None else xmask.to(dev)

    # per-sample probabilities, through the dump tail vote_multi uses; the
    # sink sees the windows stably sorted by model row
    chunks = []
    eng._x_arena, eng._y_arena = x, y
    eng._eval_sweep(gp, *d, T, EV_DUMP, x_mask=xm,
                    dump_sink=lambda stid, sy, p: chunks.append(
                        (stid.cpu(), sy.cpu(), p.cpu())))
    order = torch.argsort(tr, stable=True).tolist()
    p64 = torch.cat([ref[w]["p"] for w in order])
    y64 = torch.cat([ref[w]["y"] for w in order])
    t64 = torch.cat([ti[w].repeat(int(ln[w])) for w in order])
    assert torch.equal(torch.cat([c[0] for c in chunks]), t64), case
    assert torch.equal(torch.cat([c[1] for c in chunks]), y64), case
    pk = torch.cat([c[2] for c in chunks])
    perr = (pk.double() - p64).abs().max().item()
    record(case, "prob", CNN_PROB_ERR32, perr, CNN_PROB_TOL)

    top2 = p64.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < NEAR_TIE_CNN
    assert near.float().mean().item() <= NEAR_TIE_MAX_SHARE, case
    pred = p64.argmax(1)
    want = torch.zeros(4, T, dtype=torch.float64)
    want[0].index_add_(0, t64, (pred == y64).double())
    want[1].index_add_(0, t64, torch.ones_like(y64, dtype=torch.float64))
    want[2].index_add_(0, t64, torch.cat([ref[w]["ce"] for w in order]))
    want[3].index_add_(0, t64, torch.cat([ref[w]["mse"] for w in order]))
    near_t = torch.zeros(T, dtype=torch.float64).index_add_(
        0, t64, near.double())
    conf = torch.zeros(T, O, O, dtype=torch.float64)
    conf.view(-1).index_add_(0, (t64 * O + y64) * O + pred,
                             torch.ones_like(y64, dtype=torch.float64))
    near_ty = torch.zeros(T, O, dtype=torch.float64)
    near_ty.view(-1).index_add_(0, t64 * O + y64, near.double())

    acc = eng.eval_tasks_stacked(gp, *d, T, want_mse=True, x_arena=x,
                                 y_arena=y, x_mask=xm).cpu()
    cf = eng.confusion_tasks(gp, x, y, *d, T, O, x_mask=xm).cpu()
    torch.cuda.synchronize()
    lerr = ((acc[2] - want[2]).abs() / want[1].clamp(min=1)).max().item()
    merr = ((acc[3] - want[3]).abs() / want[1].clamp(min=1)).max().item()
    record(case, "loss/sample", CNN_LOSS_ERR32, lerr, CNN_LOSS_TOL)
    record(case, "mse/sample", CNN_MSE_ERR32, merr, CNN_MSE_TOL)

    assert perr <= CNN_PROB_TOL, (case, perr)
    assert torch.equal(acc[1], want[1]), case
    assert ((acc[0] - want[0]).abs() <= near_t).all(), (case, acc[0], want[0])
    assert lerr <= CNN_LOSS_TOL, (case, lerr)
    assert merr <= CNN_MSE_TOL, (case, merr)
    # confusion: every sample lands in its (task, label) row; a cell may be
    # off by the near-tied samples of that row, nowhere else
    assert torch.equal(cf.sum(2), conf.sum(2)), case
    assert ((cf - conf).abs() <= near_ty[:, :, None]).all(), case


def case_cnn_eval_dump(case="cnn eval O=10", O=10):
    world = cnn_world(O, K=3, seed=2)
    eng = cnn_engine(world)
    check_cnn_eval(case, world, eng, cnn_eval_inputs(world))
    return eng, world


# --------------------------------------------------------------------------
# err32: the yardstick column of the PARITY.md table (CPU only)
# --------------------------------------------------------------------------

def measure_mlp_train_err32():
    worst = {"param": 0.0, "m": 0.0, "v": 0.0, "vmax": 0.0}
    sets = [(SMALL_SHAPES, SMALL_LENS, [100 + i for i in range(5)]),
            (GENERIC_SHAPES, GENERIC_LENS, GENERIC_SEEDS)]
    for shapes, lens, seeds in sets:
        for i, (kind, d, o) in enumerate(shapes):
            for optname in ("sgd", "adam"):
                for masked in (False, True):
                    inp = mlp_train_inputs(kind, d, o, lens, masked, seeds[i])
                    figs, _ = mlp_train_figures(inp, optname)
                    for k, (e32, _) in figs.items():
                        print(f"{kind}({d},{o}) {optname} mask={int(masked)}"
                              f" {k} err32={e32:.3e}")
                        worst[k] = max(worst[k], e32)
    # the fused broadcast/partial case of test_gpu_mlp_edges (the broadcast
    # only replaces the start weights; same conditioning)
    inp = mlp_train_inputs("fnn", 12, 4, GENERIC_LENS, False, FUSED_SEED, G=9)
    for k, (e32, _) in mlp_train_figures(inp, "adam")[0].items():
        print(f"fused fnn(12,4) adam {k} err32={e32:.3e}")
        worst[k] = max(worst[k], e32)
    return worst


def measure_round_err32():
    """ROUND_TRAIN_ERR32: every part A and part B case with fp32 mlp_torch
    standing in for the kernel (its `kernel` figure is then err32)."""
    worst = {q: 0.0 for q in ROUND_QS}
    for small in (True, False):
        for case, kind, d, o, lens, seed, optname in carried_cases(small):
            figs = check_carried(case, carried_inputs(kind, d, o, lens, seed),
                                 optname, mlp_torch, "cpu")
            for q, (e32, _) in figs.items():
                worst[q] = max(worst[q], e32)
    for case, kind, d, o, masked, seed in fused_cases():
        figs = check_fused_chain(case, fused_inputs(kind, d, o, masked, seed),
                                 mlp_torch, "cpu")
        for q, (e32, _) in figs.items():
            worst[q] = max(worst[q], e32)
    return worst


CASES = {"small_train": case_small_train,
         "rounds_small_train": case_rounds_small_train,
         "rounds_small_fused": case_rounds_small_fused,
         "cnn_grad_edges": case_cnn_grad_edges,
         "cnn_eval_dump": case_cnn_eval_dump}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print(f"usage: {argv[0]} {{{'|'.join(CASES)}}}")
        return 2
    CASES[argv[1]]()
    print(f"case {argv[1]} OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
