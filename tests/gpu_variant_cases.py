"""Check bodies shared by tests/test_gpu_mlp_edges.py, tests/test_gpu_cnn_edges.py
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


CASES = {"small_train": case_small_train,
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
