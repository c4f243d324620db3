"""FedProx proximal local training (`fedprox_mu`) on the CPU.

Every executed local step hands the optimizer grad + mu * (w - w0), w0 being
the weights the pair started the round from (Li et al., MLSys 2020). The
specification is ops/mlp_torch.train_fused; here it is held to an
independent oracle (eager torch minimising CE + mu/2 |p - p0|^2 by autograd
with torch.optim), the module engines to the same kind of eager loop, and
FLJob rounds to a float64 replay of the specification. Shared bodies:
tests/fedprox_cases.py. The HIP kernels: tests/test_gpu_fedprox.py.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fedprox_cases as fc
import gpu_variant_cases as vc
import orderstat_cases as oc
import secagg_cases as sc
from feddrift_amd.config import Config, config_from_argv
from feddrift_amd.engine.fljob import TrainPlan
from feddrift_amd.models.generic_packer import ModulePacker
from feddrift_amd.models.packed import PackedMLP, spec_for
from feddrift_amd.models.zoo import (CNN_DropOut, FeedForwardNN,
                                     LogisticRegression)
from feddrift_amd.ops import mlp_hip, mlp_torch
from feddrift_amd.ops.module_engine import ModuleEngine
from feddrift_amd.ops.module_vmap import VmapEngine

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CPU = torch.device("cpu")


# ------------------------------------------------------- independent oracle

def _data(n, d, o, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, d, generator=g) * 10,
            torch.randint(0, o, (n,), generator=g))


def _flat(sd):
    return torch.cat([v.reshape(-1) for v in sd.values()])


def _eager_prox(model, opt, x, y, picks, batch, mu):
    params = list(model.parameters())
    p0 = [p.detach().clone() for p in params]
    for k in picks:
        xb, yb = x[k * batch:(k + 1) * batch], y[k * batch:(k + 1) * batch]
        opt.zero_grad()
        loss = F.cross_entropy(model(xb), yb)
        loss = loss + 0.5 * mu * sum(((p - q) ** 2).sum()
                                     for p, q in zip(params, p0))
        loss.backward()
        opt.step()


ORACLE_SHAPES = {"fnn": (3, 2, 50, 0), "lr": (4, 3, 40, 5)}


@pytest.mark.parametrize("mu", [0.1, 1.0])
@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("kind", ["fnn", "lr"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                         ids=["f64", "f32"])
def test_train_fused_matches_eager_prox(dtype, kind, optname, mu):
    """fnn(3->6->2) and lr(4->3), E = 5: float64 agrees with the autograd
    oracle to 1e-12 relative, float32 to the atol=2e-6, rtol=1e-5 of
    tests/test_ops.py::test_train_fused_matches_eager_fnn."""
    torch.manual_seed(7)
    d, o, batch, seed = ORACLE_SHAPES[kind]
    E, picks = 5, [1, 0, 3, 2, 1]
    spec = spec_for(kind, d, o)
    packer = PackedMLP(spec)
    x, y = _data(4 * batch, d, o, seed)
    x = x.to(dtype)
    model = (FeedForwardNN(d, o, 6) if kind == "fnn"
             else LogisticRegression(d, o)).to(dtype)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    if optname == "adam":
        opt = torch.optim.Adam(model.parameters(), lr=0.01,
                               weight_decay=0.001, amsgrad=True)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.01)
    _eager_prox(model, opt, x, y, picks, batch, mu)
    ref = _flat(model.state_dict())

    # the packed layout is the state_dict order (PackedMLP.flatten is fp32)
    assert torch.equal(packer.flatten(sd0), _flat(sd0).float())
    params = _flat(sd0).unsqueeze(0).clone()
    assert params.dtype == dtype
    ost = mlp_torch.make_opt_state(optname, 1, spec.n_params, 0.01, 0.001,
                                   "cpu", dtype=dtype, mu=mu)
    assert ost["mu"] == mu
    off = torch.tensor([[k * batch for k in picks]])
    ln = torch.full((1, E), batch)
    mlp_torch.train_fused(spec, params, torch.tensor([0]), x, y, off, ln, ost)
    err = (params[0] - ref).abs()
    print(f"FIG oracle {kind} {optname} mu={mu} {dtype} | "
          f"max err {err.max():.3e} | max rel {(err / ref.abs()).max():.3e}")
    # the term does something: the plain run ends elsewhere
    plain = _flat(sd0).unsqueeze(0).clone()
    mlp_torch.train_fused(spec, plain, torch.tensor([0]), x, y, off, ln,
                          mlp_torch.make_opt_state(optname, 1, spec.n_params,
                                                   0.01, 0.001, "cpu",
                                                   dtype=dtype))
    if dtype == torch.float64:
        # (the weakest case, lr with sgd at mu = 0.1, moves by 6e-6)
        assert (plain[0] - ref).abs().max() > 1e-6
        assert torch.allclose(params[0], ref, rtol=1e-12, atol=0.0), err.max()
    else:
        assert torch.allclose(params[0], ref, atol=2e-6, rtol=1e-5), err.max()


def test_anchor_argument_and_default():
    """anchor=None is the rows at entry; an explicit anchor is pulled to."""
    inp = vc.mlp_train_inputs("fnn", 3, 2, vc.SMALL_LENS, False, 100)
    spec, rows = inp["spec"], inp["rows"]
    x, p0 = inp["x"].double(), inp["params"].double()

    def run(anchor):
        p = p0.clone()
        opt = fc.prox_opt("adam", inp["R"], spec.n_params, "cpu",
                          torch.float64, 1.0)
        mlp_torch.train_fused(spec, p, rows, x, inp["y"], inp["off"],
                              inp["ln"], opt, anchor=anchor)
        return p
    assert torch.equal(run(None), run(p0[rows].clone()))
    moved = run(p0[rows] + 0.5)
    assert (moved - run(None)).abs().max() > 1e-3


# ---------------------------------------------------------- module engines

def _cnn_nodrop():
    m = CNN_DropOut(only_digits=True)
    m.dropout_1.p = 0.0
    m.dropout_2.p = 0.0
    return m


def _bn_model():
    from feddrift_amd.models.resnet import FlatImageModel
    torch.manual_seed(9)
    backbone = torch.nn.Sequential(
        torch.nn.Conv2d(1, 4, 3, padding=1), torch.nn.BatchNorm2d(4),
        torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(4 * 6 * 6, 3))
    return FlatImageModel(backbone, (1, 6, 6))


def _engine_world(which):
    torch.manual_seed(21)
    make, d, o, n = ((_cnn_nodrop, 784, 10, 64) if which == "cnn"
                     else (_bn_model, 36, 3, 256))
    # (B = n / 4 is a power of two: the vmap engine forms 1 / n in fp32)
    packer = ModulePacker(make())
    K, G = 2, 4
    rows = []
    for k in range(K):
        m = make()
        with torch.no_grad():      # distinct rows (_bn_model seeds its init)
            for p in m.parameters():
                p.add_(0.02 * k * torch.randn(p.shape))
        rows.append(packer.flatten(m.state_dict()))
    glob = torch.stack(rows)
    x = torch.rand(n, d) * (1.0 if which == "cnn" else 5.0)
    y = torch.randint(0, o, (n,))
    B = n // 4
    offs = np.array([[0, B, 2 * B], [B, 0, 3 * B], [2 * B, 3 * B, 0],
                     [3 * B, B, 2 * B]])
    lens = np.full((G, 3), B)
    lens[2, 1] = 0                 # a skipped step
    if which == "cnn":
        # (under vmap a BatchNorm model takes its batch statistics over the
        # padded batch, so the BN case keeps one length per step)
        lens[3, 0] = B // 2
    plan = TrainPlan(np.arange(G), offs, lens, np.ones((2, K)))
    return make, packer, glob, x, y, plan, K


# |engine - oracle| in float64: both run the same arithmetic in a different
# order (hand-written Adam against torch.optim, vmap's batched convolutions
# against eager ones); 1e-10 is 1e6 roundings of 1e-16 and at most a
# hundredth of what mu = 1 moves these weights by (asserted below)
ENGINE_TOL64 = 1e-10


@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("which", ["cnn", "bn"])
@pytest.mark.parametrize("engine", ["sequential", "vmap"])
def test_module_engines_match_eager_prox(engine, which, optname):
    """CNN_DropOut with dropout off, and a BatchNorm model, in float64: the
    term covers the trainable slice only, buffers move through the weights
    they saw (compared with the eager loop's buffers, not with mu = 0)."""
    make, packer, glob, x, y, plan, K = _engine_world(which)
    # (the engines build their rate vector in fp32: give the oracle that)
    lr, wd, mu = float(np.float32(0.01)), 0.001, 1.0
    glob, x = glob.double(), x.double()
    want = fc.eager_prox_round(make, packer, glob, plan, x, y, K, optname,
                               lr, wd, mu)
    plain = fc.eager_prox_round(make, packer, glob, plan, x, y, K, optname,
                                lr, wd, 0.0)
    cls = ModuleEngine if engine == "sequential" else VmapEngine
    eng = cls(make().double(), packer, CPU)
    opt = vc.opt_to(eng.make_opt_state(optname, len(plan.rows), lr, wd,
                                       mu=mu), CPU, torch.float64)
    assert opt["mu"] == mu
    reps = torch.zeros(len(plan.rows), packer.n_params, dtype=torch.float64)
    eng.train(glob.clone(), reps, plan, opt, x, y, n_models=K)
    err = (reps - want).abs()
    eff = (want - plain).abs().max().item()
    # the sequential engine leaves through ModulePacker.dump_from, which
    # rounds the row to fp32 once
    tol = ENGINE_TOL64 + (2.0 ** -24 * want.abs()
                          if engine == "sequential" else 0.0 * want)
    print(f"FIG {engine} {which} {optname} | err {err.max():.3e} | bound "
          f"{tol.max():.3e} | effect of mu {eff:.3e}")
    assert eff >= 100 * tol.max().item()
    assert (err <= tol).all(), err.max()
    if which == "bn":
        assert packer.n_train_params < packer.n_params
    if optname == "adam":
        assert opt["t"].tolist() == [3, 3, 2, 3]
    # mu = 0.0 and the call without the key: the same bits
    outs = []
    for mu0 in (0.0, None):
        o0 = vc.opt_to(eng.make_opt_state(optname, len(plan.rows), lr, wd),
                       CPU, torch.float64)
        if mu0 is None:
            del o0["mu"]
        r0 = torch.zeros_like(reps)
        eng.train(glob.clone(), r0, plan, o0, x, y, n_models=K)
        outs.append(r0)
    assert torch.equal(outs[0], outs[1])
    tol0 = ENGINE_TOL64 + (2.0 ** -24 * plain.abs()
                           if engine == "sequential" else 0.0 * plain)
    assert ((outs[0] - plain).abs() <= tol0).all()


# ------------------------------------------------- identities and behaviour

ALL_INPUTS = [(k, d, o, vc.SMALL_LENS, 100 + i)
              for i, (k, d, o) in enumerate(vc.SMALL_SHAPES)] + \
             [(k, d, o, vc.GENERIC_LENS, vc.GENERIC_SEEDS[i])
              for i, (k, d, o) in enumerate(vc.GENERIC_SHAPES)]


@pytest.mark.parametrize("kind,d,o,lens,seed", ALL_INPUTS)
def test_mu_zero_is_the_plain_run_bit_for_bit(kind, d, o, lens, seed):
    for optname in ("sgd", "adam"):
        for masked in (False, True):
            inp = vc.mlp_train_inputs(kind, d, o, lens, masked, seed)
            for dtype in (torch.float32, torch.float64):
                zero = fc.mlp_train_ref(inp, optname, dtype, 0.0)
                absent = fc.mlp_train_ref(inp, optname, dtype, None)
                assert "mu" not in absent[1] and zero[1]["mu"] == 0.0
                fc.assert_same_bits((kind, d, o, optname, masked), zero,
                                    absent)


@pytest.mark.parametrize("optname", ["sgd", "adam"])
def test_first_executed_step_is_free(optname):
    """w == w0 exactly at a pair's first executed step, so a pair with at
    most one executed step has the bits of mu = 0, wherever that step is."""
    inp = vc.mlp_train_inputs("fnn", 3, 2, vc.SMALL_LENS, True, 100)
    ln = torch.zeros_like(inp["ln"])
    for g in range(ln.shape[0] - 1):          # the last pair: no step at all
        ln[g, g % ln.shape[1]] = vc.SMALL_LENS[g % len(vc.SMALL_LENS)]
    inp = dict(inp, ln=ln)
    for dtype in (torch.float32, torch.float64):
        a = fc.mlp_train_ref(inp, optname, dtype, 0.0)
        b = fc.mlp_train_ref(inp, optname, dtype, 10.0)
        fc.assert_same_bits(optname, a, b)
        assert not torch.equal(a[0], inp["params"].to(dtype))
    # a second executed step is not free
    ln2 = ln.clone()
    ln2[0, (0 + 1) % ln.shape[1]] = 7
    inp2 = dict(inp, ln=ln2)
    a = fc.mlp_train_ref(inp2, optname, torch.float64, 0.0)
    b = fc.mlp_train_ref(inp2, optname, torch.float64, 10.0)
    r0 = inp["rows"][0]
    assert not torch.equal(a[0][r0], b[0][r0])
    rest = inp["rows"][1:]
    assert torch.equal(a[0][rest], b[0][rest])


@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("kind,d,o,lens,seed", [
    ("fnn", 3, 2, vc.SMALL_LENS, 100), ("fnn", 12, 4, vc.GENERIC_LENS, 102),
    ("lr", 4, 2, vc.GENERIC_LENS, 100)])
def test_larger_mu_stays_closer_to_the_anchor(kind, d, o, lens, seed,
                                              optname):
    """The mean over pairs of |w - w0| strictly decreases over mu = 0, 0.1,
    1, 10 (float64). Per-pair monotonicity does not hold and is not
    asserted."""
    inp = vc.mlp_train_inputs(kind, d, o, lens, False, seed)
    rows = inp["rows"]
    w0 = inp["params"].double()[rows]
    dist = []
    for mu in fc.MUS:
        p, _ = fc.mlp_train_ref(inp, optname, torch.float64, mu)
        dist.append((p[rows] - w0).norm(dim=1).mean().item())
    print(f"FIG drift {kind}({d},{o}) {optname} | " +
          " ".join(f"mu={m:g}:{v:.4e}" for m, v in zip(fc.MUS, dist)))
    assert all(a > b for a, b in zip(dist, dist[1:])), dist


# ------------------------------------------------------------------- config

def test_config_and_cli():
    assert Config().fedprox_mu == 0.0
    assert config_from_argv(["--fedprox_mu", "0.1"]).fedprox_mu == 0.1
    assert config_from_argv([]).fedprox_mu == 0.0
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="fedprox_mu"):
            Config(fedprox_mu=bad)
        with pytest.raises(ValueError, match="fedprox_mu"):
            mlp_torch.make_opt_state("sgd", 1, 3, 0.01, 0.0, "cpu", mu=bad)
    with pytest.raises(ValueError, match="fedprox_mu"):
        config_from_argv(["--fedprox_mu", "-1"])
    # a hand-built state is checked where it is used, too
    inp = vc.mlp_train_inputs("lr", 2, 2, vc.SMALL_LENS, False, 104)
    for bad in (-0.1, float("nan"), float("inf")):
        opt = fc.prox_opt("sgd", inp["R"], inp["spec"].n_params, "cpu",
                          torch.float32, bad)
        with pytest.raises(ValueError, match="fedprox_mu"):
            mlp_torch.train_fused(inp["spec"], inp["params"].clone(),
                                  inp["rows"], inp["x"], inp["y"],
                                  inp["off"], inp["ln"], opt)
    # every existing positional call keeps working
    st = mlp_torch.make_opt_state("adam", 2, 5, 0.01, 0.0, "cpu",
                                  torch.float64)
    assert st["mu"] == 0.0 and st["m"].dtype == torch.float64


def test_classic_fedavg_script_takes_the_option(monkeypatch):
    """scripts/run_fedavg_classic.py, run through its own main(): the value
    given on the command line is the one in the Config its FLJob gets."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "run_fedavg_classic_under_test",
        os.path.join(REPO, "scripts", "run_fedavg_classic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Caught(Exception):
        pass

    def fake_job(cfg, comm, logger, dataset=None):
        raise Caught(cfg)
    monkeypatch.setattr(mod, "FLJob", fake_job)
    base = ["run_fedavg_classic.py", "--dataset", "sea", "--model", "fnn",
            "--client_num_in_total", "2", "--client_num_per_round", "2",
            "--n_train", "40", "--n_test_per_client", "4"]
    for extra, want in (([], 0.0), (["--fedprox_mu", "0.25"], 0.25)):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(Caught) as e:
            mod.main()
        assert e.value.args[0].fedprox_mu == want
    monkeypatch.setattr(sys, "argv", base + ["--fedprox_mu", "-1"])
    with pytest.raises(ValueError, match="fedprox_mu"):
        mod.main()


# ----------------------------------------------------------------- fallback

@pytest.mark.parametrize("bcast", [False, True])
def test_large_mlp_fallback_forwards_the_anchor(monkeypatch, bcast):
    """A spec beyond the LDS caps takes mlp_torch inside mlp_hip.train_fused;
    with the fused broadcast the anchor is the global row, not the (zeroed)
    replica row the launch found."""
    def no_load():
        raise AssertionError("o > 64 reached the HIP extension")
    monkeypatch.setattr(mlp_hip.hip_loader, "load", no_load)
    torch.manual_seed(0)
    spec = spec_for("lr", 10, 100)
    assert not mlp_hip._fits_train(spec)
    n, G, E, K = 300, 3, 3, 2
    x, y = torch.rand(n, 10), torch.randint(0, 100, (n,))
    glob = torch.randn(K, spec.n_params) * 0.3
    model_of = torch.tensor([1, 0, 1], dtype=torch.int32)
    rows = torch.arange(G)
    off = torch.randint(0, n - 40, (G, E))
    ln = torch.randint(1, 40, (G, E))

    def opt():
        return mlp_torch.make_opt_state("adam", G, spec.n_params, 0.01, 1e-3,
                                        "cpu", mu=1.0)
    ref = glob[model_of.long()].clone()
    mlp_torch.train_fused(spec, ref, rows, x, y, off, ln, opt())
    if bcast:
        got = torch.zeros(G, spec.n_params)
        mlp_hip.train_fused(spec, got, rows, x, y, off, ln, opt(),
                            in_params=glob, model_of=model_of)
    else:
        got = glob[model_of.long()].clone()
        mlp_hip.train_fused(spec, got, rows, x, y, off, ln, opt())
    assert torch.equal(got, ref)
    plain = glob[model_of.long()].clone()
    mlp_torch.train_fused(spec, plain, rows, x, y, off, ln,
                          mlp_torch.make_opt_state("adam", G, spec.n_params,
                                                   0.01, 1e-3, "cpu"))
    assert (plain - ref).abs().max() > 1e-4


# -------------------------------------------------------------------- FLJob

def test_fljob_rounds_follow_the_specification(tmp_path):
    """A seeded SEA job with mu = 0.1 on the CPU: replicas and Adam state
    against the float64 replay under vc.ROUND_TRAIN_TOL, the aggregated
    models against the float64 mean of the job's replicas; and it is not
    the mu = 0 job."""
    job = sc.make_job(tmp_path / "a", device=CPU, fedprox_mu=0.1)
    twin = sc.make_job(tmp_path / "b", device=CPU)
    assert job.backend is mlp_torch and job.opt["mu"] == 0.1
    assert twin.opt["mu"] == 0.0
    ci = job.client_sampling(0)
    K = job.n_models
    for r in range(3):
        twin.global_params.copy_(job.global_params)
        plan, _, _ = fc.prox_round(job, "fljob cpu mu=0.1", r, ci)
        tplan = twin.algo.plan(twin, r, ci)
        assert np.array_equal(tplan.step_off, plan.step_off)
        twin.train(tplan)
        rows = torch.from_numpy(np.array(plan.rows))
        gap = (job.replicas[rows] - twin.replicas[rows]).abs().max().item()
        print(f"FIG fljob cpu r{r} | mu=0.1 against mu=0: {gap:.3e}")
        assert gap >= fc.EFFECT_FACTOR * vc.ROUND_TRAIN_TOL["param"], gap
        mean, bound, has = sc.mean_and_bound_atomic(job.replicas,
                                                    plan.sample_num, K)
        prev = job.global_params.double().numpy().copy()
        job.algo.aggregate(job, r, plan, ci)
        twin.algo.aggregate(twin, r, tplan, ci)
        gp = job.global_params.double().numpy()
        touched = 0
        for m in range(K):
            if not has[m] or np.array_equal(gp[m], prev[m]):
                continue
            touched += 1
            assert np.all(np.abs(gp[m] - mean[m]) <= bound[m]), (r, m)
        assert touched


COMPOSE = {
    "clip": dict(robust_fused=1, robust_norm_bound=0.05),
    "median": dict(robust_agg="median", n_clients=6),
    "ring": dict(secure_agg=2),
}


@pytest.mark.parametrize("what", list(COMPOSE))
def test_fljob_composes_with_the_aggregation_options(tmp_path, what):
    """mu = 0.1 under robust_fused=1 with a norm bound, robust_agg=median
    and secure_agg=2: the replicas equal the float64 replay `prox train
    (then clip)`, the global rows that aggregation's own float64 statistic
    of them, within that aggregation's own bound."""
    kw = COMPOSE[what]
    job = sc.make_job(tmp_path, device=CPU, fedprox_mu=0.1, **kw)
    ci = job.client_sampling(0)
    K = job.n_models
    for r in range(3):
        prev = job.global_params.double().numpy().copy()
        plan, _, _ = fc.prox_round(
            job, f"fljob cpu {what}", r, ci,
            clip_bound=kw.get("robust_norm_bound", 0.0))
        if what == "median":
            stat, bound, has, _ = oc.job_stat_and_bound(
                job.replicas, plan, K, "median", 0.0)
        elif what == "ring":
            stat, bound, has = sc.mean_and_bound(job.replicas,
                                                 plan.sample_num, K)
        else:
            stat, bound, has = sc.mean_and_bound_atomic(
                job.replicas, plan.sample_num, K)
        job.algo.aggregate(job, r, plan, ci)
        gp = job.global_params.double().numpy()
        touched = 0
        for m in range(K):
            if not has[m] or np.array_equal(gp[m], prev[m]):
                continue
            touched += 1
            err = np.abs(gp[m] - stat[m])
            print(f"FIG fljob cpu {what} r{r} model {m} | err/bound "
                  f"{(err / np.maximum(bound[m], 1e-300)).max():.3f}")
            assert np.all(err <= bound[m]), (what, r, m)
        assert touched
    if what == "clip":
        st = job.clip_stats()
        assert st[:, 1].sum() > 0


# --------------------------------------------------------------- multi-rank

_WORKER = r"""
import os, sys, pathlib
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
import torch
import secagg_cases as sc

job = sc.make_job(pathlib.Path({log!r}), device=torch.device("cpu"),
                  n_clients=6, fedprox_mu=0.1)
assert job.opt["mu"] == 0.1
ci = job.client_sampling(0)
K, E = job.n_models, job.cfg.epochs
for r in range(2):
    plan = job.algo.plan(job, r, ci)
    # batch picks that depend only on the global (worker, model) id and the
    # round, so every world size trains the same windows (the job's own
    # pick RNG is seeded per rank)
    t = plan.template
    for i, row in enumerate(plan.rows):
        w, m = job.owned_workers[int(row) // K], int(row) % K
        g = np.random.default_rng(1000 + (r * 64 + w) * K + m)
        pick = int(t.pool_start[i]) + g.integers(0, int(t.pool_size[i]), E)
        plan.step_off[i] = t.pool_off[pick]
        plan.step_len[i] = t.pool_len[pick]
    job.train(plan)
    if r == 1:
        reps = job.replicas.numpy().copy()
        before = job.global_params.numpy().copy()
    job.algo.aggregate(job, r, plan, ci)
np.savez(os.path.join({log!r}, "rank%d.npz" % job.comm.rank),
         global_params=job.global_params.numpy(), replicas=reps,
         before=before, owned=np.asarray(job.owned_workers),
         sample_num=np.asarray(plan.sample_num, dtype=np.float32))
"""


def _launch(nproc, log, port):
    os.makedirs(log, exist_ok=True)
    path = os.path.join(log, "worker.py")
    with open(path, "w") as f:
        f.write(_WORKER.format(repo=REPO, log=log))
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           "--nnodes", "1", "--nproc-per-node", str(nproc), path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_world2_matches_world1(tmp_path):
    """Two gloo ranks train the pairs one rank trains, from the same
    windows: the replicas of the second round agree per (worker, model)
    within the fp32 train bound (they start from global rows that differ by
    the rounding of round one's all-reduced sums), the final global rows
    within the bound of the mean plus that."""
    w1, w2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    _launch(1, w1, 29681)
    _launch(2, w2, 29682)
    one = np.load(os.path.join(w1, "rank0.npz"))
    two = [np.load(os.path.join(w2, f"rank{r}.npz")) for r in range(2)]
    assert np.array_equal(two[0]["global_params"].view(np.uint32),
                          two[1]["global_params"].view(np.uint32))
    K = one["sample_num"].shape[1]
    tol = vc.ROUND_TRAIN_TOL["param"]
    assert np.abs(one["before"] - two[0]["before"]).max() <= tol
    seen = 0
    for t in two:
        for wi, w in enumerate(t["owned"]):
            wi1 = list(one["owned"]).index(w)
            a = t["replicas"][wi * K:(wi + 1) * K].astype(np.float64)
            b = one["replicas"][wi1 * K:(wi1 + 1) * K].astype(np.float64)
            assert np.abs(a - b).max() <= tol, (w, np.abs(a - b).max())
            seen += 1
    assert seen == len(one["owned"]) == 6
    # the prox term was live: the replicas left their global rows
    assert np.abs(one["replicas"][:K] - one["before"]).max() > 1e-3
    mean, bound, upd = sc.mean_and_bound_atomic(
        torch.from_numpy(one["replicas"]), one["sample_num"], K)
    diff = np.abs(two[0]["global_params"].astype(np.float64)
                  - one["global_params"].astype(np.float64))
    for m in range(K):
        if upd[m]:
            print(f"FIG world2 model {m} | max diff {diff[m].max():.3e} | "
                  f"bound {bound[m].max():.3e}")
            assert np.all(diff[m] <= bound[m] + tol)
