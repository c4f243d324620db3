"""FedProx proximal local training on the HIP train kernels, against float64
on the CPU.

mlp_train_small_kernel (all five template shapes, both block sizes),
mlp_train_kernel and cnn_opt_step add mu * (w - w0) to the gradient of every
executed step, w0 read from where the weights were staged. Bodies and
bounds: tests/fedprox_cases.py (PARITY.md, "Proximal local training"): the
bound is min(4 x err32, 5e-5) with err32 taken at the same mu, every case
asserts that mu moves the float64 result by at least 10 x that bound, and
every MLP case asserts that mu = 0.0 gives the bits of a call without the
key. The CPU side: tests/test_fedprox.py.
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

import fedprox_cases as fc  # noqa: E402
import gpu_variant_cases as vc  # noqa: E402
import secagg_cases as sc  # noqa: E402
from feddrift_amd.engine.fljob import TrainPlan  # noqa: E402
from feddrift_amd.ops import mlp_hip, mlp_torch  # noqa: E402

DEV = torch.device("cuda:0")

SMALL = list(fc.small_cases())
GENERIC = list(fc.generic_cases())


# --------------------------------------------------------------------------
# MLP kernels
# --------------------------------------------------------------------------

@pytest.mark.parametrize("case,kind,d,o,optname,masked,seed", SMALL,
                         ids=[c[0].replace(" ", "-") for c in SMALL])
def test_small_kernel(case, kind, d, o, optname, masked, seed):
    """SMALL_LENS (1, 63, 64, 65, 200), G = 6, E = 4, one zero-length
    step; 64-thread blocks (the default)."""
    inp = vc.mlp_train_inputs(kind, d, o, vc.SMALL_LENS, masked, seed)
    assert int((inp["ln"] == 0).sum()) == 1
    fc.check_prox_train(case, inp, optname)


def test_small_kernel_256_thread_blocks():
    """fnn(3,2) x {sgd, adam} x {no mask, x_mask} in a child process with
    FEDDRIFT_TRAIN_BS64_MIN_G set huge (latched once per process)."""
    from feddrift_amd.ops import hip_loader
    hip_loader.load()                  # the child must find it built
    env = dict(os.environ, FEDDRIFT_TRAIN_BS64_MIN_G="1000000")
    r = subprocess.run([sys.executable, fc.__file__, "small_bs256"], env=env,
                       timeout=240, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-4000:])
    assert "case small_bs256 OK" in r.stdout


@pytest.mark.parametrize("case,kind,d,o,optname,seed", GENERIC,
                         ids=[c[0].replace(" ", "-") for c in GENERIC])
def test_generic_kernel(case, kind, d, o, optname, seed):
    """fnn(12,4) P = 412, fnn(8,5) P = 229, lr(4,2) P = 10 with
    GENERIC_LENS (1, 511, 512, 513, 1100)."""
    inp = vc.mlp_train_inputs(kind, d, o, vc.GENERIC_LENS, False, seed)
    assert inp["spec"].n_params in (412, 229, 10)
    fc.check_prox_train(case, inp, optname)


def test_fused_broadcast_anchor_is_the_global_row():
    """The replica rows the launch finds are zero; the weights and the
    anchor both come from in_params. A kernel that took the anchor from the
    replica row would pull every weight towards 0."""
    inp = fc.fused_inputs()
    glob, model_of, sw = inp["glob"], inp["model_of"], inp["sample_w"]
    K, P = fc.FUSED_K, inp["spec"].n_params
    assert not inp["params"][inp["rows"]].any()
    partial = torch.zeros(K, P + 1, device=DEV)
    # what the wrong anchor would give, in float64: far outside the bound
    wrong = dict(inp, params=inp["params"].clone(), bcast=None)
    wrong["params"][inp["rows"]] = glob[model_of]
    spec = inp["spec"]
    pw = wrong["params"].double()
    ow = fc.prox_opt("adam", inp["R"], P, "cpu", torch.float64, fc.MU)
    mlp_torch.train_fused(spec, pw, inp["rows"], inp["x"].double(), inp["y"],
                          inp["off"], inp["ln"], ow,
                          anchor=torch.zeros(9, P, dtype=torch.float64))
    right, _ = fc.mlp_train_ref(inp, "adam", torch.float64, fc.MU)
    gap = (pw - right).abs().max().item()
    vc.record("prox fused fnn(12,4)", "zero-row anchor against global-row",
              None, gap, fc.EFFECT_FACTOR * fc.PROX_TRAIN_TOL["param"])
    assert gap >= fc.EFFECT_FACTOR * fc.PROX_TRAIN_TOL["param"]

    got = fc.check_prox_train(
        "prox fused fnn(12,4) adam", inp, "adam",
        in_params=glob.to(DEV), model_of=model_of.to(torch.int32).to(DEV),
        sample_w=sw.to(DEV), partial=partial)
    # partial under the bound of test_fused_broadcast_and_partial: at most
    # 3 terms per model, one rounding of each product and of each sum
    reps = got[0][inp["rows"]].double()
    want = torch.zeros(K, P + 1, dtype=torch.float64)
    mag = torch.zeros(K, P + 1, dtype=torch.float64)
    s = sw.double()
    want.index_add_(0, model_of, torch.cat([s[:, None] * reps, s[:, None]],
                                           1))
    mag.index_add_(0, model_of, torch.cat([(s[:, None] * reps).abs(),
                                           s[:, None]], 1))
    part = partial.cpu().double()
    assert ((part - want).abs() <= 2 * 3 * 2.0 ** -24 * mag).all()
    assert (part[4] == 0).all()
    assert torch.equal(glob, inp["glob"])


# --------------------------------------------------------------------------
# cnn_opt_step, as a function of the gradient the kernel itself consumed
# --------------------------------------------------------------------------

CNN_LENS = np.array([(17, 64), (64, 1), (0, 16), (16, 0), (1, 1)],
                    dtype=np.int64)
BOTH = [0, 1, 4]              # pairs whose two steps both execute
ONE = [2, 3]                  # (0, 16) and (16, 0): one executed step
CNN_WD = 1e-3
# sgd: the pull of step 2 is lr * mu * |w1 - w0| = lr^2 * mu * |g1|, 1e-6 *
# |g1| at mu = 1 against a rounding slack of 2^-23 * |w| (2e-8): mu = 1
# misses the factor 10, so the sgd case runs at mu = 100 (lr * mu = 0.1)
CNN_MU = {"sgd": 100.0, "adam": 1.0}
# 1 - beta as cnn_opt_step forms them, in fp32
OMB1 = float(np.float32(1) - np.float32(0.9))
OMB2 = float(np.float32(1) - np.float32(0.999))


def _cnn_plan(E, seed=3):
    G = len(CNN_LENS)
    rng = np.random.default_rng(seed)
    off = rng.integers(0, vc.CNN_N - 64, (G, 2)).astype(np.int64)
    return TrainPlan(np.arange(G, dtype=np.int64), off[:, :E].copy(),
                     CNN_LENS[:, :E].copy(), np.ones((G, 1), np.float32))


def _cnn_run(eng, world, plan, optname, mu):
    G = len(plan.rows)
    reps = torch.zeros(G, world["P"], device=DEV)
    opt = eng.make_opt_state(optname, G, vc.CNN_LR,
                             CNN_WD if optname == "adam" else 0.0, mu=mu)
    eng.train(world["gp"].to(DEV), reps, plan, opt, world["x"].to(DEV),
              world["y"].to(DEV), world["K"])
    torch.cuda.synchronize()
    st = {k: v.cpu() for k, v in opt.items() if torch.is_tensor(v)}
    return reps.cpu(), st, eng._ws["grad"][:G].cpu()


def _same(a, b, sel=slice(None)):
    return torch.equal(a[0][sel], b[0][sel]) and all(
        torch.equal(a[1][k][sel], b[1][k][sel]) for k in a[1])


@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("O", [10, 62])
def test_cnn_opt_step(O, optname):
    """Dropout off, K = 2, G = 5, E = 2; P mod 4 = 2, so the scalar tail
    runs. The E = 1 run gives w1 and the Adam state after step 1, the
    workspace of the E = 2 run the gradient g2 that step 2 consumed.

    Adam: the parameters are asserted within 4 x err32 of the float64
    specification step (measured on an MI355X: 1.5e-8 against 7.0e-8 at
    O = 10, 1.3e-8 against 5.9e-8 at O = 62). cnn_opt_step forms 1 - beta
    as `1.f - 0.9f` / `1.f - 0.999f` (2.4e-7 and 1.3e-5 off the constants
    torch rounds from double), a quirk pinned by recorded baselines
    (PARITY.md, "Kernel edge and variant coverage") that this option leaves
    alone; against the specification's constants it puts m at 2.6-5.7 x
    and v at 60-120 x their err32 whatever mu is (recorded). So the stored
    m / v / vmax are asserted within 4 x err32 of the float64 step that
    uses the kernel's two constants, err32 being the fp32 form of that
    same step."""
    world = vc.cnn_world(O, K=2)
    assert world["P"] % 4 == 2
    mu = CNN_MU[optname]
    case = f"cnn opt step O={O} {optname} mu={mu:g}"
    eng = vc.cnn_engine(world)
    one = _cnn_run(eng, world, _cnn_plan(1), optname, mu)
    again = _cnn_run(eng, world, _cnn_plan(1), optname, mu)
    assert _same(one, again), "the pipeline has no float atomics"
    two = _cnn_run(eng, world, _cnn_plan(2), optname, mu)
    plain = _cnn_run(eng, world, _cnn_plan(2), optname, 0.0)
    g2 = two[2]
    # at most one executed step: the bits of mu = 0
    assert _same(two, plain, ONE), case
    assert torch.equal(one[0][2], world["gp"][0])        # (0, .): untouched
    if optname == "adam":
        assert two[1]["t"].tolist() == [2, 2, 1, 1, 2]

    w0 = world["gp"][torch.tensor(BOTH) % 2].double()
    w1 = one[0][BOTH].double()
    g = g2[BOTH].double()
    lr = torch.tensor(vc.CNN_LR, dtype=torch.float32).double()
    d = w1 - w0
    if optname == "sgd":
        gs = g + mu * d
        step = lr * gs
        want = w1 - step
        # one rounding each of w1 - w0, mu * d, g + mu * d (the first three
        # reach the weight times lr), lr * gs and w1 - step: 2^-23 x the
        # magnitude of every operand, as check_cnn_grads counts the plain
        # step's two
        slack = 2.0 ** -23 * (w1.abs() + step.abs()) + 1e-38 \
            + lr * 2.0 ** -23 * (mu * (w1.abs() + w0.abs())
                                 + 2 * mu * d.abs() + g.abs())
        err = (two[0][BOTH].double() - want).abs()
        eff = (lr * mu * d).abs().max().item()
        vc.record(case, "step / slack", None, (err / slack).max().item(),
                  1.0)
        vc.record(case, "effect of mu", None, eff,
                  fc.EFFECT_FACTOR * slack.max().item())
        assert eff >= fc.EFFECT_FACTOR * slack.max().item(), case
        assert (err <= slack).all(), (case, (err / slack).max())
    else:
        def spec_step(dtype, mu_):
            p = one[0][BOTH].to(dtype).clone()
            st = {k: one[1][k][BOTH].to(dtype).clone()
                  for k in ("m", "v", "vmax")}
            st["t"] = one[1]["t"][BOTH].clone()
            gr = g2[BOTH].to(dtype) + mu_ * (
                p - world["gp"][torch.tensor(BOTH) % 2].to(dtype))
            mlp_torch._apply_update(
                "adam", torch.full((len(BOTH),), vc.CNN_LR).to(dtype),
                CNN_WD, st, p, gr)
            return dict(st, param=p)
        s64, s32 = spec_step(torch.float64, mu), spec_step(torch.float32, mu)
        eff = (s64["param"] - spec_step(torch.float64, 0.0)["param"]) \
            .abs().max().item()
        got = dict(param=two[0][BOTH], m=two[1]["m"][BOTH],
                   v=two[1]["v"][BOTH], vmax=two[1]["vmax"][BOTH])
        figs = {}
        for q in ("param", "m", "v", "vmax"):
            e32 = (s32[q].double() - s64[q]).abs().max().item()
            ke = (got[q].double() - s64[q]).abs().max().item()
            figs[q] = (e32, ke)
            vc.record(case, q, e32, ke, 4 * e32)
        vc.record(case, "effect of mu", None, eff, fc.EFFECT_FACTOR * 4
                  * figs["param"][0])
        assert eff >= fc.EFFECT_FACTOR * 4 * figs["param"][0], case
        e32, ke = figs["param"]
        assert ke <= 4 * e32, (case, ke, e32)

        # the state the prox body stored: the same step with the kernel's
        # own 1 - beta (see the docstring), float64 against fp32
        def kernel_step(dtype):
            p = one[0][BOTH].to(dtype)
            m, v, vm = (one[1][k][BOTH].to(dtype) for k in ("m", "v", "vmax"))
            gr = g2[BOTH].to(dtype) + mu * (
                p - world["gp"][torch.tensor(BOTH) % 2].to(dtype))
            gr = gr + CNN_WD * p
            m = mlp_torch.ADAM_B1 * m + OMB1 * gr
            v = mlp_torch.ADAM_B2 * v + OMB2 * gr * gr
            return dict(m=m, v=v, vmax=torch.maximum(vm, v))
        k64, k32 = kernel_step(torch.float64), kernel_step(torch.float32)
        sfigs = {}
        for q in ("m", "v", "vmax"):
            e32 = (k32[q].double() - k64[q]).abs().max().item()
            ke = (got[q].double() - k64[q]).abs().max().item()
            sfigs[q] = (e32, ke)
            vc.record(case, q + " (kernel's 1 - beta)", e32, ke, 4 * e32)
        # mu is live in what was stored: without the pull, m ends elsewhere
        m_plain = plain[1]["m"][BOTH].double()
        assert (k64["m"] - m_plain).abs().max().item() \
            >= fc.EFFECT_FACTOR * 4 * sfigs["m"][0], case
        for q, (e32, ke) in sfigs.items():
            assert ke <= 4 * e32, (case, q, ke, e32)

    # chunked: one pair per chunk, the anchor found per chunk
    eng2 = vc.cnn_engine(world)
    eng2.WS_BUDGET = 1
    assert eng2._chunk_pairs(64) == 1
    chunked = _cnn_run(eng2, world, _cnn_plan(2), optname, mu)
    assert _same(two, chunked), case


# --------------------------------------------------------------------------
# FLJob
# --------------------------------------------------------------------------

def test_fljob_round_sea_fnn(tmp_path):
    """Rounds on the fused default path with mu = 0.1."""
    job = sc.make_job(tmp_path, secure_agg=0, use_hip_kernels="always",
                      fedprox_mu=0.1)
    assert job.device.type == "cuda" and job.backend is mlp_hip
    ci = job.client_sampling(0)
    K = job.n_models
    for r in range(2):
        prev = job.global_params.double().cpu().numpy().copy()
        plan, _, figs = fc.prox_round(job, "fljob hip mu=0.1", r, ci)
        assert figs["effect"] >= fc.EFFECT_FACTOR \
            * vc.ROUND_TRAIN_TOL["param"], figs
        mean, bound, has = sc.mean_and_bound_atomic(job.replicas,
                                                    plan.sample_num, K)
        job.algo.aggregate(job, r, plan, ci)
        torch.cuda.synchronize()
        gp = job.global_params.double().cpu().numpy()
        touched = 0
        for m in range(K):
            if not has[m] or np.array_equal(gp[m], prev[m]):
                continue
            touched += 1
            assert np.all(np.abs(gp[m] - mean[m]) <= bound[m]), (r, m)
        assert touched


def test_fljob_round_mnist_cnn(tmp_path):
    """One round of MNIST-shaped CNN_DropOut at 4 clients on CnnHipEngine,
    dropout off, against the eager float64 loop on the CPU under
    vc.ROUND_TRAIN_TOL["param"]. The optimizer is sgd: Adam's first step
    g / (|g| + eps) amplifies the fp32 rounding of gradients near eps by up
    to lr whatever mu is (tests/test_gpu_cnn.py bounds only its bulk).
    lr = 0.05 and mu = 10 (lr * mu = 0.5) make the pull lr^2 * mu * |g1|
    large against the bound (asserted)."""
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_mnist
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    from feddrift_amd.models.zoo import CNN_DropOut
    from feddrift_amd.ops.cnn_hip import CnnHipEngine
    n_clients, mu = 4, 10.0
    ds = DriftDataset(data_dir="/nonexistent", dataset="MNIST",
                      num_client=n_clients)
    rng = np.random.default_rng(0)
    for c in range(n_clients):
        for t in range(3):
            arr = sample_mnist(40, 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    cfg = Config(model="cnn", dataset="MNIST", data_dir="/nonexistent",
                 client_num_in_total=n_clients,
                 client_num_per_round=n_clients, batch_size=20, epochs=2,
                 comm_round=1, total_train_iteration=2,
                 curr_train_iteration=1, concept_num=2,
                 concept_drift_algo="softcluster",
                 concept_drift_algo_arg="mmacc_06", bench_mode=1,
                 report_client=0, log_dir=str(tmp_path),
                 client_optimizer="sgd", lr=0.05, fedprox_mu=mu)
    job = FLJob(cfg, Communicator(),
                MetricLogger(enabled=False, to_file=False), dataset=ds)
    assert isinstance(job.mod_engine, CnnHipEngine)
    job.mod_engine.dropout_override = (0.0, 0.0)
    assert job.opt["mu"] == mu
    K = job.n_models
    ci = job.client_sampling(0)
    plan = job.algo.plan(job, 0, ci)
    plan = TrainPlan(np.array(plan.rows, copy=True),
                     np.array(plan.step_off, copy=True),
                     np.array(plan.step_len, copy=True), plan.sample_num)
    assert (plan.step_len > 0).all() and len(plan.rows) >= n_clients
    glob0 = job.global_params.detach().cpu().clone()
    job.train(plan)
    torch.cuda.synchronize()
    got = job.replicas.detach().cpu()[plan.rows].double()

    def make():
        m = CNN_DropOut(only_digits=True)
        m.dropout_1.p = m.dropout_2.p = 0.0
        return m
    x, y = job.arena.x.cpu(), job.arena.y.cpu()
    lr = float(np.float32(cfg.lr))
    want = fc.eager_prox_round(make, job.packer, glob0, plan, x, y, K, "sgd",
                               lr, 0.0, mu)
    first = TrainPlan(plan.rows[:1], plan.step_off[:1], plan.step_len[:1],
                      plan.sample_num)
    plain = fc.eager_prox_round(make, job.packer, glob0, first, x, y, K,
                                "sgd", lr, 0.0, 0.0)
    err = (got - want).abs().max().item()
    eff = (want[:1] - plain).abs().max().item()
    tol = vc.ROUND_TRAIN_TOL["param"]
    vc.record("fljob hip cnn sgd mu=10", "param", None, err, tol)
    vc.record("fljob hip cnn sgd mu=10", "effect of mu", None, eff,
              fc.EFFECT_FACTOR * tol)
    assert eff >= fc.EFFECT_FACTOR * tol, eff
    assert err <= tol, err
