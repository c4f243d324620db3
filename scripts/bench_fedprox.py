#!/usr/bin/env python3
"""Measurements of the FedProx option (`fedprox_mu`) on one GPU, written to
profiles/fedprox.json (each --part merges its own key into the file).

  bench     mu = 0 costs nothing: bench.py of a parent checkout (--parent
            DIR, built) and of this tree by turns, each run a fresh process;
            the change's median against the min-max spread of the parent's
            own runs, and --dump-outputs of both builds array for array.
  cost      mu = 0 against mu = 0.1 on the same build: full rounds (plan ->
            train -> aggregate) of bench.py's SEA-4 fnn shape at --fleets
            clients and of the config-3 CNN round (MNIST CNN_DropOut,
            FedDrift-Eager, 10 clients). Method of
            scripts/bench_robust_agg.py: warm-up, device synchronisation on
            both sides of the timed region, a round count from a probe, the
            two settings in one process timed by turns, twice each.
  compiler  hipcc's kernel-resource-usage remarks for the three train
            kernels of both trees (no GPU needed).
  generic   the generic mlp_train_kernel (not on bench.py's path) of the
            parent and of this tree: one train_fused launch of G pairs, E =
            5 Adam steps of 500 samples, on the three generic test shapes;
            fresh processes by turns, three each, mu-less.
  accuracy  mean Test/Acc over the canonical SEA-4 timeline (FedDrift
            H_A_C_1_10_0 and the single-model win-1 baseline, change points
            A) at mu in {0, 0.01, 0.1, 1}; a record, not a gate.
"""

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
# --tree DIR (the generic_child part): import feddrift_amd from that checkout
TREE = (os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
        if "--tree" in sys.argv else REPO)
sys.path.insert(0, TREE)
sys.path.insert(0, HERE)

MU = 0.1
KERNELS = ("mlp_train_kernel", "mlp_train_small_kernel", "cnn_opt_step",
           "cnn_opt_step_prox")


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def save(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


# ------------------------------------------------------------------- bench

def run_bench(tree, steps, warmup, dump=None):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
           "--steps", str(steps), "--warmup", str(warmup)]
    if dump:
        cmd += ["--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py of {tree} ended with {r.returncode}: "
                           + r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def part_bench(a):
    runs = {"parent": [], "change": []}
    key = "value"                   # fl_rounds_per_sec of bench.py's line
    for i in range(a.runs):
        for name, tree in (("parent", a.parent), ("change", REPO)):
            res = run_bench(tree, a.steps, a.warmup)
            res = {k: res[k] for k in ("metric", "value", "ms_per_step")}
            runs[name].append(res)
            print(i, name, json.dumps(res), flush=True)
    tmp = tempfile.mkdtemp(prefix="fedprox_dump_")
    same = {}
    dirs = {}
    for name, tree in (("parent", a.parent), ("change", REPO)):
        dirs[name] = os.path.join(tmp, name)
        run_bench(tree, a.steps, a.warmup, dump=dirs[name])
    for f in sorted(os.listdir(dirs["parent"])):
        x = np.load(os.path.join(dirs["parent"], f))
        y = np.load(os.path.join(dirs["change"], f))
        same[f] = bool(x.shape == y.shape and
                       np.array_equal(x.view(np.uint8), y.view(np.uint8)))
    shutil.rmtree(tmp, ignore_errors=True)
    out = {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup "
                      f"{a.warmup}", "runs_each": a.runs,
           "order": "parent, change, parent, change, ...",
           "results": runs, "dump_outputs_bit_identical": same}
    p = [r[key] for r in runs["parent"]]
    c = [r[key] for r in runs["change"]]
    out.update(metric="fl_rounds_per_sec", parent_min=min(p),
               parent_max=max(p), parent_median=float(np.median(p)),
               change_median=float(np.median(c)), change_min=min(c),
               change_max=max(c),
               change_median_inside_parent_spread=bool(
                   min(p) <= float(np.median(c)) <= max(p)),
               # (higher is better: above the parent's fastest run is
               # outside its spread on the harmless side)
               change_median_at_least_parent_min=bool(
                   float(np.median(c)) >= min(p)))
    return out


# -------------------------------------------------------------------- cost

def config3_cnn(comm):
    """-> (make(**cfg_kw) -> FLJob, n_clients, log_dir): the config-3 CNN
    round (MNIST CNN_DropOut, FedDrift-Eager, 10 clients, E = 5, batch 100)
    in its steady state."""
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_mnist
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    n = 10
    ds = DriftDataset(data_dir="/nonexistent", dataset="MNIST", num_client=n)
    rng = np.random.default_rng(0)
    for c in range(n):
        for t in range(5):
            arr = sample_mnist(200, (c % 4) if t >= 3 else 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    log_dir = tempfile.mkdtemp(prefix="fedprox_cnn_")

    def cnn(**kw):
        cfg = Config(model="cnn", dataset="MNIST", data_dir="/nonexistent",
                     client_num_in_total=n, client_num_per_round=n,
                     batch_size=100, lr=0.003, epochs=5, comm_round=10 ** 9,
                     total_train_iteration=4, curr_train_iteration=3,
                     concept_num=4, concept_drift_algo="softcluster",
                     concept_drift_algo_arg="mmacc_06", bench_mode=1,
                     log_dir=log_dir, report_client=0, **kw)
        return FLJob(cfg, comm, MetricLogger(enabled=False, to_file=False),
                     dataset=ds)
    return cnn, n, log_dir


def part_cnn_rounds(a):
    """--rounds config-3 CNN rounds at --mu and nothing else: the workload
    of a `rocprofv3 --kernel-trace --stats -- python ...` run of its own
    (scripts/rocpd_stats.py reads its database)."""
    import torch
    import bench_robust_agg as br
    from feddrift_amd.comm import Communicator
    comm = Communicator()
    cnn, n, log_dir = config3_cnn(comm)
    job = cnn(fedprox_mu=a.mu)
    br.timed(job, np.arange(n), 0, a.rounds)
    shutil.rmtree(log_dir, ignore_errors=True)
    return {"rounds": a.rounds, "mu": a.mu}


def part_cost(a):
    import torch
    import bench
    import bench_robust_agg as br
    from feddrift_amd.comm import Communicator
    comm = Communicator()

    def pair(make, n_clients):
        runners = {mu: br.Runner(make(fedprox_mu=mu), n_clients, a.seconds,
                                 a.max_rounds) for mu in (0.0, MU)}
        for _ in range(2):
            for mu in (0.0, MU):
                runners[mu].repeat()
        res = {f"mu={mu:g}": runners[mu].result() for mu in (0.0, MU)}
        res["ratio"] = round(res[f"mu={MU:g}"]["ms_per_round_mean"]
                             / res["mu=0"]["ms_per_round_mean"], 4)
        for k, v in res.items():
            if isinstance(v, dict):
                v["rounds_per_sec"] = round(1e3 / v["ms_per_round_mean"], 1)
        del runners
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return res

    out = {"device": (torch.cuda.get_device_name(0)
                      if comm.device.type == "cuda" else "cpu"),
           "method": "round = plan+train+aggregate; two repeats per setting, "
                     "settings timed by turns in one process; spread = "
                     "|a-b|/mean",
           "sea_fnn": {}, "mu": MU}
    for n in a.fleets:
        ds = bench.build_dataset(n, seed=1234)
        out["sea_fnn"][str(n)] = pair(
            lambda **kw: br.fnn_job(comm, ds, n, **kw), n)
        print(n, json.dumps(out["sea_fnn"][str(n)]), flush=True)
    if not a.skip_cnn:
        cnn, n, log_dir = config3_cnn(comm)
        out["config3_cnn"] = pair(cnn, n)
        out["config3_cnn"]["config"] = ("MNIST CNN_DropOut, softcluster "
                                        "mmacc_06, 10 clients, E=5, batch "
                                        "100")
        print("cnn", json.dumps(out["config3_cnn"]), flush=True)
        shutil.rmtree(log_dir, ignore_errors=True)
    return out


# ----------------------------------------------------------------- generic

GENERIC_SHAPES = (("fnn", 12, 4), ("fnn", 8, 5), ("lr", 4, 2))


def part_generic_child(a):
    """us per train_fused launch of the checkout named by --tree."""
    import time
    import torch
    import feddrift_amd
    from feddrift_amd.models.packed import spec_for
    from feddrift_amd.ops import mlp_hip, mlp_torch
    assert os.path.abspath(feddrift_amd.__file__).startswith(TREE)
    dev = torch.device("cuda:0")
    G, E, B, N = a.pairs, 5, 500, 20000
    out = {}
    for kind, d, o in GENERIC_SHAPES:
        spec = spec_for(kind, d, o)
        assert mlp_hip._fits_train(spec)
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(N, d, generator=g) * 10).to(dev)
        y = torch.randint(0, o, (N,), generator=g).to(dev)
        p0 = (torch.randn(G, spec.n_params, generator=g) * 0.4).to(dev)
        rows = torch.arange(G, device=dev)
        off = torch.randint(0, N - B, (G, E), generator=g).to(dev)
        ln = torch.full((G, E), B, device=dev)
        opt = mlp_torch.make_opt_state("adam", G, spec.n_params, 0.01, 1e-3,
                                       dev)
        params = p0.clone()

        def run(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                mlp_hip.train_fused(spec, params, rows, x, y, off, ln, opt)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6
        run(10)
        n = int(max(10, min(2000, a.seconds * 1e6 / max(run(10), 1.0))))
        out[f"{kind}({d},{o}) P={spec.n_params}"] = [round(run(n), 2),
                                                     round(run(n), 2)]
    return out


def part_generic(a):
    runs = {"parent": [], "change": []}
    for i in range(3):
        for name, tree in (("parent", a.parent), ("change", REPO)):
            r = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--part",
                 "generic_child", "--tree", tree, "--pairs", str(a.pairs),
                 "--seconds", str(a.seconds), "--out", os.devnull],
                capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: {r.returncode} "
                                   + r.stderr[-2000:])
            res = json.loads([ln for ln in r.stdout.splitlines()
                              if ln.startswith("{")][-1])
            runs[name].append(res)
            print(i, name, json.dumps(res), flush=True)
    out = {"what": f"us per train_fused launch (mlp_train_kernel), G = "
                   f"{a.pairs} pairs, E = 5 Adam steps x 500 samples, no "
                   "mu; fresh processes by turns, two timings each",
           "runs": runs, "median_us": {}, "ratio_change_over_parent": {}}
    for shape in runs["parent"][0]:
        med = {n: float(np.median([t for r in runs[n] for t in r[shape]]))
               for n in runs}
        out["median_us"][shape] = {n: round(v, 2) for n, v in med.items()}
        out["ratio_change_over_parent"][shape] = round(
            med["change"] / med["parent"], 4)
    return out


# ---------------------------------------------------------------- compiler

def resource_usage(tree):
    """{kernel: {VGPRs, SGPRs, scratch, occupancy, LDS, spills}} from
    hipcc's kernel-resource-usage remarks."""
    import sysconfig
    import torch.utils.cpp_extension as ce
    incs = ce.include_paths() + [sysconfig.get_paths()["include"],
                                 "/opt/rocm/include"]
    flags = ["-DWITH_HIP", "-DTORCH_EXTENSION_NAME=feddrift_hip",
             "-DTORCH_API_INCLUDE_EXTENSION_H", "-D__HIP_PLATFORM_AMD__=1",
             "-DUSE_ROCM=1", "-DHIPBLAS_V2", "-DCUDA_HAS_FP16=1",
             "-D__HIP_NO_HALF_OPERATORS__=1",
             "-D__HIP_NO_HALF_CONVERSIONS__=1",
             "-DHIP_ENABLE_WARP_SYNC_BUILTINS=1", "-std=c++17"]
    out = {}
    for src in ("feddrift_kernels.hip", "cnn_kernels.hip"):
        cmd = (["hipcc", "--offload-arch=gfx950", "--cuda-device-only",
                "-O3", "-S", "-Rpass-analysis=kernel-resource-usage", "-o",
                os.devnull] + flags + [f"-I{i}" for i in incs]
               + [os.path.join(tree, "feddrift_amd", "ops", "hip", src)])
        r = subprocess.run(cmd, capture_output=True, text=True, check=True)
        name = None
        for ln in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", ln)
            if m:
                name = m.group(1)
                dem = subprocess.run(["c++filt", name], capture_output=True,
                                     text=True).stdout.strip()
                name = dem if any(k in dem for k in KERNELS) else None
                if name:
                    name = re.sub(r"^void |\(TrainArgs\)|\(CnnArgs\)", "",
                                  name)
                    out[name] = {}
                continue
            if name is None:
                continue
            for key, pat in (("VGPRs", r" VGPRs: (\d+)"),
                             ("AGPRs", r" AGPRs: (\d+)"),
                             ("SGPRs", r" SGPRs: (\d+)"),
                             ("scratch_B", r"ScratchSize \[bytes/lane\]: "
                                           r"(\d+)"),
                             ("occupancy", r"Occupancy \[waves/SIMD\]: "
                                           r"(\d+)"),
                             ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                             ("vgpr_spill", r"VGPRs Spill: (\d+)"),
                             ("LDS_B", r"LDS Size \[bytes/block\]: (\d+)")):
                m = re.search(pat, ln)
                if m:
                    out[name][key] = int(m.group(1))
    return out


def part_compiler(a):
    return {"command": "hipcc --offload-arch=gfx950 --cuda-device-only -O3 "
                       "-S -Rpass-analysis=kernel-resource-usage",
            "parent": resource_usage(a.parent),
            "change": resource_usage(REPO)}


# ---------------------------------------------------------------- accuracy

def part_accuracy(a):
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import generate_data
    from feddrift_amd.engine.timeline import run_timeline
    comm = Communicator()
    out = {"metric": "mean Test/Acc over the timeline (10 iterations x "
                     f"{a.rounds} rounds), SEA-4, change points A",
           "seeds": list(range(a.seeds)), "runs": {}}
    for algo, arg in (("softcluster", "H_A_C_1_10_0"), ("single", "")):
        for mu in (0.0, 0.01, 0.1, 1.0):
            accs = []
            for seed in range(a.seeds):
                data_dir = tempfile.mkdtemp(prefix=f"fedprox_sea_{seed}_")
                cp = os.path.join(REPO, "data", "changepoints")
                os.makedirs(os.path.join(data_dir, "changepoints"))
                for f in os.listdir(cp):
                    if f.endswith(".cp"):
                        shutil.copy(os.path.join(cp, f),
                                    os.path.join(data_dir, "changepoints", f))
                np.random.seed(seed)
                generate_data("sea", data_dir, 10, 10, 0, 100, 0.0, 1, "A")
                log_dir = os.path.join(data_dir, "run")
                os.makedirs(log_dir)
                cfg = Config(model="fnn", dataset="sea", data_dir=data_dir,
                             client_num_in_total=10, client_num_per_round=10,
                             batch_size=500, lr=0.01, epochs=5,
                             comm_round=a.rounds, total_train_iteration=10,
                             concept_num=4, concept_drift_algo=algo,
                             concept_drift_algo_arg=arg, change_points="A",
                             dummy_arg=seed, sample_num=100, log_dir=log_dir,
                             report_client=0, fedprox_mu=mu)
                accs.append(round(run_timeline(cfg, comm)["avg_test_acc"],
                                  4))
                shutil.rmtree(data_dir, ignore_errors=True)
            out["runs"][f"{algo}:{arg} mu={mu:g}"] = {
                "values": accs, "mean": round(float(np.mean(accs)), 4)}
            print(algo, arg, mu, accs, flush=True)
            partial = load(a.out)           # keep what is done so far
            partial["accuracy"] = out
            save(a.out, partial)
    for name, key in (("seed_variance.json", "softcluster:H_A_C_1_10_0 mu=0"),
                      ("seed_variance_win1.json", "single: mu=0")):
        rec = load(os.path.join(REPO, "profiles", name)).get("values", [])
        out["runs"][key]["recorded_" + name] = rec[:a.seeds]
        out["runs"][key]["reproduces_record"] = \
            rec[:a.seeds] == out["runs"][key]["values"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", required=True,
                   choices=["bench", "cost", "compiler", "accuracy",
                            "generic", "generic_child", "cnn_rounds"])
    p.add_argument("--mu", type=float, default=0.0)
    p.add_argument("--tree", help="generic_child: checkout to import")
    p.add_argument("--pairs", type=int, default=3400)
    p.add_argument("--parent", help="built checkout of the parent commit")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--max-rounds", type=int, default=2000)
    p.add_argument("--fleets", type=int, nargs="+",
                   default=[10, 3400, 20000])
    p.add_argument("--skip-cnn", action="store_true")
    p.add_argument("--seeds", type=int, default=3)
    p.add_argument("--rounds", type=int, default=200)
    p.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                 "fedprox.json"))
    a = p.parse_args()
    if a.part in ("bench", "compiler", "generic") and not a.parent:
        p.error(f"--part {a.part} needs --parent DIR")
    if a.parent:
        a.parent = os.path.abspath(a.parent)
    res = {"bench": part_bench, "cost": part_cost,
           "compiler": part_compiler, "accuracy": part_accuracy,
           "generic": part_generic,
           "generic_child": part_generic_child,
           "cnn_rounds": part_cnn_rounds}[a.part](a)
    if a.part in ("generic_child", "cnn_rounds"):
        print(json.dumps(res))
        return
    out = load(a.out)
    out[{"bench": "mu0_costs_nothing", "cost": "cost_of_mu",
         "compiler": "compiler_view", "generic": "generic_kernel",
         "accuracy": "accuracy"}[a.part]] = res
    save(a.out, out)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
