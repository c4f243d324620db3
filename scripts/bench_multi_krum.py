#!/usr/bin/env python3
"""Cost of the Multi-Krum aggregation (robust_agg=multi_krum) on one GPU.

Part 1, the op alone: ops/hip/krum_kernels.hip against a torch float64
formulation of the same rule on the same device (written here only:
torch.cdist without the matrix-multiply shortcut, squared; topk of the
q + 1 smallest; argsort; index_select; mean), at three shapes: K = 10
models x 340 participants at P = 38 (the MLP fleet), one model of 10
participants at CNN_DropOut's packed size, and 2 models x 5,000 at P = 38
— the last under the default scratch bound (whole) and under
scratch_rows = 512 (ten passes).

Part 2, full rounds (plan -> train -> aggregate): bench.py's SEA-4 fnn
configuration at 3,400 clients and the FEMNIST-shaped CNN round of
scripts/bench_robust_agg.py, `mean` against `multi_krum`. The `mean` round
runs no code of this option.

Method (as scripts/bench_order_stat.py): warm-up, device synchronisation on
both sides of the timed region, an iteration count chosen from a short
probe so that the timed region lasts about --seconds, the compared things
in one process and timed by turns, twice each; `spread` is |a - b| / mean
of the two repeats. No ratio is fixed in advance: the figures are recorded
as they come.

Writes --out (default profiles/multi_krum.json, the committed record)."""

import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, ".."))
sys.path.insert(0, _HERE)

import bench
import bench_order_stat as bos
import bench_robust_agg as bra
from feddrift_amd.comm import Communicator
from feddrift_amd.ops import krum_hip

AGGS = {"mean": {}, "multi_krum": dict(robust_agg="multi_krum")}
FRAC = 0.2


def torch_multi_krum(bank, rows_by_model, qs, ss, out):
    """The same rule with library calls, distances and scores in float64."""
    for m, (rows, q, s) in enumerate(zip(rows_by_model, qs, ss)):
        x = bank[rows]
        xd = x.double()
        D = torch.cdist(xd, xd,
                        compute_mode="donot_use_mm_for_euclid_dist").square()
        D.fill_diagonal_(0.0)
        scores = torch.topk(D, q + 1, dim=1, largest=False).values.sum(dim=1)
        keep = torch.argsort(scores)[:s]
        out[m] = x.index_select(0, keep).mean(dim=0)


def measure_op(dev, K, n_per, P, seconds, scratch_rows=None):
    rng = np.random.default_rng(K * 1000 + n_per)
    U = K * n_per
    bank = torch.from_numpy(
        (rng.standard_normal((U, P)) * 0.3).astype(np.float32)).to(dev)
    rows = rng.permutation(U)
    models = np.repeat(np.arange(K), n_per)
    plan = krum_hip.KrumPlan(rows, models, np.ones(U, np.float32), K, FRAC)
    rows_by_model = [torch.as_tensor(plan.rows[plan.mod_off[m]:
                                               plan.mod_off[m + 1]],
                                     device=dev) for m in range(K)]
    qs, ss = [int(q) for q in plan.q], [int(s) for s in plan.s]
    out_k = torch.zeros(K, P, device=dev)
    out_t = torch.zeros(K, P, device=dev)
    fns = {"hip": lambda: krum_hip.aggregate(bank, plan, out_k,
                                             scratch_rows=scratch_rows),
           "torch_f64": lambda: torch_multi_krum(bank, rows_by_model, qs, ss,
                                                 out_t)}
    iters, reps = {}, {k: [] for k in fns}
    for name, fn in fns.items():
        bos.time_fn(fn, 3)                                  # warm-up
        probe = bos.time_fn(fn, 5)
        iters[name] = int(min(20000, max(5, seconds * 1e6 / probe)))
    for _ in range(2):
        for name, fn in fns.items():
            bos.time_fn(fn, max(1, iters[name] // 10))
            reps[name].append(bos.time_fn(fn, iters[name]))
    res = {"K": K, "participants_per_model": n_per, "P": P, "frac": FRAC,
           "f": int(plan.f[0]), "q": qs[0], "s": ss[0],
           "scratch_rows": scratch_rows or krum_hip.scratch_rows(),
           "passes": -(-n_per // plan._scratch[1]),
           "max_abs_diff": float((out_k - out_t).abs().max())}
    for name, (a, b) in reps.items():
        res[name] = {"iters": iters[name], "us": [round(a, 2), round(b, 2)],
                     "us_mean": round((a + b) / 2, 2),
                     "spread": round(abs(a - b) / ((a + b) / 2), 4)}
    res["hip_over_torch_f64"] = round(
        res["hip"]["us_mean"] / res["torch_f64"]["us_mean"], 3)
    return res


def measure_rounds(make, n_clients, seconds, max_rounds):
    runners = {name: bra.Runner(make(**kw), n_clients, seconds, max_rounds)
               for name, kw in AGGS.items()}
    for _ in range(2):
        for r in runners.values():
            r.repeat()
    res = {name: r.result() for name, r in runners.items()}
    res["multi_krum"]["overhead_over_mean_ms"] = round(
        res["multi_krum"]["ms_per_round_mean"]
        - res["mean"]["ms_per_round_mean"], 4)
    sel = runners["multi_krum"].job.krum_selection()
    res["multi_krum"]["kept_per_model"] = [len(s) for s in sel]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["op", "rounds", "both"], default="both")
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--max-rounds", type=int, default=2000)
    p.add_argument("--fleet", type=int, default=3400)
    p.add_argument("--cnn-clients", type=int, default=40)
    p.add_argument("--out", default=os.path.join(
        _HERE, "..", "profiles", "multi_krum.json"))
    a = p.parse_args()
    comm = Communicator()
    assert comm.device.type == "cuda", "this benchmark needs a GPU"
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["device"] = torch.cuda.get_device_name(0)
    out["method"] = ("warm-up, synchronise on both sides, iteration count "
                     "from a probe; compared things timed by turns in one "
                     "process, twice each; spread = |a-b|/mean")
    out["kernel"] = {"tile": krum_hip.tile(), "chunk": krum_hip.chunk(),
                     "score_lds": krum_hip.score_lds(),
                     "scratch_rows": krum_hip.scratch_rows(),
                     "selection": "bitwise bisection, 63 passes"}
    if a.part in ("op", "both"):
        from feddrift_amd.models import zoo
        from feddrift_amd.models.generic_packer import ModulePacker
        cnn_p = ModulePacker(zoo.CNN_DropOut()).n_params
        out["op"] = {}
        for shape, (K, n_per, P, sr) in (
                ("mlp_fleet", (10, 340, 38, None)),
                ("cnn_10", (1, 10, cnn_p, None)),
                ("large_n/whole", (2, 5000, 38, None)),
                ("large_n/scratch_rows_512", (2, 5000, 38, 512))):
            r = measure_op(comm.device, K, n_per, P, a.seconds, sr)
            out["op"][shape] = r
            print(shape, json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if a.part in ("rounds", "both"):
        n = a.fleet
        ds = bench.build_dataset(n, seed=1234)
        out["rounds"] = {"sea": {
            "config": "SEA-4 fnn(3-6-2), softcluster H_A_F_1_06_0, "
                      f"K={bench.N_MODELS}, E={bench.EPOCHS}, "
                      f"batch {bench.SEQ}, {n} clients",
            **measure_rounds(lambda **kw: bra.fnn_job(comm, ds, n, **kw), n,
                             a.seconds, a.max_rounds)}}
        print("sea", json.dumps(out["rounds"]["sea"]), flush=True)
        nc = a.cnn_clients
        cds = bra.cnn_dataset(nc)
        log_dir = tempfile.mkdtemp(prefix="krum_bench_")
        out["rounds"]["cnn"] = {
            "config": f"FEMNIST-shaped CNN_DropOut, aue, K=4, E=5, batch "
                      f"100, {nc} clients",
            **measure_rounds(lambda **kw: bra.cnn_job(comm, cds, nc, log_dir,
                                                      **kw), nc, a.seconds,
                             a.max_rounds)}
        print("cnn", json.dumps(out["rounds"]["cnn"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
