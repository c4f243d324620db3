#!/usr/bin/env python3
"""Cost of the order-statistic aggregation (robust_agg) on one GPU.

Part 1, the op alone: ops/hip/orderstat_kernels.hip against a
torch.sort(dim=0) + slice + mean implementation of the same specification
on the same device (written here only), for `median` and `trimmed_mean 0.1`
at two shapes: K = 10 models x 340 participants at P = 38 (3,400 in all,
the MLP fleet), and one model of 10 participants at CNN_DropOut's packed
size.

Part 2, full rounds (plan -> train -> aggregate) of bench.py's SEA-4 fnn
configuration at 10 and 3,400 clients: `mean` against `trimmed_mean` and
`median`, with the per-phase split.

Method (as scripts/bench_robust_agg.py): warm-up, device synchronisation on
both sides of the timed region, an iteration count chosen from a short
probe so that the timed region lasts about --seconds, the compared things
in one process and timed by turns, twice each; `spread` is |a - b| / mean
of the two repeats. No ratio is fixed in advance: the figures are recorded
as they come.

Writes --out (default profiles/order_stat.json, the committed record)."""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, ".."))
sys.path.insert(0, _HERE)

import bench
import bench_robust_agg as bra
from feddrift_amd.comm import Communicator
from feddrift_amd.comm import robust as spec
from feddrift_amd.ops import orderstat_hip

AGGS = {"mean": {},
        "trimmed_mean": dict(robust_agg="trimmed_mean", robust_trim_frac=0.1),
        "median": dict(robust_agg="median")}


def torch_sort_stat(bank, rows_by_model, ks, out):
    """The same statistic with library calls: gather, sort every column,
    mean of the kept slice."""
    for m, (rows, k) in enumerate(zip(rows_by_model, ks)):
        srt = torch.sort(bank[rows], dim=0).values
        out[m] = srt[k:len(rows) - k].mean(dim=0)


def time_fn(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def measure_op(dev, K, n_per, P, kind, frac, seconds):
    rng = np.random.default_rng(K * 1000 + n_per)
    U = K * n_per
    bank = torch.from_numpy(
        (rng.standard_normal((U, P)) * 0.3).astype(np.float32)).to(dev)
    rows = rng.permutation(U)
    models = np.repeat(np.arange(K), n_per)
    plan = orderstat_hip.OrderStatPlan(rows, models, np.ones(U, np.float32),
                                       K, kind, frac)
    rows_by_model = [torch.as_tensor(plan.rows[plan.mod_off[m]:
                                               plan.mod_off[m + 1]],
                                     device=dev) for m in range(K)]
    ks = [int(k) for k in plan.k]
    out_k = torch.zeros(K, P, device=dev)
    out_t = torch.zeros(K, P, device=dev)
    fns = {"hip": lambda: orderstat_hip.aggregate(bank, plan, out_k),
           "torch_sort": lambda: torch_sort_stat(bank, rows_by_model, ks,
                                                 out_t)}
    iters, reps = {}, {k: [] for k in fns}
    for name, fn in fns.items():
        time_fn(fn, 3)                                      # warm-up
        probe = time_fn(fn, 5)
        iters[name] = int(min(20000, max(5, seconds * 1e6 / probe)))
    for _ in range(2):
        for name, fn in fns.items():
            time_fn(fn, max(1, iters[name] // 10))
            reps[name].append(time_fn(fn, iters[name]))
    res = {"K": K, "participants_per_model": n_per, "P": P, "kind": kind,
           "frac": frac, "k": ks[0],
           "max_abs_diff": float((out_k - out_t).abs().max())}
    for name, (a, b) in reps.items():
        res[name] = {"iters": iters[name], "us": [round(a, 2), round(b, 2)],
                     "us_mean": round((a + b) / 2, 2),
                     "spread": round(abs(a - b) / ((a + b) / 2), 4)}
    res["hip_over_torch_sort"] = round(
        res["hip"]["us_mean"] / res["torch_sort"]["us_mean"], 3)
    return res


def measure_rounds(comm, n_clients, seconds, max_rounds):
    ds = bench.build_dataset(n_clients, seed=1234)
    runners = {name: bra.Runner(bra.fnn_job(comm, ds, n_clients, **kw),
                                n_clients, seconds, max_rounds)
               for name, kw in AGGS.items()}
    for _ in range(2):
        for r in runners.values():
            r.repeat()
    res = {name: r.result() for name, r in runners.items()}
    base = res["mean"]["ms_per_round_mean"]
    for name in ("trimmed_mean", "median"):
        res[name]["overhead_over_mean_ms"] = round(
            res[name]["ms_per_round_mean"] - base, 4)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["op", "rounds", "both"], default="both")
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--max-rounds", type=int, default=2000)
    p.add_argument("--fleets", type=int, nargs="+", default=[10, 3400])
    p.add_argument("--out", default=os.path.join(
        _HERE, "..", "profiles", "order_stat.json"))
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
    out["kernel"] = {"tile": orderstat_hip.tile(),
                     "lds_rows": orderstat_hip.lds_rows(),
                     "selection": "bitwise bisection, 32 passes"}
    if a.part in ("op", "both"):
        from feddrift_amd.models import zoo
        from feddrift_amd.models.generic_packer import ModulePacker
        cnn_p = ModulePacker(zoo.CNN_DropOut()).n_params
        out["op"] = {}
        for shape, (K, n_per, P) in (("mlp_fleet", (10, 340, 38)),
                                     ("cnn_10", (1, 10, cnn_p))):
            for kind, frac in (("median", 0.0), ("trimmed_mean", 0.1)):
                r = measure_op(comm.device, K, n_per, P, kind, frac,
                               a.seconds)
                assert spec.trim_count(kind, frac, n_per) == r["k"]
                out["op"][f"{shape}/{kind}"] = r
                print(shape, kind, json.dumps(r), flush=True)
    if a.part in ("rounds", "both"):
        out["rounds"] = {
            "config": "SEA-4 fnn(3-6-2), softcluster H_A_F_1_06_0, "
                      f"K={bench.N_MODELS}, E={bench.EPOCHS}, "
                      f"batch {bench.SEQ}", "fleets": {}}
        for n in a.fleets:
            out["rounds"]["fleets"][str(n)] = measure_rounds(
                comm, n, a.seconds, a.max_rounds)
            print(n, json.dumps(out["rounds"]["fleets"][str(n)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
