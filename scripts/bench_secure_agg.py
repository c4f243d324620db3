#!/usr/bin/env python3
"""Cost of secure aggregation on one GPU: full rounds (plan -> train ->
aggregate) of bench.py's SEA-4 fnn configuration at 10 and 3,400 clients
under secure_agg=0 and secure_agg=2 (mask graph degree 0 = complete, and
16), plus secure_agg=1 at 10 clients and at the largest fleet of a ladder
whose round still takes about a second — the mode that mode 2 replaces.

World 1 has only intra-rank pairs, which mode 2 skips by default; the
switch is cleared here so every pair mask is drawn and the figures are the
protocol's full cost.

Method: warm-up rounds, device synchronisation on both sides of the timed
region, and a round count chosen from a short probe so that the timed
region lasts about --seconds. The per-phase split comes from a second,
shorter pass that synchronises after every phase (PhaseTimer), so its sum
is a little above the unsynchronised round time.

Writes the result to --out (default profiles/secure_agg.json, the
committed record)."""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import bench
from feddrift_amd.comm import Communicator
from feddrift_amd.config import Config
from feddrift_amd.engine.fljob import FLJob
from feddrift_amd.engine.profiling import PhaseTimer
from feddrift_amd.eval.metrics import MetricLogger


def make_job(comm, ds, n_clients, secure, degree):
    cfg = Config(model="fnn", dataset="sea", data_dir="/nonexistent",
                 client_num_in_total=n_clients,
                 client_num_per_round=n_clients, batch_size=bench.SEQ,
                 client_optimizer="adam", lr=0.01, epochs=bench.EPOCHS,
                 comm_round=10 ** 9,
                 total_train_iteration=bench.CURR_ITER + 1,
                 curr_train_iteration=bench.CURR_ITER,
                 concept_num=bench.N_MODELS,
                 concept_drift_algo="softcluster",
                 concept_drift_algo_arg="H_A_F_1_06_0", change_points="A",
                 dummy_arg=0, report_client=0, bench_mode=1,
                 secure_agg=secure, secure_agg_degree=degree)
    job = FLJob(cfg, comm, MetricLogger(enabled=False, to_file=False),
                dataset=ds)
    job.secagg_skip_intra = False
    return job


def sync(job):
    if job.device.type == "cuda":
        torch.cuda.synchronize()


def one_round(job, r, idx, timer=None):
    if timer is None:
        plan = job.algo.plan(job, r, idx)
        job.train(plan)
        job.algo.aggregate(job, r, plan, idx)
        job.algo.post_aggregate(job, r)
        return
    with timer.phase("plan"):
        plan = job.algo.plan(job, r, idx)
    with timer.phase("train"):
        job.train(plan)
    with timer.phase("aggregate"):
        job.algo.aggregate(job, r, plan, idx)
        job.algo.post_aggregate(job, r)


def timed(job, idx, start, rounds):
    sync(job)
    t0 = time.perf_counter()
    for r in range(start, start + rounds):
        one_round(job, r, idx)
    sync(job)
    return time.perf_counter() - t0


def measure(job, n_clients, seconds, max_rounds):
    idx = np.arange(n_clients)
    timed(job, idx, 0, 3)                              # warm-up + caches
    probe = timed(job, idx, 3, 3) / 3
    rounds = int(min(max_rounds, max(5, seconds / max(probe, 1e-6))))
    timed(job, idx, 6, max(2, rounds // 10))           # warm-up proper
    dt = timed(job, idx, 6 + rounds, rounds)
    timer = PhaseTimer(sync_fn=lambda: sync(job))
    n_ph = max(3, rounds // 5)
    for r in range(n_ph):
        one_round(job, 10 ** 6 + r, idx, timer)
    job.check_secure_guard()
    return {"rounds": rounds, "timed_s": round(dt, 4),
            "ms_per_round": round(dt / rounds * 1e3, 4),
            "phase_avg_ms": {k: v["avg_ms"]
                             for k, v in timer.summary().items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seconds", type=float, default=2.0)
    p.add_argument("--max-rounds", type=int, default=4000)
    p.add_argument("--fleets", type=int, nargs="+", default=[10, 3400])
    p.add_argument("--mode1-ladder", type=int, nargs="+",
                   default=[10, 25, 50, 100, 200, 400, 800, 1600])
    p.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
        "secure_agg.json"))
    a = p.parse_args()
    comm = Communicator()
    out = {"device": (torch.cuda.get_device_name(0)
                      if comm.device.type == "cuda" else "cpu"),
           "config": "SEA-4 fnn(3-6-2), softcluster H_A_F_1_06_0, "
                     f"K={bench.N_MODELS}, E={bench.EPOCHS}, "
                     f"batch {bench.SEQ}; round = plan+train+aggregate",
           "fleets": {}, "mode1": {}}
    for n in a.fleets:
        ds = bench.build_dataset(n, seed=1234)
        res = {}
        for name, secure, degree in (("plain", 0, 0),
                                     ("ring_complete", 2, 0),
                                     ("ring_degree16", 2, 16)):
            job = make_job(comm, ds, n, secure, degree)
            res[name] = measure(job, n, a.seconds, a.max_rounds)
            print(n, name, json.dumps(res[name]), flush=True)
            del job
        base = res["plain"]["ms_per_round"]
        for name in ("ring_complete", "ring_degree16"):
            res[name]["ratio_to_plain"] = round(
                res[name]["ms_per_round"] / base, 3)
        out["fleets"][str(n)] = res
    # the mode this replaces: climb the ladder until a round passes ~1 s
    for n in a.mode1_ladder:
        ds = bench.build_dataset(n, seed=1234)
        job = make_job(comm, ds, n, 1, 0)
        idx = np.arange(n)
        timed(job, idx, 0, 1)
        per = timed(job, idx, 1, 2) / 2
        out["mode1"][str(n)] = {"ms_per_round": round(per * 1e3, 2)}
        print(n, "mode1", out["mode1"][str(n)], flush=True)
        del job
        if per > 1.0:
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
