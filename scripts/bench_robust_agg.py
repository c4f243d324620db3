#!/usr/bin/env python3
"""Cost of the defended aggregation on one GPU: full rounds (plan -> train
-> aggregate) with no defence, with clipping, and with clipping + noise +
the adam server optimizer, each defence under robust_fused=0 (the torch
path) and robust_fused=1 (ops/hip/robust_kernels.hip).

Run A: bench.py's SEA-4 fnn configuration at 10 and 3,400 clients.
Run B: the CNN configuration (femnist, CNN_DropOut, aue) at the largest
fleet of a short ladder whose torch-path round still fits in memory and
takes about a second.

Method (as scripts/bench_secure_agg.py): warm-up rounds, device
synchronisation on both sides of the timed region, a round count chosen
from a short probe so that the timed region lasts about --seconds, and the
per-phase split from a second pass that synchronises after every phase. The
two engines of one defence live in the same process and are timed by
turns, twice each; `spread` is |a - b| / mean of the two repeats.

Writes the result to --out (default profiles/robust_fused.json, the
committed record); --run A or B measures one half and merges it in."""

import argparse
import json
import os
import sys
import tempfile
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

BOUND = 0.05
DEFENCES = {
    "none": {},
    "clip": dict(robust_norm_bound=BOUND),
    "clip_noise_adam": dict(robust_norm_bound=BOUND, robust_noise=1e-3,
                            server_optimizer="adam", server_lr=0.01),
}


def fnn_job(comm, ds, n_clients, **kw):
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
                 dummy_arg=0, report_client=0, bench_mode=1, **kw)
    return FLJob(cfg, comm, MetricLogger(enabled=False, to_file=False),
                 dataset=ds)


def cnn_dataset(n_clients):
    from feddrift_amd.data.generators import sample_femnist
    from feddrift_amd.data.loader import DriftDataset
    ds = DriftDataset(data_dir="/nonexistent", dataset="femnist",
                      num_client=n_clients)
    rng = np.random.default_rng(0)
    for c in range(n_clients):
        for t in range(3):
            arr = sample_femnist(100, c % 4 if t >= 1 else 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    return ds


def cnn_job(comm, ds, n_clients, log_dir, **kw):
    cfg = Config(model="cnn", dataset="femnist", data_dir="/nonexistent",
                 client_num_in_total=n_clients,
                 client_num_per_round=n_clients, batch_size=100, lr=0.003,
                 epochs=5, comm_round=10 ** 9, total_train_iteration=3,
                 curr_train_iteration=1, concept_num=4, ensemble_window=4,
                 concept_drift_algo="aue", log_dir=log_dir, report_client=0,
                 **kw)
    from feddrift_amd.engine.timeline import clean_state_files
    clean_state_files(cfg)
    return FLJob(cfg, comm, MetricLogger(enabled=False, to_file=False),
                 dataset=ds)


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


class Runner:
    """One job's measurement state: warm-up and probe once, then repeats."""

    def __init__(self, job, n_clients, seconds, max_rounds):
        self.job, self.idx = job, np.arange(n_clients)
        timed(job, self.idx, 0, 3)                         # warm-up + caches
        probe = timed(job, self.idx, 3, 3) / 3
        self.rounds = int(min(max_rounds,
                              max(3, seconds / max(probe, 1e-6))))
        self.next = 6
        self.repeats = []

    def repeat(self):
        job, idx = self.job, self.idx
        timed(job, idx, self.next, max(1, self.rounds // 10))
        self.next += max(1, self.rounds // 10)
        dt = timed(job, idx, self.next, self.rounds)
        self.next += self.rounds
        self.repeats.append(dt / self.rounds * 1e3)

    def result(self):
        job = self.job
        timer = PhaseTimer(sync_fn=lambda: sync(job))
        for r in range(max(3, self.rounds // 5)):
            one_round(job, 10 ** 6 + r, self.idx, timer)
        a, b = self.repeats
        out = {"rounds": self.rounds,
               "ms_per_round": [round(a, 4), round(b, 4)],
               "ms_per_round_mean": round((a + b) / 2, 4),
               "spread": round(abs(a - b) / ((a + b) / 2), 4),
               "phase_avg_ms": {k: v["avg_ms"]
                                for k, v in timer.summary().items()}}
        if job.cfg.robust_fused and job.cfg.robust_norm_bound > 0:
            st = job.clip_stats()
            out["clip_fraction"] = round(
                float(st[:, 0].sum()) / max(float(st[:, 1].sum()), 1.0), 4)
        return out


def measure_fleet(make, n_clients, seconds, max_rounds):
    """make(**cfg_kw) -> FLJob. Every defence under both engines, timed by
    turns; an allocation failure is recorded as the finding."""
    res = {}
    for name, kw in DEFENCES.items():
        runners = {}
        try:
            for fused in (0, 1):
                runners[fused] = Runner(make(robust_fused=fused, **kw),
                                        n_clients, seconds, max_rounds)
            for _ in range(2):
                for fused in (0, 1):
                    runners[fused].repeat()
            for fused in (0, 1):
                res[f"{name}/fused{fused}"] = runners[fused].result()
        except torch.OutOfMemoryError as e:
            failed = 1 if 0 in runners else 0
            res[f"{name}/fused{failed}"] = {"error": "out of memory",
                                            "detail": str(e)[:200]}
        for fused in (0, 1):
            print(n_clients, name, fused,
                  json.dumps(res.get(f"{name}/fused{fused}")), flush=True)
        del runners
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    base = res.get("none/fused0", {}).get("ms_per_round_mean")
    for name in ("clip", "clip_noise_adam"):
        r0, r1 = res.get(f"{name}/fused0", {}), res.get(f"{name}/fused1", {})
        if "ms_per_round_mean" in r0 and "ms_per_round_mean" in r1:
            r1["ratio_to_fused0"] = round(
                r1["ms_per_round_mean"] / r0["ms_per_round_mean"], 3)
        for r in (r0, r1):
            if base and "ms_per_round_mean" in r:
                r["overhead_over_none_ms"] = round(
                    r["ms_per_round_mean"] - base, 4)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", choices=["A", "B", "AB"], default="AB")
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--max-rounds", type=int, default=2000)
    p.add_argument("--fleets", type=int, nargs="+", default=[10, 3400])
    p.add_argument("--cnn-ladder", type=int, nargs="+",
                   default=[50, 100, 200, 400, 800])
    p.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
        "robust_fused.json"))
    a = p.parse_args()
    comm = Communicator()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["device"] = (torch.cuda.get_device_name(0)
                     if comm.device.type == "cuda" else "cpu")
    out["defences"] = {k: dict(v) for k, v in DEFENCES.items()}
    out["method"] = ("round = plan+train+aggregate; two repeats per engine, "
                     "engines timed by turns in one process; spread = "
                     "|a-b|/mean")
    if "A" in a.run:
        out["run_A"] = {
            "config": "SEA-4 fnn(3-6-2), softcluster H_A_F_1_06_0, "
                      f"K={bench.N_MODELS}, E={bench.EPOCHS}, "
                      f"batch {bench.SEQ}", "fleets": {}}
        for n in a.fleets:
            ds = bench.build_dataset(n, seed=1234)
            out["run_A"]["fleets"][str(n)] = measure_fleet(
                lambda **kw: fnn_job(comm, ds, n, **kw), n, a.seconds,
                a.max_rounds)
    if "B" in a.run:
        log_dir = tempfile.mkdtemp(prefix="robust_bench_")
        ladder, chosen, ds = {}, None, None
        # climb until the torch-path clip round passes ~1 s or fails to fit
        for n in a.cnn_ladder:
            ds_n = cnn_dataset(n)
            try:
                job = cnn_job(comm, ds_n, n, log_dir, robust_fused=0,
                              robust_norm_bound=BOUND)
                idx = np.arange(n)
                timed(job, idx, 0, 1)
                per = timed(job, idx, 1, 2) / 2
                ladder[str(n)] = {
                    "ms_per_round": round(per * 1e3, 2),
                    "hbm_gib": round(torch.cuda.max_memory_allocated()
                                     / 2 ** 30, 2)
                    if comm.device.type == "cuda" else None}
                del job
            except torch.OutOfMemoryError as e:
                ladder[str(n)] = {"error": "out of memory",
                                  "detail": str(e)[:200]}
                break
            finally:
                if torch.cuda.is_available():
                    torch.cuda.empty_cache()
            print(n, "cnn ladder", ladder[str(n)], flush=True)
            chosen, ds = n, ds_n
            if per > 1.0:
                break
        out["run_B"] = {
            "config": "femnist CNN_DropOut, aue, K<=4, E=5, batch 100",
            "ladder_fused0_clip": ladder, "fleet": chosen}
        if chosen is not None:
            out["run_B"]["result"] = measure_fleet(
                lambda **kw: cnn_job(comm, ds, chosen, log_dir, **kw),
                chosen, a.seconds, a.max_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
