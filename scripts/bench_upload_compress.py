#!/usr/bin/env python3
"""Measurements of upload compression (`upload_compress=topk`) on one GPU,
written to profiles/upload_compress.json (each --part merges its own key
into the file). Nothing here is a gate; the record is the deliverable.

  cost      `none` against `topk` at ratio 0.01 and 0.1, with and without
            error feedback, on the same build: full rounds (plan -> train ->
            aggregate) of bench.py's SEA-4 fnn shape at --fleets clients and
            of the config-3 CNN round (the shapes of scripts/bench_fedprox.py).
            Method of scripts/bench_robust_agg.py: warm-up, device
            synchronisation on both sides of the timed region, a round count
            from a probe, all settings in one process timed by turns, twice
            each, the spread reported. For every shape also: the compress
            pass alone on the job's own banks (enqueued back to back,
            synchronised around), the bytes the pass must move, computed
            from the shapes, and the share of the HBM peak that time gives.
  rounds    --rounds rounds of one shape and setting and nothing else: the
            workload of a `rocprofv3 --kernel-trace --stats -- python ...`
            run of its own.
  kernels   read that run's database (--db) with scripts/rocpd_stats.py's
            query, keep the compress kernels, and set their summed time per
            pass against the bytes of the shape.
  accuracy  final Test/Acc of a short SEA-4 FedDrift timeline under `none`,
            `topk` 0.1 with error feedback and `topk` 0.1 without; recorded,
            not asserted.
"""

import argparse
import json
import os
import shutil
import sqlite3
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

# HBM3E peak of the MI355X (spec) and what a float4 copy reaches
HBM_PEAK_TBS = 8.0
HBM_COPY_TBS = 6.29

SETTINGS = [("none", {})] + [
    (f"topk r={r:g} ef={ef}",
     dict(upload_compress="topk", compress_ratio=r,
          compress_error_feedback=ef))
    for r in (0.01, 0.1) for ef in (1, 0)]


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def save(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def pass_bytes(pairs, P, K, ef):
    """Bytes one pass must move at the least: every pair's row read and
    written once, its residual row read and written once with error
    feedback, the K global rows read once."""
    per_row = 4 * P * (4 if ef else 2)
    return pairs * per_row + 4 * K * P


def make_shape(comm, shape):
    """-> (make(**cfg_kw) -> FLJob, n_clients, cleanup)."""
    import bench
    import bench_fedprox as bf
    import bench_robust_agg as br
    kind, _, n = shape.partition(":")
    if kind == "sea":
        n = int(n)
        ds = bench.build_dataset(n, seed=1234)
        return (lambda **kw: br.fnn_job(comm, ds, n, **kw)), n, lambda: None
    cnn, n, log_dir = bf.config3_cnn(comm)
    return cnn, n, lambda: shutil.rmtree(log_dir, ignore_errors=True)


def pass_alone(job, seconds):
    """us per compress pass on the job's banks and last plan, steady state."""
    import torch
    import bench_robust_agg as br
    idx = np.arange(job.cfg.client_num_per_round)
    plan = job.algo.plan(job, 10 ** 7, idx)
    if plan.rows.size == 0:
        return None

    def run(n):
        br.sync(job)
        t0 = time.perf_counter()
        for _ in range(n):
            job._compress_pass(plan)
        br.sync(job)
        return (time.perf_counter() - t0) / n * 1e6
    run(3)
    n = int(max(5, min(2000, seconds * 1e6 / max(run(5), 1.0))))
    us = [round(run(n), 2), round(run(n), 2)]
    job.compress_stats()
    return {"pairs": int(plan.rows.size), "calls": n, "us_per_pass": us}


def part_cost(a):
    import torch
    import bench_robust_agg as br
    from feddrift_amd.comm import Communicator
    comm = Communicator()
    out = {"device": (torch.cuda.get_device_name(0)
                      if comm.device.type == "cuda" else "cpu"),
           "method": "round = plan+train+aggregate; two repeats per setting, "
                     "settings timed by turns in one process; spread = "
                     "|a-b|/mean; pass alone = the compress pass enqueued "
                     "back to back on the job's banks, synchronised around",
           "hbm_peak_TBs": HBM_PEAK_TBS, "hbm_float4_copy_TBs": HBM_COPY_TBS,
           "shapes": {}}
    shapes = [f"sea:{n}" for n in a.fleets] + \
        ([] if a.skip_cnn else ["config3_cnn"])
    for shape in shapes:
        make, n, cleanup = make_shape(comm, shape)
        runners = {}
        for name, kw in SETTINGS:
            runners[name] = br.Runner(make(**kw), n, a.seconds, a.max_rounds)
        for _ in range(2):
            for name, _ in SETTINGS:
                runners[name].repeat()
        res = {}
        for name, kw in SETTINGS:
            job = runners[name].job
            r = runners[name].result()
            r["ratio_to_none"] = None
            if kw:
                st = job.compress_stats()
                r["sent_fraction"] = round(
                    float(st[:, 0].sum()) / max(float(st[:, 1].sum()), 1), 5)
                alone = pass_alone(job, a.seconds)
                if alone:
                    ef = kw["compress_error_feedback"]
                    nbytes = pass_bytes(alone["pairs"], job.n_params,
                                        job.n_models, ef)
                    tbs = nbytes / (min(alone["us_per_pass"]) * 1e-6) / 1e12
                    alone.update(
                        P=job.n_params, k=job._compress_k,
                        bytes_min=nbytes, achieved_TBs=round(tbs, 4),
                        share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 4))
                r["pass_alone"] = alone
            res[name] = r
        base = res["none"]["ms_per_round_mean"]
        for name in res:
            res[name]["ratio_to_none"] = round(
                res[name]["ms_per_round_mean"] / base, 4)
        out["shapes"][shape] = res
        print(shape, json.dumps(res), flush=True)
        partial = load(a.out)                  # keep what is done so far
        partial["cost"] = out
        save(a.out, partial)
        del runners
        cleanup()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    return out


def part_rounds(a):
    import bench_robust_agg as br
    from feddrift_amd.comm import Communicator
    comm = Communicator()
    make, n, cleanup = make_shape(comm, a.shape)
    kw = {} if a.ratio <= 0 else dict(
        upload_compress="topk", compress_ratio=a.ratio,
        compress_error_feedback=a.ef)
    job = make(**kw)
    br.timed(job, np.arange(n), 0, a.rounds)
    info = {"rounds": a.rounds, "P": job.n_params, "K": job.n_models}
    if kw:
        st = job.compress_stats()
        info["pairs_per_round"] = float(st[:, 1].sum()) / job.n_params \
            / a.rounds
    cleanup()
    prev = load(a.out).get("rounds", {})
    prev[f"{a.shape} r={a.ratio:g} ef={a.ef}"] = info
    return prev


def part_kernels(a):
    con = sqlite3.connect(a.db)
    tabs = [r[0] for r in con.execute(
        "SELECT name FROM sqlite_master WHERE type='table' "
        "AND name LIKE 'rocpd_kernel_dispatch%'")]
    kernels = {}
    for t in tabs:
        sfx = t[len("rocpd_kernel_dispatch_"):]
        for name, calls, total_ms, avg_us in con.execute(
                f"SELECT ks.kernel_name, COUNT(*), SUM(k.end-k.start)/1e6, "
                f"AVG(k.end-k.start)/1e3 "
                f"FROM rocpd_kernel_dispatch_{sfx} k "
                f"JOIN rocpd_info_kernel_symbol_{sfx} ks "
                f"ON k.kernel_id=ks.id GROUP BY ks.kernel_name"):
            if "compress_" in name or "robust_" in name or "train" in name:
                kernels[name[:60]] = {"calls": calls,
                                      "total_ms": round(total_ms, 3),
                                      "avg_us": round(avg_us, 2)}
    rec = {"rounds": a.rounds, "ratio": a.ratio, "ef": a.ef,
           "kernels": kernels}
    per_pass = sum(v["total_ms"] for k, v in kernels.items()
                   if "compress_" in k) * 1e3 / max(a.rounds, 1)
    rec["compress_us_per_round"] = round(per_pass, 2)
    info = load(a.out).get("rounds", {}).get(
        f"{a.shape} r={a.ratio:g} ef={a.ef}", {})
    pairs = a.pairs or info.get("pairs_per_round", 0)
    params, models = info.get("P", a.params), info.get("K", a.models)
    rec["pairs_per_round"] = pairs
    if pairs and params and per_pass > 0:
        nbytes = int(pass_bytes(pairs, params, models, a.ef))
        tbs = nbytes / (per_pass * 1e-6) / 1e12
        rec.update(bytes_min=nbytes, achieved_TBs=round(tbs, 4),
                   share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 4))
    prev = load(a.out).get("kernels", {})
    prev[f"{a.shape} r={a.ratio:g} ef={a.ef}"] = rec
    return prev


def part_accuracy(a):
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import generate_data
    from feddrift_amd.engine.timeline import run_timeline
    comm = Communicator()
    out = {"metric": f"Test/Acc of a SEA-4 FedDrift timeline (H_A_C_1_10_0, "
                     f"change points A, {a.iters} iterations x {a.rounds} "
                     "rounds, 10 clients); recorded, not asserted",
           "runs": {}}
    for name, kw in (SETTINGS[0], SETTINGS[3], SETTINGS[4]):
        data_dir = tempfile.mkdtemp(prefix="compress_sea_")
        cp = os.path.join(REPO, "data", "changepoints")
        os.makedirs(os.path.join(data_dir, "changepoints"))
        for f in os.listdir(cp):
            if f.endswith(".cp"):
                shutil.copy(os.path.join(cp, f),
                            os.path.join(data_dir, "changepoints", f))
        np.random.seed(0)
        generate_data("sea", data_dir, a.iters, 10, 0, 100, 0.0, 1, "A")
        log_dir = os.path.join(data_dir, "run")
        os.makedirs(log_dir)
        cfg = Config(model="fnn", dataset="sea", data_dir=data_dir,
                     client_num_in_total=10, client_num_per_round=10,
                     batch_size=500, lr=0.01, epochs=5, comm_round=a.rounds,
                     total_train_iteration=a.iters, concept_num=4,
                     concept_drift_algo="softcluster",
                     concept_drift_algo_arg="H_A_C_1_10_0", change_points="A",
                     dummy_arg=0, sample_num=100, log_dir=log_dir,
                     report_client=0, **kw)
        res = run_timeline(cfg, comm)
        per_iter = [round(float(v), 4)
                    for v in res["per_iteration_test_acc"]]
        out["runs"][name] = {
            "final_iteration_test_acc": per_iter[-1],
            "avg_test_acc": round(float(res["avg_test_acc"]), 4),
            "per_iteration_test_acc": per_iter}
        print(name, json.dumps(out["runs"][name]), flush=True)
        shutil.rmtree(data_dir, ignore_errors=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", required=True,
                   choices=["cost", "rounds", "kernels", "accuracy"])
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--max-rounds", type=int, default=2000)
    p.add_argument("--fleets", type=int, nargs="+",
                   default=[10, 3400, 20000])
    p.add_argument("--skip-cnn", action="store_true")
    p.add_argument("--shape", default="sea:3400",
                   help="rounds / kernels: sea:N or config3_cnn")
    p.add_argument("--ratio", type=float, default=0.1,
                   help="rounds / kernels: 0 = upload_compress none")
    p.add_argument("--ef", type=int, default=1)
    p.add_argument("--rounds", type=int, default=50)
    p.add_argument("--iters", type=int, default=4)
    p.add_argument("--db", help="kernels: the rocprofv3 database")
    p.add_argument("--pairs", type=int, default=0,
                   help="kernels: trained pairs per round of the shape")
    p.add_argument("--params", type=int, default=0)
    p.add_argument("--models", type=int, default=4)
    p.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                 "upload_compress.json"))
    a = p.parse_args()
    res = {"cost": part_cost, "rounds": part_rounds, "kernels": part_kernels,
           "accuracy": part_accuracy}[a.part](a)
    if res is not None:
        out = load(a.out)
        out[a.part] = res
        save(a.out, out)
        print(json.dumps(res)[:2000])


if __name__ == "__main__":
    main()
