#!/usr/bin/env python3
"""Measurements of the quantised upload kinds (`upload_compress=quant`,
`topk_quant`) on one GPU, written to profiles/upload_quant.json (each --part
merges its own key into the file). Nothing here is a gate; the record is the
deliverable. The method and the helpers are those of
scripts/bench_upload_compress.py.

  cost      `none`, `topk` 0.1, `quant` at 8 bits and `topk_quant` 0.1 at
            4 bits, all with error feedback, on the same build: full rounds
            (plan -> train -> aggregate) of bench.py's SEA-4 fnn shape at
            --fleets clients and of the config-3 CNN round, and the compress
            pass alone on the job's own banks. The yardstick is `topk` and
            `none` of the parent build measured by its own
            scripts/bench_upload_compress.py in the same visit; the
            quantiser's extra cost over `topk` is reported, not targeted.
  accuracy  first-iteration and final Test/Acc and the logged WireFrac of
            the short SEA-4 FedDrift timeline of
            scripts/bench_upload_compress.py under `none`, `topk` 0.1,
            `quant` at 8, 4 and 2 bits and `topk_quant` 0.1 at 4 bits;
            recorded, not asserted. Any device: the arithmetic is the
            specification's on all of them.
"""

import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import bench_upload_compress as buc  # noqa: E402


def setting(kind, ratio=0.1, bits=8):
    return dict(upload_compress=kind, compress_ratio=ratio,
                compress_bits=bits, compress_error_feedback=1)


COST = [("none", {}),
        ("topk r=0.1", setting("topk")),
        ("quant b=8", setting("quant", bits=8)),
        ("topk_quant r=0.1 b=4", setting("topk_quant", bits=4))]
ACCURACY = COST[:3] + [("quant b=4", setting("quant", bits=4)),
                       ("quant b=2", setting("quant", bits=2)), COST[3]]


def part_cost(a):
    import torch
    import bench_robust_agg as br
    from feddrift_amd.comm import Communicator
    comm = Communicator()
    out = {"device": (torch.cuda.get_device_name(0)
                      if comm.device.type == "cuda" else "cpu"),
           "method": "round = plan+train+aggregate; two repeats per setting, "
                     "settings timed by turns in one process; pass alone = "
                     "the compress pass enqueued back to back on the job's "
                     "banks, synchronised around",
           "shapes": {}}
    shapes = [f"sea:{n}" for n in a.fleets] + \
        ([] if a.skip_cnn else ["config3_cnn"])
    for shape in shapes:
        make, n, cleanup = buc.make_shape(comm, shape)
        runners = {name: br.Runner(make(**kw), n, a.seconds, a.max_rounds)
                   for name, kw in COST}
        for _ in range(2):
            for name, _ in COST:
                runners[name].repeat()
        res = {}
        for name, kw in COST:
            job = runners[name].job
            r = runners[name].result()
            if kw:
                st = job.compress_stats()
                r["sent_fraction"] = round(
                    float(st[:, 0].sum()) / max(float(st[:, 1].sum()), 1), 5)
                wire = job._wire_stats(st)
                r["wire_fraction"] = round(
                    float(wire[:, 0].sum()) / max(float(wire[:, 1].sum()), 1),
                    5)
                alone = buc.pass_alone(job, a.seconds)
                if alone:
                    alone.update(P=job.n_params, k=job._compress_k)
                r["pass_alone"] = alone
            res[name] = r
        base = res["none"]["ms_per_round_mean"]
        for name in res:
            res[name]["ratio_to_none"] = round(
                res[name]["ms_per_round_mean"] / base, 4)
        out["shapes"][shape] = res
        print(shape, json.dumps(res), flush=True)
        partial = buc.load(a.out)                  # keep what is done so far
        partial["cost"] = out
        buc.save(a.out, partial)
        del runners
        cleanup()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    return out


def part_accuracy(a):
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import generate_data
    from feddrift_amd.engine.timeline import run_timeline
    comm = Communicator()
    out = {"metric": f"Test/Acc of a SEA-4 FedDrift timeline (H_A_C_1_10_0, "
                     f"change points A, {a.iters} iterations x {a.rounds} "
                     "rounds, 10 clients) and the mean logged "
                     "Compress/WireFrac; recorded, not asserted",
           "device": str(comm.device), "runs": {}}
    for name, kw in ACCURACY:
        data_dir = tempfile.mkdtemp(prefix="quant_sea_")
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
        wire = []
        metrics = os.path.join(log_dir, "metrics.jsonl")
        if os.path.exists(metrics):
            with open(metrics) as f:
                for line in f:
                    rec = json.loads(line)
                    wire += [v for k, v in rec.items()
                             if str(k).startswith("Compress/WireFrac")]
        out["runs"][name] = {
            "first_iteration_test_acc": per_iter[0],
            "final_iteration_test_acc": per_iter[-1],
            "avg_test_acc": round(float(res["avg_test_acc"]), 4),
            "per_iteration_test_acc": per_iter,
            "wire_fraction_mean": round(float(np.mean(wire)), 5)
            if wire else None}
        print(name, json.dumps(out["runs"][name]), flush=True)
        shutil.rmtree(data_dir, ignore_errors=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", required=True, choices=["cost", "accuracy"])
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--max-rounds", type=int, default=2000)
    p.add_argument("--fleets", type=int, nargs="+", default=[3400, 20000])
    p.add_argument("--skip-cnn", action="store_true")
    p.add_argument("--rounds", type=int, default=50)
    p.add_argument("--iters", type=int, default=4)
    p.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                 "upload_quant.json"))
    a = p.parse_args()
    res = {"cost": part_cost, "accuracy": part_accuracy}[a.part](a)
    out = buc.load(a.out)
    out[a.part] = res
    buc.save(a.out, out)
    print(json.dumps(res)[:2000])


if __name__ == "__main__":
    main()
