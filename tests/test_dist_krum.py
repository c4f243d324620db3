"""robust_agg=multi_krum across processes (gloo): every rank gathers all
participant rows and their global worker ids (Communicator.all_gather_rows)
and computes the same selection; score ties go to the lower worker id and
the kept rows are added in (score, id) order, so the gather order cannot
matter and world 2 is bit-equal to world 1."""

import os
import subprocess
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# Two rounds with replicas that depend only on the global (worker, model)
# id and the round, so every world size uploads the same values.
_WORKER = r"""
import os, sys, pathlib
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
import torch
import secagg_cases as sc

job = sc.make_job(pathlib.Path({log!r}), device=torch.device("cpu"),
                  n_clients=10, robust_agg="multi_krum", robust_krum_frac=0.2,
                  robust_fused=1, robust_noise=1e-3, server_optimizer="adam",
                  server_lr=0.01)
ci = job.client_sampling(0)
K = job.n_models
totals, picked = [], []
for r in range(2):
    plan = job.algo.plan(job, r, ci)
    job.train(plan)
    for wi, w in enumerate(job.owned_workers):
        for m in range(K):
            g = torch.Generator().manual_seed(1000 + (r * 64 + w) * K + m)
            job.replicas[wi * K + m] = job.global_params[m] + \
                0.1 * torch.randn(job.n_params, generator=g)
            if w == 3 and m == 1:                     # a participant of 1
                job.replicas[wi * K + m] = float("nan")
    before = job.replicas.clone()
    totals.append(job.aggregate(plan).numpy().copy())
    sel = job.krum_selection()
    assert len(sel) == K
    picked.append(np.stack([np.pad(s, (0, 10 - len(s)), constant_values=-1)
                            for s in sel]))
    assert torch.equal(before.view(torch.int32),
                       job.replicas.view(torch.int32))
np.savez(os.path.join({log!r}, "rank%d.npz" % job.comm.rank),
         global_params=job.global_params.numpy(), totals=np.stack(totals),
         picked=np.stack(picked), owned=np.asarray(job.owned_workers))
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


def test_world2_is_bit_equal_to_world1(tmp_path):
    w1, w2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    _launch(1, w1, 29691)
    _launch(2, w2, 29692)
    one = np.load(os.path.join(w1, "rank0.npz"))
    two = [np.load(os.path.join(w2, f"rank{r}.npz")) for r in range(2)]
    assert np.array_equal(two[0]["owned"], np.arange(0, 10, 2))
    assert np.array_equal(two[1]["owned"], np.arange(1, 10, 2))
    g1 = one["global_params"].view(np.uint32)
    for t in two:
        assert np.array_equal(t["global_params"].view(np.uint32), g1)
        assert np.array_equal(t["totals"], one["totals"])
        assert np.array_equal(t["picked"], one["picked"])
    # worker 3's NaN row was left out in both rounds (n = 5, s = 4 on its
    # model), and the totals are the weight sums
    picked = one["picked"]                       # [round, model, 10]
    assert np.all((picked >= 0).sum(axis=2) == 4)
    assert not np.any(picked[:, 1] == 3)
    assert np.all(np.isfinite(one["global_params"]))
    assert np.all(one["totals"] > 0)
