"""upload_compress=topk across processes (gloo): the rule has no index
tie-break and a pair's residual lives with its replica row, so what a worker
uploads and keeps does not depend on which rank owns it; with the median,
whose summation order is fixed, world 2 is bit-equal to world 1."""

import os
import subprocess
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# Two rounds with replicas that depend only on the global (worker, model)
# id and the round, so every world size trains the same values. Training
# runs plain and the compress pass is called on the rows written here.
_WORKER = r"""
import os, sys, pathlib
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
import torch
import secagg_cases as sc

job = sc.make_job(pathlib.Path({log!r}), device=torch.device("cpu"),
                  n_clients=10, robust_agg="median", upload_compress="topk",
                  compress_ratio=0.1, compress_error_feedback=1)
ci = job.client_sampling(0)
K, P = job.n_models, job.n_params
nW = len(job.owned_workers)
uploads, residuals, stats = [], [], []
for r in range(2):
    plan = job.algo.plan(job, r, ci)
    job._compress = False
    job.train(plan)
    job._compress = True
    for wi, w in enumerate(job.owned_workers):
        for m in range(K):
            g = torch.Generator().manual_seed(1000 + (r * 64 + w) * K + m)
            job.replicas[wi * K + m] = job.global_params[m] + \
                0.1 * torch.randn(P, generator=g)
            if w == 3 and m == 1:
                job.replicas[wi * K + m, 7] = float("inf")
    job._compress_pass(plan)
    uploads.append(job.replicas.numpy().reshape(nW, K, P).copy())
    residuals.append(job._residual.numpy().reshape(nW, K, P).copy())
    job.aggregate(plan)
    stats.append(job.compress_stats())
np.savez(os.path.join({log!r}, "rank%d.npz" % job.comm.rank),
         global_params=job.global_params.numpy(), uploads=np.stack(uploads),
         residuals=np.stack(residuals), stats=np.stack(stats),
         owned=np.asarray(job.owned_workers))
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


def _by_worker(ranks, name):
    """[round, worker, K, P] by global worker id."""
    out = {}
    for t in ranks:
        for wi, w in enumerate(t["owned"]):
            out[int(w)] = t[name][:, wi]
    return np.stack([out[w] for w in sorted(out)], axis=1)


def test_world2_is_bit_equal_to_world1(tmp_path):
    w1, w2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    _launch(1, w1, 29693)
    _launch(2, w2, 29694)
    one = [np.load(os.path.join(w1, "rank0.npz"))]
    two = [np.load(os.path.join(w2, f"rank{r}.npz")) for r in range(2)]
    assert np.array_equal(two[0]["owned"], np.arange(0, 10, 2))
    assert np.array_equal(two[1]["owned"], np.arange(1, 10, 2))
    for name in ("uploads", "residuals"):
        a, b = _by_worker(one, name), _by_worker(two, name)
        assert a.shape == b.shape and a.shape[:2] == (2, 10)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    g1 = one[0]["global_params"].view(np.uint32)
    for t in two:
        assert np.array_equal(t["global_params"].view(np.uint32), g1)
        assert np.array_equal(t["stats"], one[0]["stats"])
    # something was held back and carried, the Inf of worker 3 travelled
    # rather than staying in its residual, and about a tenth was sent
    res = _by_worker(one, "residuals")
    assert np.any(res[0] != 0) and np.all(np.isfinite(res))
    up = _by_worker(one, "uploads")
    assert np.isinf(up[:, 3, 1, 7]).all()
    stats = one[0]["stats"]                      # [round, K, 2]
    assert np.all(stats[:, :, 1] > 0)
    frac = stats[:, :, 0] / stats[:, :, 1]
    assert np.all((frac >= 0.1) & (frac < 0.2))
