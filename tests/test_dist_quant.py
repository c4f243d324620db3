"""upload_compress=topk_quant across processes (gloo): the scale is an
integer maximum, the draws are keyed by the GLOBAL worker id and every rank
advances the compress-pass counter once per pass, trained rows or not; so
what a worker uploads and keeps does not depend on which rank owns it, and
with the median, whose summation order is fixed, world 2 is bit-equal to
world 1."""

import os
import subprocess
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# Three rounds with replicas that depend only on the global (worker, model)
# id and the round, so every world size trains the same values. Training
# runs plain and the compress pass is called on the rows written here. In
# round 1 only the even workers are compressed: at world 2 rank 1, which
# owns the odd ones, holds an empty plan, and its counter must still move
# for round 2 to draw what world 1 draws.
_WORKER = r"""
import copy, os, sys, pathlib
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
import torch
import secagg_cases as sc

job = sc.make_job(pathlib.Path({log!r}), device=torch.device("cpu"),
                  n_clients=10, robust_agg="median",
                  upload_compress="topk_quant", compress_ratio=0.1,
                  compress_bits=4, compress_error_feedback=1)
ci = job.client_sampling(0)
K, P = job.n_models, job.n_params
nW = len(job.owned_workers)
own = np.asarray(job.owned_workers)
uploads, residuals, stats, empty = [], [], [], []
for r in range(3):
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
    part = plan
    if r == 1:
        part = copy.copy(plan)
        part.rows = plan.rows[own[plan.rows // K] % 2 == 0]
        part.template = None
    empty.append(part.rows.size == 0)
    assert job._compress_ctr == r
    job._compress_pass(part)
    uploads.append(job.replicas.numpy().reshape(nW, K, P).copy())
    residuals.append(job._residual.numpy().reshape(nW, K, P).copy())
    job.aggregate(plan)
    stats.append(job.compress_stats())
np.savez(os.path.join({log!r}, "rank%d.npz" % job.comm.rank),
         global_params=job.global_params.numpy(), uploads=np.stack(uploads),
         residuals=np.stack(residuals), stats=np.stack(stats),
         owned=own, empty=np.asarray(empty), ctr=job._compress_ctr)
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
    _launch(1, w1, 29695)
    _launch(2, w2, 29696)
    one = [np.load(os.path.join(w1, "rank0.npz"))]
    two = [np.load(os.path.join(w2, f"rank{r}.npz")) for r in range(2)]
    assert np.array_equal(two[0]["owned"], np.arange(0, 10, 2))
    assert np.array_equal(two[1]["owned"], np.arange(1, 10, 2))
    # rank 1 held an empty plan in round 1, and only there
    assert two[1]["empty"].tolist() == [False, True, False]
    assert not two[0]["empty"].any() and not one[0]["empty"].any()
    assert all(int(t["ctr"]) == 3 for t in one + two)
    for name in ("uploads", "residuals"):
        a, b = _by_worker(one, name), _by_worker(two, name)
        assert a.shape == b.shape and a.shape[:2] == (3, 10)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    g1 = one[0]["global_params"].view(np.uint32)
    for t in two:
        assert np.array_equal(t["global_params"].view(np.uint32), g1)
        assert np.array_equal(t["stats"], one[0]["stats"])
    # the quantisation error was kept and carried, the Inf of worker 3
    # travelled rather than staying in its residual, and at most about a
    # tenth was written
    res = _by_worker(one, "residuals")
    assert np.any(res[0] != 0) and np.all(np.isfinite(res))
    up = _by_worker(one, "uploads")
    assert np.isinf(up[[0, 2], 3, 1, 7]).all()
    stats = one[0]["stats"]                      # [round, K, 2]
    assert np.all(stats[[0, 2], :, 1] > 0)
    tot = stats.sum(axis=1)                      # [round, 2]
    assert 0 < tot[1, 1] < tot[0, 1] == tot[2, 1]    # the even workers only
    frac = tot[:, 0] / tot[:, 1]
    assert np.all((frac > 0) & (frac < 0.2))
