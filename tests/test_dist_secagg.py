"""secure_agg=2 across processes (gloo): the int64 ring contributions that
the ranks put on the wire are masked, and their all_reduce is exact."""

import json
import os
import subprocess
import sys

import numpy as np

from feddrift_amd.comm import secure_agg as sa

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_WORKER_TIMELINE = r"""
import json, os, sys
sys.path.insert(0, {repo!r})
import numpy as np
from feddrift_amd.comm import Communicator
from feddrift_amd.config import Config
from feddrift_amd.engine.timeline import run_timeline

cfg = Config(model="fnn", dataset="sea", data_dir={data!r},
             client_num_in_total=6, client_num_per_round=6,
             batch_size=300, lr=0.01, epochs=5, comm_round=6,
             total_train_iteration=3, concept_num=2,
             concept_drift_algo="softcluster",
             concept_drift_algo_arg="H_A_C_1_10_0",
             change_points="T", dummy_arg=0, log_dir={log!r},
             report_client=0, secure_agg=int(os.environ["FD_SECURE"]))
comm = Communicator()
out = run_timeline(cfg, comm)
if comm.is_root:
    with open(os.path.join({log!r}, "result.json"), "w") as f:
        json.dump(out["per_iteration_test_acc"], f)
"""

# One aggregation with replicas that depend only on the global (worker,
# model) id, so every world size uploads the same values.
_WORKER_ONE_AGG = r"""
import os, sys
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
import torch
import secagg_cases as sc

import pathlib
job = sc.make_job(pathlib.Path({log!r}), device=torch.device("cpu"),
                  n_clients=6, secure_agg=2)
job.secagg_keep_contrib = True
ci = job.client_sampling(0)
plan = job.algo.plan(job, 0, ci)
job.train(plan)
K = job.n_models
for wi, w in enumerate(job.owned_workers):
    for m in range(K):
        g = torch.Generator().manual_seed(1000 + w * K + m)
        job.replicas[wi * K + m] = torch.randn(job.n_params, generator=g)
job.algo.aggregate(job, 0, plan, ci)
np.savez(os.path.join({log!r}, "rank%d.npz" % job.comm.rank),
         contrib=job._secagg_contrib.numpy(),
         replicas=job.replicas.numpy(),
         sample_num=np.asarray(plan.sample_num, dtype=np.float32),
         owned=np.asarray(job.owned_workers, dtype=np.int64),
         global_params=job.global_params.numpy())
"""


def _write_data(tmp_path):
    from feddrift_amd.data.generators import generate_data
    d = str(tmp_path / "data")
    os.makedirs(os.path.join(d, "changepoints"), exist_ok=True)
    mat = np.zeros((4, 6), dtype=int)
    mat[2:, :3] = 1
    np.savetxt(os.path.join(d, "changepoints", "T.cp"), mat, fmt="%u")
    np.random.seed(0)
    generate_data("sea", d, 3, 6, 0, 300, 0.0, 1, "T")
    return d


def _launch(worker, nproc, data, log, port, env_extra=None):
    os.makedirs(log, exist_ok=True)
    path = os.path.join(log, "worker.py")
    with open(path, "w") as f:
        f.write(worker.format(repo=REPO, data=data, log=log))
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           "--nnodes", "1", "--nproc-per-node", str(nproc), path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_world2_ring_secure_agg_matches_plain(tmp_path):
    data = _write_data(tmp_path)
    res = {}
    for secure, port in ((0, 29660), (2, 29661)):
        log = str(tmp_path / f"s{secure}")
        _launch(_WORKER_TIMELINE, 2, data, log, port,
                {"FD_SECURE": str(secure)})
        with open(os.path.join(log, "result.json")) as f:
            res[secure] = json.load(f)
    assert abs(res[0][0] - res[2][0]) < 5e-3, res
    assert np.allclose(res[0], res[2], atol=0.02), res


def test_world3_contributions_masked_and_sum_exact(tmp_path):
    w1 = str(tmp_path / "w1")
    w3 = str(tmp_path / "w3")
    _launch(_WORKER_ONE_AGG, 1, "", w1, 29662)
    _launch(_WORKER_ONE_AGG, 3, "", w3, 29663)
    one = np.load(os.path.join(w1, "rank0.npz"))
    ranks = [np.load(os.path.join(w3, f"rank{r}.npz")) for r in range(3)]
    K = one["sample_num"].shape[1]
    W = 6
    act = one["sample_num"] > 0                        # [W, K], world 1
    graph = sa.build_mask_graph(act, 0, 0, 1)
    # world 1 skips its (all intra-rank) pairs: the plain quantised sum
    wi, mo = np.nonzero(act)
    plain, bad = sa.ring_contribution(
        one["replicas"], wi * K + mo, wi, mo, one["sample_num"][wi, mo], K,
        graph, 0, 0, 24, W, masked=False)
    assert not bad and np.array_equal(one["contrib"], plain)

    total = np.zeros_like(plain, dtype=np.uint64)
    for r, d in enumerate(ranks):
        assert np.array_equal(d["owned"], np.arange(r, W, 3))
        sn = d["sample_num"]
        assert np.array_equal(sn > 0, act[d["owned"]])
        lw, lm = np.nonzero(sn > 0)
        own_plain, _ = sa.ring_contribution(
            d["replicas"], lw * K + lm, d["owned"][lw], lm, sn[lw, lm], K,
            graph, 0, 0, 24, W, masked=False)
        masked_models = 0
        for m in range(K):
            ws = graph.active[m]
            mine = [w for w in ws if w % 3 == r]
            if mine and any(w % 3 != r for w in ws):
                masked_models += 1
                assert np.all(d["contrib"][m] != own_plain[m]), (r, m)
            else:
                assert np.array_equal(d["contrib"][m], own_plain[m])
        assert masked_models, r
        total = total + d["contrib"].astype(np.uint64)
        assert np.array_equal(d["global_params"], one["global_params"])
    total = (total & np.uint64(sa.RING_MASK)).astype(np.int64)
    assert np.array_equal(total, one["contrib"])
