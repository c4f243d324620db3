"""Shared cases for the ring-arithmetic secure aggregation tests
(tests/test_secure_agg_ring.py on the CPU, tests/test_gpu_secagg.py against
the HIP kernels): a replica bank whose upload rows are neither sorted nor
contiguous, weights that include a non-integer, per-rank plans under the
`w % world` ownership rule, and the FLJob round helper with the error
bound of the issue, computed from the inputs."""

import numpy as np
import torch

from feddrift_amd.comm import secure_agg as sa
from feddrift_amd.ops.secagg_hip import SecaggPlan

F = 24
MASK = np.uint64(sa.RING_MASK)


class Case:
    """Uploads = the True cells of act [W, K]."""

    def __init__(self, P, act, degree=0, seed=0, scale=1.0):
        rng = np.random.default_rng(seed)
        self.act = np.asarray(act, dtype=bool)
        self.W, self.K = self.act.shape
        self.P = P
        self.pairs = np.argwhere(self.act)
        rng.shuffle(self.pairs)                       # upload order: mixed
        U = len(self.pairs)
        R = 2 * U + 3                                  # bank with holes
        self.rows = rng.choice(R, size=U, replace=False)
        self.bank = (rng.standard_normal((R, P)) * scale).astype(np.float32)
        self.weights = rng.choice(
            np.array([1.0, 2.5, 7.0, 120.0], np.float32), size=U)
        self.graph = sa.build_mask_graph(self.act, degree, seed, 1)
        self.base = sa.job_key(seed, 1)
        self.ctr = 5

    def owned(self, rank, world):
        return self.pairs[:, 0] % world == rank

    def plan(self, rank=0, world=1):
        s = self.owned(rank, world)
        return SecaggPlan(self.rows[s], self.pairs[s, 0], self.pairs[s, 1],
                          self.weights[s], self.K, self.graph)

    def reference(self, rank=0, world=1, skip_intra=True, masked=True,
                  n_workers=None):
        s = self.owned(rank, world)
        return sa.ring_contribution(
            self.bank, self.rows[s], self.pairs[s, 0], self.pairs[s, 1],
            self.weights[s], self.K, self.graph, self.base, self.ctr, F,
            n_workers or self.W, rank, world, skip_intra, masked)

    def cross_rank_models(self, rank, world):
        """Models in which `rank` owns a worker with a neighbour elsewhere."""
        out = []
        for m in range(self.K):
            for w in self.graph.active[m]:
                if w % world == rank and any(
                        o % world != rank
                        for o in self.graph.neighbours(m, int(w))):
                    out.append(m)
                    break
        return out


def ring_sum(contribs):
    tot = np.zeros_like(np.asarray(contribs[0]), dtype=np.uint64)
    for c in contribs:
        tot = tot + np.asarray(c).astype(np.uint64)
    return (tot & MASK).astype(np.int64)


def act_matrix(W, K, spec):
    """spec[m] = list of active workers of model m."""
    act = np.zeros((W, K), dtype=bool)
    for m, ws in enumerate(spec):
        act[list(ws), m] = True
    return act


def mean_and_bound(replicas, sample_num, K, frac_bits=F):
    """float64 weighted mean [K, P] of the replicas ([nW*K, P], weights
    [nW, K]) and the per-element bound
      [sum_w (2^-(F+1) + 2^-24 |n_w theta_w|)] / sum n + 2^-24 |mean|."""
    reps = replicas.detach().cpu().double().numpy()
    nW = sample_num.shape[0]
    reps = reps.reshape(nW, K, -1)
    n = np.asarray(sample_num, dtype=np.float32).astype(np.float64)
    tot = n.sum(axis=0)                                    # [K]
    safe = np.where(tot > 0, tot, 1.0)
    mean = np.einsum("wk,wkp->kp", n, reps) / safe[:, None]
    active = (n > 0)[:, :, None]
    err = (active * (2.0 ** -(frac_bits + 1))
           + 2.0 ** -24 * np.abs(n[:, :, None] * reps)).sum(axis=0)
    bound = err / safe[:, None] + 2.0 ** -24 * np.abs(mean)
    return mean, bound, tot > 0


def mean_and_bound_atomic(replicas, sample_num, K):
    """The sibling of mean_and_bound for the default (float) aggregation:
    fp32 products n_w theta_w added in fp32 in any order, then one fp32
    multiply by the reciprocal of the total. Per element
      2 n_terms 2^-24 sum_w |n_w theta_w| / sum n + 4 2^-24 |mean|,
    n_terms = the model's count of workers with a positive weight (one
    rounding of each product, one of each running sum)."""
    reps = replicas.detach().cpu().double().numpy()
    nW = sample_num.shape[0]
    reps = reps.reshape(nW, K, -1)
    n = np.asarray(sample_num, dtype=np.float32).astype(np.float64)
    tot = n.sum(axis=0)                                    # [K]
    safe = np.where(tot > 0, tot, 1.0)
    mean = np.einsum("wk,wkp->kp", n, reps) / safe[:, None]
    mag = np.abs(n[:, :, None] * reps).sum(axis=0)
    n_terms = np.maximum((n > 0).sum(axis=0), 1)           # [K]
    bound = (2.0 * n_terms * 2.0 ** -24 / safe)[:, None] * mag \
        + 4.0 * 2.0 ** -24 * np.abs(mean)
    return mean, bound, tot > 0


def make_job(tmp_path, device=None, n_clients=4, k=2, **cfg_kw):
    """The setup of tests/test_secure_agg.py."""
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_sea
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    ds = DriftDataset(data_dir="/nonexistent", dataset="sea",
                      num_client=n_clients)
    rng = np.random.default_rng(0)
    for c in range(n_clients):
        for t in range(3):
            arr = sample_sea(120, c % 2, rng)
            ds.store.put(c, t, arr[:, :3], arr[:, 3])
    tag = "_".join(f"{a}{b}" for a, b in sorted(cfg_kw.items()))
    cfg = Config(model="fnn", dataset="sea", data_dir="/nonexistent",
                 client_num_in_total=n_clients,
                 client_num_per_round=n_clients,
                 batch_size=120, epochs=2, comm_round=3,
                 total_train_iteration=2, curr_train_iteration=1,
                 concept_num=k, concept_drift_algo="softcluster",
                 concept_drift_algo_arg="H_A_C_1_10_0", bench_mode=1,
                 report_client=0, log_dir=str(tmp_path / f"j{tag}"),
                 **cfg_kw)
    comm = Communicator(device=device) if device is not None \
        else Communicator()
    return FLJob(cfg, comm, MetricLogger(enabled=False, to_file=False),
                 dataset=ds)


def rounds_against_float64(job, n_rounds=3):
    """Run rounds; after each aggregation yield (global_params float64
    numpy, float64 mean, bound, updated-model mask)."""
    ci = job.client_sampling(0)
    out = []
    for r in range(n_rounds):
        plan = job.algo.plan(job, r, ci)
        job.train(plan)
        torch_sync(job)
        mean, bound, upd = mean_and_bound(job.replicas, plan.sample_num,
                                          job.n_models)
        job.algo.aggregate(job, r, plan, ci)
        out.append((job.global_params.detach().cpu().double().numpy(),
                    mean, bound, upd))
    return out


def torch_sync(job):
    if job.device.type == "cuda":
        torch.cuda.synchronize()
