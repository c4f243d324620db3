"""Run configuration: argparse surface + the string micro-DSL parsers.

Compatible with the reference CLI surface:
  * the argparse flags of fedml_experiments/distributed/fedavg_cont_ens/main_fedavg.py:42-139
  * the DRIFT_ALGO / DRIFT_ALGO_ARG mini-DSLs parsed in
    fedml_api/distributed/fedavg_ens/FedAvgEnsDataLoader.py:1272-1341 (softcluster),
    :269-314 (driftsurf), :128-143 (ada)
  * the retrain_data DSL of fedml_api/data_preprocessing/common/retrain.py:7-91
"""

from __future__ import annotations

import argparse
from dataclasses import dataclass, field, fields


# Per-dataset default drift-detection deltas
# (reference FedAvgEnsDataLoader.py:1274 and :455).
DEFAULT_DELTAS = {"sea": 0.04, "sine": 0.20, "circle": 0.10, "MNIST": 0.10}
# DriftSurf uses its own table (reference FedAvgEnsDataLoader.py:274).
DRIFTSURF_DELTAS = {"sea": 0.02, "sine": 0.10, "circle": 0.05}


@dataclass
class Config:
    model: str = "fnn"
    dataset: str = "sea"
    data_dir: str = "./data"
    client_num_in_total: int = 10
    client_num_per_round: int = 10
    batch_size: int = 500
    client_optimizer: str = "adam"       # reference default: adam (amsgrad, wd)
    lr: float = 0.01
    wd: float = 0.001
    epochs: int = 5                      # local steps per round
    comm_round: int = 200
    frequency_of_the_test: int = 1
    ci: int = 0
    total_train_iteration: int = 10
    curr_train_iteration: int = 0
    drift_together: int = 0
    report_client: int = 1
    retrain_data: str = "win-1"
    concept_drift_algo: str = "softcluster"
    concept_drift_algo_arg: str = ""
    ensemble_window: int = 4
    concept_num: int = 4
    change_points: str = "rand"
    time_stretch: int = 1
    reset_models: int = 0
    # data-GENERATION surface args (consumed by scripts/prepare_data.py /
    # generate_data at data-prep time, like the reference's main_fedavg
    # arg list; the engine itself reads the generated CSVs)
    noise_prob: float = 0.0
    dummy_arg: int = 0
    sample_num: int = 500                # samples per (client, iteration)

    # engine knobs (new; no reference equivalent)
    device: str = "auto"                 # auto|cpu|cuda
    backend: str = "auto"                # auto|gloo|nccl
    use_hip_kernels: str = "auto"        # auto|always|never
    wandb: int = 0                       # optional wandb mirror of metric logs
    log_dir: str = "."                   # where checkpoints/state files go
    bench_mode: int = 0                  # 1: synthetic steady-state (bench.py)

    # robust aggregation (fedavg_robust / fedml_core robustness equivalent)
    secure_agg: int = 0                  # 1: pairwise-mask uploads
                                         # (turboaggregate equivalent)
                                         # 2: exact ring-arithmetic masks
    secure_agg_degree: int = 0           # mode 2 mask graph: 0 = complete,
                                         # d (even) = d neighbours per worker
    secure_agg_frac_bits: int = 24       # mode 2 fixed-point fraction bits
    robust_norm_bound: float = 0.0       # >0: clip client updates to this L2
    robust_noise: float = 0.0            # >0: Gaussian noise stddev on avg
    robust_fused: int = 0                # 1: clip / noise / server optimizer
                                         # on the fused path (HIP kernels on a
                                         # GPU, the specification on CPU)
    robust_agg: str = "mean"             # mean|trimmed_mean|median: the
                                         # per-coordinate statistic over a
                                         # model's uploads (unweighted for
                                         # the two order statistics);
                                         # multi_krum: the mean of the
                                         # uploads closest to the others
    robust_trim_frac: float = 0.1        # trimmed_mean: share dropped at
                                         # either end, in [0, 0.5)
    robust_krum_frac: float = 0.2        # multi_krum: share of a model's
                                         # uploads assumed Byzantine, [0, 0.5)
    robust_krum_select: int = 0          # multi_krum: uploads kept, 0 = all
                                         # but the assumed Byzantine ones;
                                         # 1 = classic Krum
    # FedOpt server optimizer ('avg' = plain FedAvg replacement)
    server_optimizer: str = "avg"
    server_lr: float = 1.0
    server_momentum: float = 0.0         # sgd only (FedAvgM)
    # FedProx proximal local training: every executed local step adds
    # mu * (w - w0) to the gradient, w0 = the global model the client got
    # this round (0 = plain local training, bit for bit)
    fedprox_mu: float = 0.0
    # upload compression: none|topk|quant|topk_quant. topk sends the
    # compress_ratio share of largest-magnitude coordinates of every trained
    # row's update; quant sends every coordinate stochastically rounded to
    # compress_bits bits against the row's largest magnitude; topk_quant
    # quantises what topk sends. With compress_error_feedback=1 what was
    # held back (the quantisation error included) joins the next update
    upload_compress: str = "none"
    compress_ratio: float = 0.01         # share of a row sent, in (0, 1]
    compress_error_feedback: int = 1
    compress_bits: int = 8               # per coordinate, sign included

    def __post_init__(self):
        self.dataset_norm = "MNIST" if self.dataset.lower() == "mnist" else self.dataset
        if self.upload_compress not in ("none", "topk", "quant",
                                        "topk_quant"):
            raise ValueError("upload_compress must be one of none, topk, "
                             f"quant, topk_quant, got '{self.upload_compress}'")
        if not 0.0 < self.compress_ratio <= 1.0:
            raise ValueError("compress_ratio must lie in (0, 1], got "
                             f"{self.compress_ratio}")
        if self.compress_error_feedback not in (0, 1):
            raise ValueError("compress_error_feedback must be 0 or 1, got "
                             f"{self.compress_error_feedback}")
        if isinstance(self.compress_bits, bool) or \
                not isinstance(self.compress_bits, int) or \
                not 2 <= self.compress_bits <= 16:
            raise ValueError("compress_bits must be an integer in [2, 16], "
                             f"got {self.compress_bits!r}")
        if not (self.fedprox_mu >= 0.0 and self.fedprox_mu != float("inf")):
            raise ValueError("fedprox_mu must be finite and >= 0, got "
                             f"{self.fedprox_mu}")
        if self.secure_agg_degree < 0 or self.secure_agg_degree % 2:
            raise ValueError("secure_agg_degree must be even and >= 0, got "
                             f"{self.secure_agg_degree}")
        if not 0 <= self.secure_agg_frac_bits <= 40:
            raise ValueError("secure_agg_frac_bits must lie in [0, 40], got "
                             f"{self.secure_agg_frac_bits}")
        if self.robust_fused not in (0, 1):
            raise ValueError("robust_fused must be 0 or 1, got "
                             f"{self.robust_fused}")
        if self.robust_agg not in ("mean", "trimmed_mean", "median",
                                   "multi_krum"):
            hint = " (classic Krum is robust_agg=multi_krum with " \
                "robust_krum_select=1)" if self.robust_agg == "krum" else ""
            raise ValueError("robust_agg must be one of mean, trimmed_mean, "
                             f"median, multi_krum, got '{self.robust_agg}'"
                             f"{hint}")
        if not 0.0 <= self.robust_trim_frac < 0.5:
            raise ValueError("robust_trim_frac must lie in [0, 0.5), got "
                             f"{self.robust_trim_frac}")
        if not 0.0 <= self.robust_krum_frac < 0.5:
            raise ValueError("robust_krum_frac must lie in [0, 0.5), got "
                             f"{self.robust_krum_frac}")
        if self.robust_krum_select < 0:
            raise ValueError("robust_krum_select must be >= 0, got "
                             f"{self.robust_krum_select}")
        if self.robust_agg != "mean" and self.secure_agg != 0:
            raise ValueError(
                f"robust_agg='{self.robust_agg}' cannot run with secure_agg="
                f"{self.secure_agg}: an order statistic needs the individual "
                "uploads, and secure aggregation exists to hide them")

    @property
    def is_softcluster(self) -> bool:
        return self.concept_drift_algo in (
            "softcluster", "softclusterwin-1", "softclusterreset")


def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    for f in fields(Config):
        if f.name in ("dataset_norm",):
            continue
        parser.add_argument("--" + f.name, type=type(f.default), default=f.default)
    return parser


def config_from_argv(argv=None) -> Config:
    parser = argparse.ArgumentParser()
    add_args(parser)
    ns, _ = parser.parse_known_args(argv)
    return Config(**{f.name: getattr(ns, f.name) for f in fields(Config)
                     if hasattr(ns, f.name)})


# ---------------------------------------------------------------------------
# DRIFT_ALGO_ARG parsers
# ---------------------------------------------------------------------------

@dataclass
class SoftClusterParams:
    """Parsed concept_drift_algo_arg for the softcluster family.

    Mirrors the parse in reference FedAvgEnsDataLoader.py:1279-1328:
      'hard' | 'hard-r' (IFCA)        -> cluster_alg as-is
      'softmax_{alpha}'               -> softmax_alpha = int
      'mmacc_{100*delta}'             -> mmacc_delta (FedDrift-Eager)
      'gmm', 'geni'                   -> as-is
      'H_{dist}_{clust}_{W}_{100d}_{100dp}' -> FedDrift hierarchical
      'cfl_{gamma}_{win-1|all}'       -> CFL inside softcluster
    """
    cluster_alg: str = ""
    mmacc_delta: float = 0.0
    softmax_alpha: int = 0
    h_delta: float = 0.0
    h_deltap: float = 0.0
    h_w: int = 0
    h_distance: str = ""
    h_cluster: str = ""
    cfl_gamma: float = 0.0
    cfl_retrain: str = ""


def parse_softcluster_arg(arg: str, dataset: str) -> SoftClusterParams:
    p = SoftClusterParams(cluster_alg=arg)
    if "mmacc" in arg:
        p.mmacc_delta = 0.01 * float(arg.split("_")[-1])
        if p.mmacc_delta == 0 and dataset in DEFAULT_DELTAS:
            p.mmacc_delta = DEFAULT_DELTAS[dataset]
    elif "softmax" in arg:
        p.softmax_alpha = int(arg.split("_")[-1])
    elif arg == "geni":
        pass
    elif "H" in arg:
        parts = arg.split("_")
        p.h_distance = parts[1]
        p.h_cluster = parts[2]
        p.h_w = int(parts[3])
        p.h_delta = 0.01 * float(parts[4])
        if p.h_delta == 0 and dataset in DEFAULT_DELTAS:
            p.h_delta = DEFAULT_DELTAS[dataset]
        p.h_deltap = 0.01 * float(parts[5])
        if p.h_deltap == 0:
            p.h_deltap = p.h_delta
    elif "cfl" in arg:
        parts = arg.split("_")
        p.cfl_gamma = float(parts[1])
        p.cfl_retrain = parts[2]
    return p


def driftsurf_delta(arg: str, dataset: str) -> float:
    """DriftSurf delta from its algo arg (reference FedAvgEnsDataLoader.py:273-278)."""
    d = 0.01 * float(arg) if arg else 0.0
    if d == 0:
        d = DRIFTSURF_DELTAS.get(dataset, 0.1)
    return d


def parse_ada_arg(arg: str):
    """'{win-1|all}_{round|iter}' (reference FedAvgEnsDataLoader.py:137-138,
    FedAvgEnsAggregatorAda.py)."""
    parts = arg.split("_")
    retrain = parts[0] if parts[0] else "win-1"
    granularity = parts[1] if len(parts) > 1 else "round"
    return retrain, granularity
