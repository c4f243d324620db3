"""CnnHipEngine.vote_multi, the path behind every ensemble-vote accuracy of
AUE, AUE-PC and KUE on the CNN configurations, held to the float64
specification of tests/vote_cases.py: many tasks at once, 1-D and [T, M]
weights, per-model masks with the soft vote, a sweep cut into chunks by
EVAL_SLOT_BUDGET, O = 62, no active model, and FLJob.ens_vote_multi on a
task list that TaskList.CHUNK splits.

Inputs, near-tie rule, bounds and the conditions that make the cases
sensitive (all asserted on the CPU before the kernel result is looked at):
tests/vote_cases.py and PARITY.md ("Ensemble vote on the CNN path").
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import gpu_variant_cases as vc  # noqa: E402
import vote_cases as vo  # noqa: E402

_ENGINES = {}


def engine(O):
    if O not in _ENGINES:
        _ENGINES[O] = vc.cnn_engine(vo.vote_world(O))
    return _ENGINES[O]


# chunked: the call runs a second time with EVAL_SLOT_BUDGET = 100
CHUNKED = {("soft", "a", True), ("hard", "c", False)}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("wkind", ["a", "b", "c"])
@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_vote_multi_against_spec(mode, wkind, masked):
    vo.check_cnn_vote(
        f"cnn vote O=10 {mode} ({wkind}) mask={int(masked)}", engine(10), 10,
        mode, wkind, masked,
        chunk_budget=100 if (mode, wkind, masked) in CHUNKED else None)


@pytest.mark.parametrize("mode,wkind,masked", [("soft", "a", True),
                                               ("hard", "c", False)])
def test_vote_multi_62_classes(mode, wkind, masked):
    vo.check_cnn_vote(
        f"cnn vote O=62 {mode} ({wkind}) mask={int(masked)}", engine(62), 62,
        mode, wkind, masked)


@pytest.mark.parametrize("wkind", ["zero", "zero_rows"])
def test_vote_multi_no_active_model(wkind):
    vo.check_cnn_no_active(f"cnn vote no active model ({wkind})", engine(10),
                           10, wkind)


def test_peaked_world_dump_and_votes():
    vo.check_peaked_probs("cnn vote O=10 dump mask=1", engine(10), 10, True)


def test_fljob_vote_multi(tmp_path):
    """FLJob.ens_vote_multi on the MNIST cnn job: the CnnHipEngine path,
    a 150-sample window that TaskList.CHUNK = 128 splits, both modes,
    against the specification on the job's own arena and models."""
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_mnist
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob, TaskList
    from feddrift_amd.eval.metrics import MetricLogger
    from feddrift_amd.ops.cnn_hip import CnnHipEngine
    ds = DriftDataset(data_dir="/nonexistent", dataset="MNIST",
                      num_client=2)
    rng = np.random.default_rng(0)
    for c in range(2):
        for t in range(3):
            arr = sample_mnist(40, 0, rng)
            ds.store.put(c, t, arr[:, :-1], arr[:, -1])
    cfg = Config(model="cnn", dataset="MNIST", data_dir="/nonexistent",
                 client_num_in_total=2, client_num_per_round=2,
                 batch_size=20, epochs=1, comm_round=1,
                 total_train_iteration=2, curr_train_iteration=1,
                 concept_num=2, concept_drift_algo="softcluster",
                 concept_drift_algo_arg="mmacc_06", bench_mode=1,
                 report_client=0, log_dir=str(tmp_path))
    job = FLJob(cfg, Communicator(),
                MetricLogger(enabled=False, to_file=False), dataset=ds)
    assert isinstance(job.mod_engine, CnnHipEngine), type(job.mod_engine)
    job.mod_engine.dropout_override = (0.0, 0.0)
    K, N = job.n_models, job.arena.x.shape[0]
    assert K >= 2 and N >= 200 and TaskList.CHUNK == 128
    # distinct, peaked models: the job starts from K copies of one init
    g = torch.Generator().manual_seed(21)
    gp = torch.randn(K, job.n_params, generator=g) * 0.05
    bounds = np.concatenate([[0], np.cumsum(job.packer.numels)])
    job.global_params.copy_(vo.peak(gp, bounds))

    T = 3
    tl = TaskList()
    t0, t1, t2 = tl.new_task(), tl.new_task(), tl.new_task()
    tl.add_windows(t2, 0, [(151, 37)])
    tl.add_windows(t0, 0, [(0, 150), (N - 1, 1)])
    assert tl.ln == [37, 128, 22, 1] and tl.n_tasks == T and t1 == 1
    idx = job.eval_tensors(tl)
    wins = (torch.tensor(tl.task_id), torch.tensor(tl.off),
            torch.tensor(tl.ln))
    pos, task_of = vo.slot_index(wins)
    world = dict(packer=job.packer, gp=job.global_params.cpu(), O=10,
                 x=job.arena.x.cpu())
    y_own = job.arena.y.cpu().clone()
    outs = vo.model_outputs(world, pos, None, torch.float64)
    o32 = vo.model_outputs(world, pos, None, torch.float32)
    weights = torch.linspace(0.5, 1.5, K)
    # the soft near-tie threshold from fp32 torch's own vote error on
    # these inputs, as vote_cases.VOTE_ERR32 is for its worlds
    err32 = (vo.votes_fp32(o32, weights, task_of).double()
             - vo.vote_rows(outs, weights, task_of, "soft")).abs().max().item()
    vc.record("fljob cnn vote", "soft votes", err32, None,
              vo.EXPF_MARGIN * err32)

    for mode in ("soft", "hard"):
        def run(y):
            job.arena.y = y.to(job.device)
            out = job.ens_vote_multi(weights.to(job.device), tl, idx, mode)
            torch.cuda.synchronize()
            return out
        res = vo.check_vote(f"fljob cnn vote {mode}", run, outs, weights,
                            task_of, pos, y_own, T, mode,
                            out_gap=vc.NEAR_TIE_CNN,
                            soft_gap=2 * vo.EXPF_MARGIN * err32)
        assert res["spec"]["out"][1].tolist() == [151.0, 0.0, 37.0]
