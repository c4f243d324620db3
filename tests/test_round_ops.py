"""CPU side of the small-fleet round's launch-argument step windows: the
packing predicate of the extension (it loads without a GPU); and
client_eval on the torch backend hands out arrays of its own."""

import numpy as np
import torch

from feddrift_amd.models.packed import spec_for
from feddrift_amd.ops import hip_loader, mlp_hip

FNN, LR = 0, 1


def _mod():
    return hip_loader.load()


def test_cap_is_256_entries():
    mod = _mod()
    assert mod.INLINE_STEPS == 256
    assert mod.inline_steps_ok(3, 6, 2, FNN, 64, 4)        # 256 entries
    assert not mod.inline_steps_ok(3, 6, 2, FNN, 257, 1)   # 257
    assert mod.inline_steps_ok(3, 6, 2, FNN, 1, 256)
    assert not mod.inline_steps_ok(3, 6, 2, FNN, 1, 257)
    assert not mod.inline_steps_ok(3, 6, 2, FNN, 65, 4)


def test_every_small_shape_and_none_other():
    mod = _mod()
    small = [(3, 6, 2, FNN), (2, 4, 2, FNN), (4, 8, 2, FNN), (3, 0, 2, LR),
             (2, 0, 2, LR)]
    for s in small:
        assert mod.inline_steps_ok(*s, 10, 5), s
    for s in [(12, 24, 4, FNN), (3, 6, 3, FNN), (3, 5, 2, FNN), (4, 0, 2, LR),
              (3, 6, 2, LR)]:
        assert not mod.inline_steps_ok(*s, 10, 5), s
    # the wrapper asks with the model's spec
    assert mlp_hip.inline_steps_ok(spec_for("fnn", 3, 2), 10, 5)
    assert mlp_hip.inline_steps_ok(spec_for("lr", 2, 2), 10, 5)
    assert not mlp_hip.inline_steps_ok(spec_for("fnn", 12, 4), 10, 5)
    assert not mlp_hip.inline_steps_ok(spec_for("fnn", 3, 2), 65, 4)


def test_empty_launches_pack():
    mod = _mod()
    assert mod.inline_steps_ok(3, 6, 2, FNN, 0, 5)
    assert mod.inline_steps_ok(3, 6, 2, FNN, 10, 0)
    assert mod.inline_steps_ok(3, 6, 2, FNN, 0, 0)
    assert not mod.inline_steps_ok(3, 6, 2, FNN, -1, 5)
    z = torch.zeros(0, 5, dtype=torch.int64)
    assert mod.steps_fit_inline(z, z)
    z = torch.zeros(10, 0, dtype=torch.int64)
    assert mod.steps_fit_inline(z, z)


def test_values_have_to_fit_int32():
    mod = _mod()
    t = lambda *v: torch.tensor([list(v)], dtype=torch.int64)  # noqa: E731
    top = 2 ** 31 - 1
    assert mod.steps_fit_inline(t(0, top), t(5, 0))
    assert not mod.steps_fit_inline(t(0, top + 1), t(5, 0))
    # off + len crossing 2^31
    assert mod.steps_fit_inline(t(top - 5), t(5))
    assert not mod.steps_fit_inline(t(top - 5), t(6))
    assert not mod.steps_fit_inline(t(5), t(top + 1))
    assert not mod.steps_fit_inline(t(-1), t(5))
    assert not mod.steps_fit_inline(t(5), t(-1))
    # more entries than the cap
    big = torch.zeros(257, 1, dtype=torch.int64)
    assert not mod.steps_fit_inline(big, big)
    ok = torch.zeros(64, 4, dtype=torch.int64)
    assert mod.steps_fit_inline(ok, ok + 500)


def _cpu_job(n=4, it=1):
    from feddrift_amd.comm import Communicator
    from feddrift_amd.config import Config
    from feddrift_amd.data.generators import sample_sea
    from feddrift_amd.data.loader import DriftDataset
    from feddrift_amd.engine.fljob import FLJob
    from feddrift_amd.eval.metrics import MetricLogger
    ds = DriftDataset(data_dir="/nonexistent", dataset="sea", num_client=n)
    rng = np.random.default_rng(0)
    for c in range(n):
        for t in range(it + 2):
            arr = sample_sea(200, c % 2, rng)
            ds.store.put(c, t, arr[:, :3], arr[:, 3])
    cfg = Config(model="fnn", dataset="sea", data_dir="/nonexistent",
                 client_num_in_total=n, client_num_per_round=n,
                 batch_size=200, epochs=2, comm_round=10 ** 9,
                 total_train_iteration=it + 1, curr_train_iteration=it,
                 concept_num=2, concept_drift_algo="softcluster",
                 concept_drift_algo_arg="H_A_C_1_10_0", bench_mode=1,
                 report_client=0, use_hip_kernels="never")
    return FLJob(cfg, Communicator(),
                 MetricLogger(enabled=True, to_file=False), dataset=ds)


def test_client_eval_on_the_torch_backend_returns_fresh_arrays():
    job = _cpu_job()
    assert not job._hip_mlp
    midx = np.array([0, 1, 0, 1])
    tr1, te1 = job.client_eval(midx)
    kept = [a.copy() for a in tr1 + te1]
    tr2, te2 = job.client_eval(midx)
    for a, b in zip(tr1 + te1, tr2 + te2):
        assert np.array_equal(a, b)
        assert not np.shares_memory(a, b)
    for a in tr2 + te2:                     # writing one leaves the other
        a[...] = -7.0
    for a, b in zip(tr1 + te1, kept):
        assert np.array_equal(a, b)
    tr3, te3 = job.client_eval(midx)
    for a, b in zip(tr3 + te3, kept):
        assert np.array_equal(a, b)

