"""Size dispatch of ops/mlp_hip.py (no GPU): every MLP kernel keeps one
sample's logits in a float[64], so a spec with more than 64 outputs must
take the torch path in all four entry points."""

import torch

from feddrift_amd.models.packed import spec_for
from feddrift_amd.ops import mlp_hip, mlp_torch


def test_fits_rejects_more_than_64_outputs():
    wide = spec_for("lr", 10, 100)
    assert not mlp_hip._fits_train(wide)
    assert not mlp_hip._fits_eval(wide)
    assert not mlp_hip._fits_train(spec_for("fnn", 10, 65))
    for ok in (spec_for("lr", 10, 64), spec_for("fnn", 3, 2)):
        assert mlp_hip._fits_train(ok) and mlp_hip._fits_eval(ok)


def test_wide_spec_routes_every_entry_point_to_torch(monkeypatch):
    # the extension must not even be looked for
    def no_load():
        raise AssertionError("o > 64 reached the HIP extension")
    monkeypatch.setattr(mlp_hip.hip_loader, "load", no_load)
    torch.manual_seed(0)
    spec = spec_for("lr", 10, 100)
    n, G, E, W, T = 300, 3, 2, 5, 2
    x = torch.rand(n, 10)
    y = torch.randint(0, 100, (n,))
    params = torch.randn(G, spec.n_params) * 0.3
    rows = torch.arange(G)
    off = torch.randint(0, n - 40, (G, E))
    ln = torch.randint(1, 40, (G, E))

    got, ref = params.clone(), params.clone()
    for fn, p in ((mlp_hip.train_fused, got), (mlp_torch.train_fused, ref)):
        opt = mlp_torch.make_opt_state("adam", G, spec.n_params, 0.01, 1e-3,
                                       "cpu")
        fn(spec, p, rows, x, y, off, ln, opt)
    assert torch.equal(got, ref)

    task_row = torch.randint(0, G, (W,))
    task_id = torch.randint(0, T, (W,))
    woff = torch.randint(0, n - 40, (W,))
    wln = torch.randint(1, 40, (W,))
    a = mlp_hip.eval_tasks(spec, params, x, y, task_row, task_id, woff, wln,
                           T, want_mse=True)
    b = mlp_torch.eval_tasks(spec, params, x, y, task_row, task_id, woff,
                             wln, T, want_mse=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    wts = torch.rand(G)
    assert torch.equal(
        mlp_hip.ens_vote_multi(spec, params, wts, x, y, task_id, woff, wln,
                               T),
        mlp_torch.ens_vote_multi(spec, params, wts, x, y, task_id, woff, wln,
                                 T))
    assert torch.equal(
        mlp_hip.confusion_tasks(spec, params, x, y, task_row, task_id, woff,
                                wln, T, 100),
        mlp_torch.confusion_tasks(spec, params, x, y, task_row, task_id,
                                  woff, wln, T, 100))


def test_opt_state_dtype_default_unchanged():
    st = mlp_torch.make_opt_state("adam", 2, 5, 0.01, 0.0, "cpu")
    assert all(st[k].dtype == torch.float32 for k in ("lr", "m", "v", "vmax"))
    assert st["t"].dtype == torch.int32
    st = mlp_torch.make_opt_state("adam", 2, 5, 0.01, 0.0, "cpu",
                                  dtype=torch.float64)
    assert all(st[k].dtype == torch.float64 for k in ("lr", "m", "v", "vmax"))
