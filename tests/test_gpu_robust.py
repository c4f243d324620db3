"""robust_fused=1 HIP kernels (ops/hip/robust_kernels.hip) against the
float64 specification (comm/robust.py, norm_diff_clipping + einsum,
ServerOptimizer): vector lengths around a block's element span and at CNN
size, pair counts below and above one slice's share, unsorted rows with
holes and an empty model, the five norm cases, the apply pass for every
optimizer kind over three launches, the noise against gaussian_noise, and
FLJob on the device. Bounds: tests/robust_cases.py."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import robust_cases as rc  # noqa: E402
import secagg_cases as sc  # noqa: E402
from feddrift_amd.comm import robust as rb  # noqa: E402
from feddrift_amd.comm import secure_agg as sa  # noqa: E402
from feddrift_amd.ops import hip_loader, robust_hip  # noqa: E402

DEV = torch.device("cuda:0")
KEY = sa.job_key(3, 1)


def test_native_extension_has_the_kernels():
    mod = hip_loader.load()
    assert mod.__file__.endswith(".so")
    assert robust_hip.span() == 1024
    assert hasattr(mod, "robust_clip") and hasattr(mod, "robust_apply")


# ------------------------------------------------------------------- clip

def _run_clip(case, with_partial=True, slices=None):
    bank = torch.from_numpy(case.bank).to(DEV)
    glob = torch.from_numpy(case.glob).to(DEV)
    partial = torch.zeros(case.K, case.P + 1, device=DEV) \
        if with_partial else None
    counts = robust_hip.new_counts(case.K, DEV)
    plan = robust_hip.ClipPlan(case.rows, case.models, case.weights, case.K)
    robust_hip.clip_accumulate(bank, plan, glob, case.bound, partial, counts,
                               slices=slices)
    torch.cuda.synchronize()
    assert torch.equal(glob.cpu(), torch.from_numpy(case.glob))
    return (bank.cpu().numpy(),
            partial.cpu().numpy() if with_partial else None,
            counts.cpu().numpy(), plan)


def _three_pairs():
    return [(0, 2.5, "rand"), (0, 7.0, "rand"), (0, 1.0, "far")]


@pytest.mark.parametrize("idx", range(5))
def test_clip_vector_lengths(idx):
    s = robust_hip.span()
    P = [1, 35, s - 1, s, s + 1][idx]
    case = rc.ClipCase(P, 1, _three_pairs(), seed=P)
    bank, partial, counts, _ = _run_clip(case)
    rc.check_clip(f"clip P={P}", case, bank, partial, counts)


def test_clip_cnn_sized_vector():
    from feddrift_amd.models import zoo
    from feddrift_amd.models.generic_packer import ModulePacker
    P = ModulePacker(zoo.CNN_DropOut()).n_params
    case = rc.ClipCase(P, 1, _three_pairs() + [(0, 120.0, "near")], seed=4)
    bank, partial, counts, plan = _run_clip(case)
    assert plan.slices(P) == 1            # the element chunks fill the chip
    rc.check_clip("clip CNN P", case, bank, partial, counts)


@pytest.mark.parametrize("n_pairs", [0, 1, 2, 70])
def test_clip_pairs_per_model(n_pairs):
    """70 pairs exceed one slice's share: several slices, summed in order."""
    pairs = [(0, [1.0, 2.5, 7.0, 120.0][i % 4], ["rand", "far"][i % 3 == 0])
             for i in range(n_pairs)]
    case = rc.ClipCase(34, 1, pairs, seed=n_pairs)
    bank, partial, counts, plan = _run_clip(case)
    assert (plan.slices(34) > 1) == (n_pairs == 70)
    rc.check_clip(f"clip pairs={n_pairs}", case, bank, partial, counts)
    if n_pairs == 0:
        assert not partial.any() and not counts.any()


def test_clip_three_models_one_empty_unsorted_rows():
    pairs = [(1, 7.0, "rand")] + \
        [(2, [1.0, 2.5, 120.0][i % 3], "rand") for i in range(6)]
    case = rc.ClipCase(229, 3, pairs, seed=11)
    assert np.any(np.diff(case.rows) < 0)
    assert np.any(np.diff(case.models) < 0)
    bank, partial, counts, _ = _run_clip(case)
    rc.check_clip("clip 3 models", case, bank, partial, counts)
    assert not partial[0].any() and not counts[0].any()


def test_clip_five_norm_cases_and_clip_only():
    case = rc.ClipCase(229, 3, rc.five_norm_pairs(), seed=1)
    bank, partial, counts, _ = _run_clip(case)
    rc.check_clip("clip five norms", case, bank, partial, counts)
    # partial=None: the replicas change in the same way, nothing else does
    bank2, none, counts2, _ = _run_clip(case, with_partial=False)
    assert none is None
    assert np.array_equal(bank2.view(np.uint32), bank.view(np.uint32))
    assert np.array_equal(counts2, counts)
    # the slice count cannot change a clipped row
    bank3, _, _, _ = _run_clip(case, slices=3)
    assert np.array_equal(bank3.view(np.uint32), bank.view(np.uint32))


# ------------------------------------------------------------------ apply

def _apply_inputs(K, P, seed):
    """partial [K, P+1] of weighted sums, a masked row and a zero-total row
    (when K allows), and the float64 average."""
    rng = np.random.default_rng(seed)
    glob = (rng.standard_normal((K, P)) * 0.3).astype(np.float32)
    tot = rng.choice(np.array([3.0, 10.5, 127.0], np.float32), size=K)
    avg = glob.astype(np.float64) + rng.standard_normal((K, P)) * 0.05
    mask = np.ones(K, dtype=np.uint8)
    if K >= 3:
        mask[1] = 0
        tot[2] = 0.0
    partial = np.zeros((K, P + 1), dtype=np.float32)
    partial[:, :P] = (avg * tot[:, None]).astype(np.float32)
    partial[:, P] = tot
    partial[tot == 0, :P] = 0.123          # stale sums under a zero total
    upd = (tot > 0) & (mask > 0)
    safe = np.where(tot > 0, tot, 1.0).astype(np.float64)
    avg64 = partial[:, :P].astype(np.float64) / safe[:, None]
    inv32 = (np.float32(1.0) / safe.astype(np.float32))
    avg32 = partial[:, :P] * inv32[:, None]
    return glob, partial, mask, tot, upd, avg64, avg32


def _launch_apply(glob_t, partial, mask, state, noise=0.0, ctr=0, slabs=None):
    part_t = torch.from_numpy(partial).to(DEV)
    mask_t = torch.from_numpy(mask).to(DEV) if mask is not None else None
    totals = torch.full((glob_t.shape[0],), -1.0, device=DEV)
    robust_hip.apply(glob_t, part_t, mask_t, totals, state, noise, KEY, ctr,
                     slabs=slabs)
    torch.cuda.synchronize()
    assert not part_t.any(), "partial not drained"
    return totals.cpu().numpy()


@pytest.mark.parametrize("K", [1, 3, 512])
@pytest.mark.parametrize("P_idx", range(3))
def test_apply_plain_average(K, P_idx):
    P = [229, 412, robust_hip.span() + 1][P_idx]
    glob, partial, mask, tot, upd, avg64, avg32 = _apply_inputs(K, P, K + P)
    glob_t = torch.from_numpy(glob).to(DEV)
    totals = _launch_apply(glob_t, partial, mask, robust_hip.ServerState("avg"))
    got = glob_t.cpu().numpy()
    assert np.array_equal(totals, tot)
    assert np.array_equal(got[~upd].view(np.uint32),
                          glob[~upd].view(np.uint32))
    if K >= 3:
        assert not upd[1] and not upd[2] and upd[0]
    rc.check(f"apply avg K={K} P={P}", "rows", got[upd], avg32[upd],
             avg64[upd])


@pytest.mark.parametrize("kind,lr,momentum", rc.SERVER_CASES)
def test_apply_optimizer_three_launches(kind, lr, momentum):
    K, P = 3, 412
    glob, avgs, upds = rc.server_inputs(K, P, seed=8)
    glob = glob.astype(np.float32)
    tot = np.array([3.0, 10.5, 127.0], np.float32)
    partials, avg64s, avg32s = [], [], []
    for a in avgs:
        p = np.zeros((K, P + 1), dtype=np.float32)
        p[:, :P] = (a * tot[:, None]).astype(np.float32)
        p[:, P] = tot
        partials.append(p)
        avg64s.append(p[:, :P].astype(np.float64) / tot[:, None])
        avg32s.append(p[:, :P] * (np.float32(1.0) / tot)[:, None])
    want = rc.server_reference(kind, lr, momentum, glob, avg64s, upds)
    spec32 = rc.server_spec(kind, lr, momentum, glob, avg32s, upds,
                            torch.float32)
    state = robust_hip.ServerState(kind, lr, momentum)
    glob_t = torch.from_numpy(glob).to(DEV)
    for step in range(3):
        mask = upds[step].astype(np.uint8)     # launch 2 skips row K-1
        _launch_apply(glob_t, partials[step], mask, state)
        rc.check(f"apply {kind} m={momentum} launch {step + 1}", "bank",
                 glob_t.cpu().numpy(), spec32[step], want[step])
    assert state.step == (0 if kind == "avg" else 3)


def test_apply_noise_matches_specification_at_any_slab_count():
    K, P, std = 3, robust_hip.span() + 1, 1e-2
    glob, partial, mask, tot, upd, avg64, avg32 = _apply_inputs(K, P, 21)
    outs = []
    for slabs in (1, 3):
        glob_t = torch.from_numpy(glob).to(DEV)
        _launch_apply(glob_t, partial, mask, robust_hip.ServerState("avg"),
                      noise=std, ctr=(1 << 32) + 5, slabs=slabs)
        outs.append(glob_t.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    got = outs[0]
    assert np.array_equal(got[~upd].view(np.uint32),
                          glob[~upd].view(np.uint32))
    z64 = rb.gaussian_noise(KEY, (1 << 32) + 5, K, P)
    z32 = rb.gaussian_noise(KEY, (1 << 32) + 5, K, P, dtype=np.float32)
    spec32 = avg32 + np.float32(std) * z32
    noise_got = got.astype(np.float64) - avg64
    rc.check("apply noise", "global - average", noise_got[upd],
             spec32[upd].astype(np.float64) - avg64[upd], std * z64[upd])
    # and it is noise: unit variance, a different draw per counter
    zs = noise_got[upd] / std
    assert abs(zs.var() - 1.0) < 0.1 and abs(zs.mean()) < 0.1
    glob_t = torch.from_numpy(glob).to(DEV)
    _launch_apply(glob_t, partial, mask, robust_hip.ServerState("avg"),
                  noise=std, ctr=6)
    assert not np.any(glob_t.cpu().numpy()[upd] == got[upd])


# ------------------------------------------------------------------ FLJob

def test_fljob_clips_on_device(tmp_path):
    job = sc.make_job(tmp_path, use_hip_kernels="always", robust_fused=1,
                      robust_norm_bound=0.05)
    assert job.device.type == "cuda"
    ci = job.client_sampling(0)
    prev = job.global_params.double().cpu().numpy().copy()
    for r in range(3):
        plan = rc.job_round(job, r, ci)
        sc.torch_sync(job)
        norms = rc.update_norms(job, plan, prev)
        print(f"FIG fljob gpu round {r} | max norm/bound "
              f"{norms.max() / 0.05:.8f}")
        assert norms.max() <= 0.05 * (1 + 2.0 ** -20)
        mean, bound, upd = sc.mean_and_bound_atomic(
            job.replicas, plan.sample_num, job.n_models)
        job.algo.aggregate(job, r, plan, ci)
        gp = job.global_params.double().cpu().numpy()
        touched = 0
        for m in range(job.n_models):
            if not upd[m] or np.array_equal(gp[m], prev[m]):
                continue
            touched += 1
            err = np.abs(gp[m] - mean[m])
            print(f"FIG fljob gpu round {r} model {m} | err/bound "
                  f"{(err / bound[m]).max():.3f}")
            assert np.all(err <= bound[m])
        assert touched
        prev = gp
    st = job.clip_stats()
    assert np.array_equal(st[:, 0], st[:, 1]) and st[:, 1].sum() > 0


def test_fljob_noise_and_adam_match_cpu_specification(tmp_path):
    # server_lr 1e-3: an Adam step is lr m / (sqrt v + eps), so a relative
    # error e of the pseudo-gradient moves the parameter by about lr e,
    # far inside the bound of the mean
    kw = dict(robust_fused=1, robust_norm_bound=0.05, robust_noise=1e-3,
              server_optimizer="adam", server_lr=1e-3)
    jg = sc.make_job(tmp_path / "g", use_hip_kernels="always", **kw)
    jc = sc.make_job(tmp_path / "c", device=torch.device("cpu"), **kw)
    assert jg.device.type == "cuda" and jc.device.type == "cpu"
    ci = jg.client_sampling(0)
    for r in range(3):
        jc.global_params.copy_(jg.global_params.cpu())
        pg = rc.job_round(jg, r, ci)
        sc.torch_sync(jg)
        # the CPU job aggregates copies of the device's clipped replicas
        pc = jc.algo.plan(jc, r, ci)
        jc.train(pc)
        assert np.array_equal(pc.sample_num, pg.sample_num)
        jc.replicas.copy_(jg.replicas.cpu())
        jc._partial_fused = False          # sum the copies, not its own rows
        mean, bound, upd = sc.mean_and_bound_atomic(
            jg.replicas, pg.sample_num, jg.n_models)
        jg.algo.aggregate(jg, r, pg, ci)
        jc.algo.aggregate(jc, r, pc, ci)
        gg = jg.global_params.double().cpu().numpy()
        gc = jc.global_params.double().numpy()
        for m in range(jg.n_models):
            diff = np.abs(gg[m] - gc[m])
            print(f"FIG fljob gpu-vs-spec round {r} model {m} | diff "
                  f"{diff.max():.3e} | bound {bound[m].max():.3e}")
            assert np.all(diff <= bound[m])
