"""MLP kernels (ops/hip/feddrift_kernels.hip) at their tile, chunk and
dispatch edges, against float64 references on the CPU.

tests/test_gpu_ops.py compares fp32 with fp32 at steps shorter than 100
samples and P <= 229; here every template instantiation of the small
kernels runs (with and without x_mask), the generic train kernel takes 1,
2 and 3 trips of its LDS chunk loop with P above and below the 256-thread
stride, the generic eval / confusion / vote kernels see windows longer
than a block, masks and per-task weights, and apply_aggregate runs with
more than one wave of parameters per model. Bounds and their derivation:
tests/gpu_variant_cases.py and PARITY.md ("Kernel edge and variant
coverage").
"""

import os

import pytest
import torch

# latched once per process by the C++ dispatch (see tests/test_gpu_ops.py):
# the five template shapes take mlp_eval_small_kernel even at tiny grids;
# every other shape still reaches the generic mlp_eval_kernel
os.environ.setdefault("FEDDRIFT_FORCE_SMALL_EVAL", "1")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import gpu_variant_cases as vc  # noqa: E402
import vote_cases as vo  # noqa: E402
from feddrift_amd.models.packed import spec_for  # noqa: E402
from feddrift_amd.ops import mlp_hip, mlp_torch  # noqa: E402

DEV = torch.device("cuda:0")

# Per-sample CE / mse of the eval kernels: 8 x the largest per-sample err32
# over the eval cases (PARITY.md table); a task's sum scales by its count.
MLP_CE_ERR32 = 1.26e-5
MLP_MSE_ERR32 = 1.25e-6
MLP_CE_TOL = 8 * MLP_CE_ERR32
MLP_MSE_TOL = 8 * MLP_MSE_ERR32

EVAL_SHAPES = vc.SMALL_SHAPES + vc.GENERIC_SHAPES
EVAL_LENS = (1, 64, 65, 255, 256, 257, 700)
W, T = 24, 5


# --------------------------------------------------------------------------
# training
# --------------------------------------------------------------------------

def test_small_train_all_template_shapes():
    vc.case_small_train()


@pytest.mark.parametrize("kind,d,o", vc.GENERIC_SHAPES)
@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("masked", [False, True])
def test_generic_train_chunk_loop(kind, d, o, optname, masked):
    """fnn(12,4): P = 412 > 256, nsub = 1; fnn(8,5): P = 229, nsub = 2;
    lr(4,2): P = 10, nsub clamps at 32. BC = 512 for all three."""
    i = vc.GENERIC_SHAPES.index((kind, d, o))
    inp = vc.mlp_train_inputs(kind, d, o, vc.GENERIC_LENS, masked,
                              seed=vc.GENERIC_SEEDS[i])
    assert inp["spec"].n_params == (412, 229, 10)[i]
    vc.check_mlp_train(f"generic {kind}({d},{o}) {optname} "
                       f"mask={int(masked)}", inp, optname)


def test_fused_broadcast_and_partial():
    """in_params / model_of / sample_w / partial on the generic kernel:
    some sample_w are 0 (the sw > 0 guard), one model has no pair."""
    kind, d, o, K = "fnn", 12, 4, 5
    inp = vc.mlp_train_inputs(kind, d, o, vc.GENERIC_LENS, False,
                              seed=vc.FUSED_SEED, G=9)
    spec, G, P = inp["spec"], 9, inp["spec"].n_params
    g = torch.Generator().manual_seed(301)
    glob = torch.randn(K, P, generator=g) * 0.4
    model_of = torch.tensor([0, 1, 2, 3, 0, 1, 2, 0, 3])   # model 4: no pair
    sample_w = torch.rand(G, generator=g) + 0.5
    sample_w[[1, 4]] = 0.0
    # reference: broadcast, then train in float64 (and fp32 for err32)
    inp["params"] = inp["params"].clone()
    inp["params"][inp["rows"]] = glob[model_of]
    partial = torch.zeros(K, P + 1, device=DEV)
    start = inp["params"].clone()
    start[inp["rows"]] = 0.0       # the kernel stages from in_params instead
    got = vc.mlp_train_hip(dict(inp, params=start), "adam",
                           in_params=glob.to(DEV),
                           model_of=model_of.to(torch.int32).to(DEV),
                           sample_w=sample_w.to(DEV), partial=partial)
    figs, o64 = vc.mlp_train_figures(inp, "adam", got)
    assert torch.equal(got[1]["t"], o64["t"])
    for k, (e32, ke) in figs.items():
        vc.record("fused fnn(12,4)", k, e32, ke, vc.MLP_TRAIN_TOL[k])
        assert ke <= vc.MLP_TRAIN_TOL[k], (k, ke)
    # partial against a float64 weighted sum of the trained replicas: the
    # kernel adds fp32 products with fp32 atomics, so each of a model's
    # (at most 3) terms contributes one rounding of the product and one of
    # the running sum
    reps = got[0][inp["rows"]].double()
    want = torch.zeros(K, P + 1, dtype=torch.float64)
    mag = torch.zeros(K, P + 1, dtype=torch.float64)
    sw = sample_w.double()
    want.index_add_(0, model_of, torch.cat([sw[:, None] * reps,
                                            sw[:, None]], 1))
    mag.index_add_(0, model_of, torch.cat([(sw[:, None] * reps).abs(),
                                           sw[:, None]], 1))
    part = partial.cpu().double()
    assert ((part - want).abs() <= 2 * 3 * 2.0 ** -24 * mag).all()
    assert (part[4] == 0).all()


@pytest.mark.parametrize("P", [412, 229])
@pytest.mark.parametrize("run", ["plain", "masked", "zero_total"])
def test_apply_aggregate_many_models(P, run):
    """K = 512 models in one launch with more than one wave of parameters
    per model: a wave that reads the totals slot after thread 0 drained it
    would skip its slice and still zero its slice of partial."""
    K = 512
    g = torch.Generator().manual_seed(400 + P)
    glob = torch.randn(K, P, generator=g)
    partial = torch.randn(K, P + 1, generator=g)
    partial[:, P] = torch.rand(K, generator=g) + 0.5
    mask = None
    if run == "masked":
        mask = (torch.rand(K, generator=g) > 0.4).to(torch.uint8)
    if run == "zero_total":
        partial[torch.rand(K, generator=g) > 0.6, P] = 0.0
    upd = partial[:, P] > 0
    if mask is not None:
        upd &= mask.bool()
    assert 0 < int(upd.sum()) < K or run == "plain"
    glob_d, part_d = glob.clone().to(DEV), partial.clone().to(DEV)
    totals = mlp_hip.apply_aggregate(
        glob_d, part_d, None if mask is None else mask.to(DEV))
    torch.cuda.synchronize()
    out = glob_d.cpu()
    want = partial[:, :P].double() / partial[:, P:].double()
    # partial * (1 / total) in fp32: a rounding of the reciprocal and one of
    # the product, each half an ulp; 4 x the half-ulp of an fp32 division
    err = (out.double() - want).abs()
    assert (err[upd] <= 4 * 2.0 ** -24 * want[upd].abs()).all(), \
        (err[upd] / want[upd].abs()).max()
    assert torch.equal(out[~upd], glob[~upd])        # bit-identical
    assert torch.equal(totals.cpu(), partial[:, P])
    assert part_d.abs().max().item() == 0.0, "partial must be drained"


# --------------------------------------------------------------------------
# eval / confusion / vote
# --------------------------------------------------------------------------

def _windows(d, o, seed, n_rows):
    """24 windows into 5 tasks; several share a task id, several a row."""
    x, y, g = vc.mlp_arena(d, o, seed)
    lens = torch.tensor(EVAL_LENS)
    ln = lens[torch.randint(0, len(lens), (W,), generator=g)]
    ln[:len(lens)] = lens
    off = (torch.rand(W, generator=g) * (vc.MLP_N - 700)).long()
    task_id = torch.randint(0, T, (W,), generator=g)
    task_row = torch.randint(0, n_rows, (W,), generator=g)
    return x, y, g, task_row, task_id, off, ln


def _per_sample(spec, params, x, wins, mask, dtype):
    """Padded per-sample model outputs [W, B, O] and validity [W, B]."""
    task_row, off, ln = wins
    ar = torch.arange(int(ln.max())).unsqueeze(0)
    valid = ar < ln.unsqueeze(1)
    idx = off.unsqueeze(1) + torch.minimum(ar, (ln - 1).unsqueeze(1))
    xs = x.to(dtype)[idx]
    if mask is not None:
        m = mask.to(dtype)
        xs = xs * (m.unsqueeze(1) if m.dim() == 2 else m)
    out = mlp_torch.forward_logits(spec, params.to(dtype)[task_row], xs)
    return out, valid, idx


def _near_tied(out):
    top2 = out.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) < vc.NEAR_TIE_MLP


@pytest.mark.parametrize("kind,d,o", EVAL_SHAPES)
@pytest.mark.parametrize("want_mse", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_eval_long_windows(kind, d, o, want_mse, masked):
    spec = spec_for(kind, d, o)
    M = 4
    x, y, g, task_row, task_id, off, ln = _windows(
        d, o, 500 + EVAL_SHAPES.index((kind, d, o)), M)
    params = torch.randn(M, spec.n_params, generator=g) * 0.4
    mask = (torch.rand(W, d, generator=g) > 0.4).float() if masked else None
    case = f"eval {kind}({d},{o}) mse={int(want_mse)} mask={int(masked)}"

    def ref(dtype):
        return mlp_torch.eval_tasks(
            spec, params.to(dtype), x.to(dtype), y, task_row, task_id, off,
            ln, T, want_mse=want_mse,
            x_mask=None if mask is None else mask.to(dtype))
    c64, t64, l64, m64 = ref(torch.float64)
    out64, valid, _ = _per_sample(spec, params, x, (task_row, off, ln), mask,
                                  torch.float64)
    near = _near_tied(out64) & valid
    assert near.sum().item() <= vc.NEAR_TIE_MAX_SHARE * valid.sum().item()
    near_t = torch.zeros(T, dtype=torch.float64).index_add_(
        0, task_id, near.sum(1).double())

    dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    ck, tk, lk, mk = mlp_hip.eval_tasks(
        spec, dv(params), dv(x), dv(y), dv(task_row), dv(task_id), dv(off),
        dv(ln), T, want_mse=want_mse, x_mask=dv(mask))
    torch.cuda.synchronize()
    assert torch.equal(tk.cpu(), t64), case
    assert ((ck.cpu() - c64).abs() <= near_t).all(), (case, ck, c64)
    lerr = ((lk.cpu() - l64).abs() / t64.clamp(min=1)).max().item()
    vc.record(case, "loss/sample", MLP_CE_ERR32, lerr, MLP_CE_TOL)
    assert lerr <= MLP_CE_TOL, (case, lerr)
    if want_mse:
        merr = ((mk.cpu() - m64).abs() / t64.clamp(min=1)).max().item()
        vc.record(case, "mse/sample", MLP_MSE_ERR32, merr, MLP_MSE_TOL)
        assert merr <= MLP_MSE_TOL, (case, merr)
    else:
        assert mk is None


@pytest.mark.parametrize("kind,d,o", [("fnn", 8, 5), ("lr", 4, 2)])
@pytest.mark.parametrize("mask_form", ["none", "1d", "per_window"])
def test_confusion_masks(kind, d, o, mask_form):
    spec = spec_for(kind, d, o)
    M = 4
    x, y, g, task_row, task_id, off, ln = _windows(d, o, 600 + d, M)
    params = torch.randn(M, spec.n_params, generator=g) * 0.4
    mask = None
    if mask_form != "none":
        shape = (d,) if mask_form == "1d" else (W, d)
        mask = (torch.rand(*shape, generator=g) > 0.4).float()
    ref = mlp_torch.confusion_tasks(
        spec, params.double(), x.double(), y, task_row, task_id, off, ln, T,
        o, x_mask=None if mask is None else mask.double())
    out64, valid, idx = _per_sample(spec, params, x, (task_row, off, ln),
                                    mask, torch.float64)
    near = _near_tied(out64) & valid
    assert near.sum().item() <= vc.NEAR_TIE_MAX_SHARE * valid.sum().item()
    near_ty = torch.zeros(T, o, dtype=torch.float64)
    near_ty.view(-1).index_add_(
        0, (task_id.unsqueeze(1) * o + y[idx])[valid], near[valid].double())
    dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    got = mlp_hip.confusion_tasks(
        spec, dv(params), dv(x), dv(y), dv(task_row), dv(task_id), dv(off),
        dv(ln), T, o, x_mask=dv(mask)).cpu()
    torch.cuda.synchronize()
    # every sample lands in its (task, label) row; a cell may be off by the
    # near-tied samples of that row, nowhere else
    assert torch.equal(got.sum(2), ref.sum(2))
    assert ((got - ref).abs() <= near_ty[:, :, None]).all(), (got, ref)


@pytest.mark.parametrize("kind,d,o", [("fnn", 8, 5), ("lr", 4, 2)])
@pytest.mark.parametrize("mode", ["hard", "soft"])
def test_vote_per_task_weights_with_masks(kind, d, o, mode):
    spec = spec_for(kind, d, o)
    M = 5
    x, y, g, _, task_id, off, ln = _windows(d, o, 700 + d, M)
    params = torch.randn(M, spec.n_params, generator=g) * 0.4
    weights = torch.rand(T, M, generator=g) + 0.1
    weights[:, 3] = 0.0                     # one model inactive everywhere
    masks = (torch.rand(M, d, generator=g) > 0.4).float()
    ref = mlp_torch.ens_vote_multi(
        spec, params.double(), weights.double(), x.double(), y, task_id, off,
        ln, T, mode=mode, masks=masks.double())
    # near-tied: the float64 vote totals, or (hard vote, where a member's
    # flip moves its whole weight) any active member's own outputs
    votes = torch.zeros(W, int(ln.max()), o, dtype=torch.float64)
    near = torch.zeros(W, int(ln.max()), dtype=torch.bool)
    for m in range(M):
        if m == 3:
            continue
        out, valid, _ = _per_sample(
            spec, params, x, (torch.full((W,), m), off, ln), masks[m],
            torch.float64)
        wm = weights.double()[task_id, m].reshape(W, 1, 1)
        if mode == "hard":
            near |= _near_tied(out)
            votes.scatter_add_(2, out.argmax(-1, keepdim=True),
                               wm.expand(W, votes.shape[1], 1).contiguous())
        else:
            votes += wm * torch.softmax(out, -1)
    near = (near | _near_tied(votes)) & valid
    assert near.sum().item() <= vc.NEAR_TIE_MAX_SHARE * valid.sum().item()
    near_t = torch.zeros(T, dtype=torch.float64).index_add_(
        0, task_id, near.sum(1).double())
    dv = lambda t: t.to(DEV)  # noqa: E731
    got = mlp_hip.ens_vote_multi(
        spec, dv(params), dv(weights), dv(x), dv(y), dv(task_id), dv(off),
        dv(ln), T, mode=mode, masks=dv(masks)).cpu()
    torch.cuda.synchronize()
    assert torch.equal(got[1], ref[1])
    assert ((got[0] - ref[0]).abs() <= near_t).all(), (got[0], ref[0])

    # The labels above are random, so a wrong prediction moves a count with
    # probability about 2 / O only, and rand + 0.1 weights never tie. Again
    # on windows that do not overlap, against tests/vote_cases.py: with the
    # labels the float64 specification itself predicts (every slot the
    # kernel gets wrong is one missing count), and, hard mode, with unit
    # weights, where mlp_vote_kernel's strict `>` has to send the exactly
    # tied votes to the lowest class.
    tid2, off2, ln2 = wins2 = _disjoint_windows(g)
    pos, task_of = vo.slot_index(wins2)
    outs = vo.mlp_outputs(spec, params, x, pos, masks)
    runs = [("per-task", weights, None)]
    if mode == "hard":
        ones = torch.ones(M)
        ones[3] = 0.0
        runs.append(("ones", ones, vo.MIN_TIE_SHARE_MLP))
    for name, w, min_ties in runs:
        def run(yy):
            out = mlp_hip.ens_vote_multi(
                spec, dv(params), dv(w), dv(x), dv(yy), dv(tid2), dv(off2),
                dv(ln2), T, mode=mode, masks=dv(masks))
            torch.cuda.synchronize()
            return out
        vo.check_vote(f"mlp vote {kind}({d},{o}) {mode} {name}", run, outs,
                      w, task_of, pos, y, T, mode, out_gap=vc.NEAR_TIE_MLP,
                      soft_gap=vc.NEAR_TIE_MLP, min_tie_share=min_ties)


def _disjoint_windows(g):
    """Ten windows of the EVAL_LENS lengths into 5 tasks, laid out one after
    another in shuffled order with random gaps."""
    ln = torch.tensor(EVAL_LENS + (65, 257, 1))
    off = torch.zeros(len(ln), dtype=torch.int64)
    at = 0
    for w in torch.randperm(len(ln), generator=g).tolist():
        at += int(torch.randint(0, 50, (1,), generator=g))
        off[w] = at
        at += int(ln[w])
    assert at <= vc.MLP_N
    task_id = torch.arange(len(ln)) % T
    return task_id[torch.randperm(len(ln), generator=g)], off, ln
