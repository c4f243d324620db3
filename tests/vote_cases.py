"""A float64 specification of the weighted ensemble vote, with the inputs,
the near-tie rule and the check body that tests/test_gpu_cnn_vote.py (the
CNN engine's `vote_multi` on the GPU), tests/test_vote_spec.py (the torch
paths, on the CPU) and the vote test of tests/test_gpu_mlp_edges.py share
(not collected: no test_ prefix).

The specification (`vote_spec`) is plain torch on the CPU and calls no
engine code:

- hard: each model adds its weight to the argmax class of its output, the
  lowest index winning a tie;
- soft: each model adds `w * softmax(output)`, where `output` is what the
  model returns. CNN_DropOut already ends in a softmax, so its soft vote
  is softmax(softmax(z)): that is what the reference's KUE vote computes
  (models/zoo.py keeps the quirk);
- a model whose weight is 0 for a task adds nothing to that task;
- the prediction is the argmax of the votes, lowest index first, so a vote
  row of zeros (no active model) predicts class 0.

Inputs that make a vote test sensitive (`vote_world`, `vote_windows`):

- the CNN worlds of gpu_variant_cases.cnn_world(O, K=4, seed=2) with the
  fc2 weight of every model multiplied by FC2_GAIN = 8, so the outputs are
  peaked and the models disagree; model DEAD has weight 0 everywhere;
- window lengths [65, 40, 64, 64, 23, 1] (257 slots), T = 5 task ids in
  shuffled order, task 2 without a window, windows that do not overlap;
- labels of two kinds: the arena's random labels, and `y_pred`, where the
  label of a slot is the specification's own prediction for it. With
  `y_pred` the expected result is correct == total, and every slot the path
  under test gets wrong is one missing count (with labels drawn at random
  over O classes a changed prediction moves the count with probability
  about 2 / O only).

Near ties (`near_slots`) are the only slack: a slot is near when rounding
of the size stated by the caller could change its prediction. None of the
thresholds derives from the error of the code under test; the constants
below are errors of fp32 torch against float64 on the same inputs,
measured on a CPU by `measure_vote_err32()` (`python tests/vote_cases.py`).
"""

import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

import gpu_variant_cases as vc  # noqa: E402

FC2_GAIN = 8.0
VOTE_M, DEAD = 4, 1
VOTE_LENS = (65, 40, 64, 64, 23, 1)
VOTE_TASKS = (3, 0, 4, 1, 0, 3)          # shuffled; task 2 has no window
VOTE_T = 5
EMPTY_TASK = 2
ZERO_ROW = 4                             # weights (b): this task's row is 0
VOTE_SLOTS = sum(VOTE_LENS)

# max |fp32 torch - float64| on the peaked worlds, per O, over the live
# models with and without masks (measure_vote_err32): the model's output
# probabilities, and the soft votes sum w * softmax(output) over weights
# (a), (b) and (c)
PEAKED_PROB_ERR32 = {10: 1.26e-6, 62: 9.42e-7}
VOTE_ERR32 = {10: 2.21e-7, 62: 3.76e-8}
# forward quantities that pass through __expf: 8 x err32 (PARITY.md)
EXPF_MARGIN = 8
PEAKED_PROB_TOL = {o: EXPF_MARGIN * e for o, e in PEAKED_PROB_ERR32.items()}
VOTE_TOL = {o: EXPF_MARGIN * e for o, e in VOTE_ERR32.items()}
# both the top and the runner-up can move by the vote bound
SOFT_NEAR_GAP = {o: 2 * t for o, t in VOTE_TOL.items()}

MIN_SOFTMAX_DIFF = 5        # soft, weights (a): single- vs double-softmax
MIN_TIE_SHARE_CNN = 0.25    # hard, weights (c): exactly tied top votes
MIN_TIE_SHARE_MLP = 0.10
U24 = 2.0 ** -24
U53 = 2.0 ** -53


# --------------------------------------------------------------------------
# the specification
# --------------------------------------------------------------------------

def slot_weights(weights, task_of, M):
    """[S, M] float64 weight of model m on slot s."""
    w = weights.detach().cpu().double()
    assert w.shape[-1] == M
    return w[task_of] if w.dim() == 2 else w[None].expand(len(task_of), M)


def vote_rows(outs, weights, task_of, mode):
    """outs [M, S, O] float64 -> votes [S, O] float64."""
    assert outs.dtype == torch.float64 and mode in ("hard", "soft")
    M, S, O = outs.shape
    ws = slot_weights(weights, task_of, M)
    votes = torch.zeros(S, O, dtype=torch.float64)
    for m in range(M):
        if mode == "hard":
            # torch.argmax returns the first maximal index
            contrib = torch.zeros(S, O, dtype=torch.float64)
            contrib.scatter_(1, outs[m].argmax(1, keepdim=True), 1.0)
        else:
            contrib = torch.softmax(outs[m], 1)
        live = ws[:, m] != 0
        votes[live] += ws[live, m, None] * contrib[live]
    return votes


def vote_spec(outs, weights, task_of, labels, T, mode):
    """-> dict(out [2, T] correct / total, pred [S], votes [S, O])."""
    votes = vote_rows(outs, weights, task_of, mode)
    pred = votes.argmax(1)
    out = torch.zeros(2, T, dtype=torch.float64)
    out[0].index_add_(0, task_of, (pred == labels).double())
    out[1].index_add_(0, task_of, torch.ones(len(task_of),
                                             dtype=torch.float64))
    return dict(out=out, pred=pred, votes=votes)


def top_gap(v):
    top2 = v.topk(2, dim=-1).values
    return top2[..., 0] - top2[..., 1]


def near_slots(outs, weights, task_of, mode, out_gap, soft_gap, sum_ulp):
    """bool [S]: slots whose prediction rounding may change.

    hard: any active model's float64 top-two output gap is below `out_gap`;
    with weights that are not all integers (sums of integers are exact)
    also a float64 vote gap below the rounding of the weight sums, M
    roundings of `sum_ulp` relative to the sum, on either side.
    soft: the float64 top-two vote gap is below `soft_gap`.
    A slot without an active model has a vote row of exact zeros and is
    never near; neither is an exact tie of integer weight sums."""
    M = outs.shape[0]
    ws = slot_weights(weights, task_of, M)
    vgap = top_gap(vote_rows(outs, weights, task_of, mode))
    if mode == "hard":
        near = ((top_gap(outs) < out_gap) & (ws.t() != 0)).any(0)
        if not bool((ws == ws.round()).all()):
            near |= vgap < 2 * M * sum_ulp * ws.abs().sum(1)
    else:
        near = vgap < soft_gap
    return near & (ws != 0).any(1)


def per_task(task_of, flags, T):
    return torch.zeros(T, dtype=torch.float64).index_add_(
        0, task_of, flags.double())


def single_softmax_pred(outs, weights, task_of):
    """argmax sum w * output: what a soft vote that takes the output of a
    model ending in a softmax as it is would predict."""
    ws = slot_weights(weights, task_of, outs.shape[0])
    return (ws.t()[:, :, None] * outs).sum(0).argmax(1)


def exact_top_ties(votes):
    return top_gap(votes) == 0


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def peak(gp, bounds):
    """Multiply the fc2 weight slice of every packed model by FC2_GAIN."""
    gp[:, bounds[6]:bounds[7]] *= FC2_GAIN
    return gp


def vote_world(O):
    def make():
        world = vc.cnn_world(O, K=VOTE_M, seed=2)
        assert world["packer"].keys[6].startswith("linear_2.w")
        peak(world["gp"], world["bounds"])
        return world
    return _cached(("world", O), make)


def vote_windows():
    """(task_id, off, ln) [6] int64: the windows of VOTE_LENS laid out one
    after another in shuffled order with random gaps, so they do not
    overlap and every offset is below CNN_N - 65."""
    def make():
        g = torch.Generator().manual_seed(7)
        ln = torch.tensor(VOTE_LENS)
        off = torch.zeros(len(ln), dtype=torch.int64)
        at = 0
        for w in torch.randperm(len(ln), generator=g).tolist():
            at += int(torch.randint(0, 11, (1,), generator=g))
            off[w] = at
            at += int(ln[w])
        assert int(off.max()) < vc.CNN_N - 65 and int(ln.min()) >= 1
        tid = torch.tensor(VOTE_TASKS)
        assert EMPTY_TASK not in VOTE_TASKS and ZERO_ROW in VOTE_TASKS
        return tid, off, ln
    return _cached("windows", make)


def slot_index(wins):
    """Arena position and task id of every slot, windows in list order."""
    tid, off, ln = wins
    pos = torch.cat([torch.arange(int(o), int(o) + int(n))
                     for o, n in zip(off, ln)])
    return pos, tid.repeat_interleave(ln)


def vote_weights(kind, M=VOTE_M, T=VOTE_T, dead=DEAD, zero_row=ZERO_ROW):
    if kind == "a":
        # no two disjoint subsets of the first four have equal sums
        w = torch.tensor([0.5, 0.8, 1.5, 0.6, 1.15])[:M - 1]
        return torch.cat([w[:dead], torch.zeros(1), w[dead:]])
    if kind == "b":
        w = torch.rand(T, M, generator=torch.Generator().manual_seed(11)) \
            + 0.1
        w[:, dead] = 0.0
        w[zero_row] = 0.0
        return w
    if kind == "c":
        w = torch.ones(M)
        w[dead] = 0.0
        return w
    if kind == "zero":
        return torch.zeros(M)
    assert kind == "zero_rows", kind
    return torch.zeros(T, M)


def vote_masks(M=VOTE_M, D=784):
    g = torch.Generator().manual_seed(13)
    return (torch.rand(M, D, generator=g) > 0.3).float()


def model_outputs(world, pos, masks, dtype):
    """[M, S, O]: every model of the world on the slots' inputs, masked per
    model as the vote masks them."""
    outs = []
    with torch.no_grad():
        for k in range(world["gp"].shape[0]):
            xs = world["x"][pos].to(dtype)
            if masks is not None:
                xs = xs * masks[k].to(dtype)
            outs.append(vc.cnn_model(world, k, dtype)(xs))
    return torch.stack(outs)


def mlp_outputs(spec, params, x, pos, masks):
    """[M, S, O] float64: what every packed MLP returns on the slots."""
    from feddrift_amd.ops import mlp_torch
    outs = []
    for m in range(params.shape[0]):
        xs = x[pos].double()
        if masks is not None:
            xs = xs * masks[m].double()
        outs.append(mlp_torch.forward_logits(
            spec, params[m:m + 1].double(), xs[None])[0])
    return torch.stack(outs)


def vote_outputs(O, masked):
    """The float64 outputs behind every CNN vote case of one (O, masked):
    computed once per process, never written to."""
    def make():
        pos, _ = slot_index(vote_windows())
        return model_outputs(vote_world(O), pos,
                             vote_masks() if masked else None, torch.float64)
    return _cached(("outs", O, masked), make)


# --------------------------------------------------------------------------
# the check body
# --------------------------------------------------------------------------

def check_vote(case, run, outs, weights, task_of, pos, y_random, T, mode,
               out_gap, soft_gap, sum_ulp=U24, min_diff=None,
               min_tie_share=None, arenas=("y_pred", "random")):
    """Hold `run(y_arena) -> [2, T]` (the path under test, on its own
    inputs) to the specification on the float64 outputs `outs`, once with
    the labels the specification itself predicts and once with y_random.

    Everything about the inputs is asserted before `run` is called."""
    S = outs.shape[1]
    assert len(pos) == S == len(task_of) and len(pos.unique()) == S
    spec = vote_spec(outs, weights, task_of, y_random[pos], T, mode)
    near = near_slots(outs, weights, task_of, mode, out_gap, soft_gap,
                      sum_ulp)
    near_t = per_task(task_of, near, T)
    vc.record(case, "near slots / slots", None, int(near.sum()) / S,
              vc.NEAR_TIE_MAX_SHARE)
    assert int(near.sum()) <= vc.NEAR_TIE_MAX_SHARE * S, (case, near.sum())
    if min_diff is not None:
        diff = single_softmax_pred(outs, weights, task_of) != spec["pred"]
        print(f"FIG {case} | single-softmax slots that differ: "
              f"{int(diff.sum())} of {S} (at least {min_diff})", flush=True)
        assert int(diff.sum()) >= min_diff, (case, int(diff.sum()))
    if min_tie_share is not None:
        ws = slot_weights(weights, task_of, outs.shape[0])
        valid = (ws != 0).any(1)
        # counted among the slots that are held exactly (not near)
        ties = exact_top_ties(spec["votes"]) & valid & ~near
        share = int(ties.sum()) / int(valid.sum())
        print(f"FIG {case} | exactly tied top votes: {share:.3f} of "
              f"{int(valid.sum())} slots (at least {min_tie_share})",
              flush=True)
        assert share >= min_tie_share, (case, share)
        # the lowest index of a tied top wins
        v = spec["votes"][ties]
        first = (v == v.max(1, keepdim=True).values).float().argmax(1)
        assert torch.equal(spec["pred"][ties], first), case
    y_pred = y_random.clone()
    y_pred[pos] = spec["pred"]
    missing = {}
    for name in arenas:
        y = y_pred if name == "y_pred" else y_random
        want = vote_spec(outs, weights, task_of, y[pos], T, mode)["out"]
        if name == "y_pred":
            assert torch.equal(want[0], want[1]), case
        got = run(y).detach().cpu()
        missing[name] = (got[0] - want[0]).abs()
        print(f"FIG {case} | {name}: correct {got[0].tolist()} want "
              f"{want[0].tolist()} total {got[1].tolist()} near "
              f"{near_t.tolist()}", flush=True)
        assert got.dtype == torch.float64 and got.shape == (2, T), case
        assert torch.equal(got[1], want[1]), (case, name, got[1], want[1])
        assert (missing[name] <= near_t).all(), \
            (case, name, got[0], want[0], near_t)
    return dict(spec=spec, near=near, missing=missing)


# --------------------------------------------------------------------------
# the CNN cases (tests/test_gpu_cnn_vote.py)
# --------------------------------------------------------------------------

def cnn_vote_run(eng, world, wins, weights, masks, mode):
    """run(y_arena) of check_vote: CnnHipEngine.vote_multi on the GPU."""
    dev = vc._dev()
    gp, x = world["gp"].to(dev), world["x"].to(dev)
    tid, off, ln = (t.to(dev) for t in wins)
    md = None if masks is None else masks.to(dev)

    def run(y):
        out = eng.vote_multi(gp, weights.to(dev), x, y.to(dev), tid, off, ln,
                             VOTE_T, mode=mode, masks=md)
        torch.cuda.synchronize()
        return out
    return run


def check_cnn_vote(case, eng, O, mode, wkind, masked, chunk_budget=None):
    world, wins = vote_world(O), vote_windows()
    pos, task_of = slot_index(wins)
    weights = vote_weights(wkind)
    masks = vote_masks() if masked else None
    run = cnn_vote_run(eng, world, wins, weights, masks, mode)
    seen = {}

    def run_both(y):
        out = run(y)
        if chunk_budget is not None:
            # cut the sweep into chunks that end inside the window list:
            # the same bits must come back
            whole = type(eng).EVAL_SLOT_BUDGET
            assert VOTE_SLOTS > 2 * chunk_budget and whole >= VOTE_SLOTS
            eng.EVAL_SLOT_BUDGET = chunk_budget
            try:
                cut = run(y)
            finally:
                del eng.EVAL_SLOT_BUDGET
            assert eng.EVAL_SLOT_BUDGET == whole
            seen["chunked"] = True
            assert torch.equal(cut, out), (case, cut, out)
        return out

    res = check_vote(
        case, run_both, vote_outputs(O, masked), weights, task_of, pos,
        world["y"], VOTE_T, mode, out_gap=vc.NEAR_TIE_CNN,
        soft_gap=SOFT_NEAR_GAP[O],
        min_diff=MIN_SOFTMAX_DIFF if (mode, wkind) == ("soft", "a") else None,
        min_tie_share=MIN_TIE_SHARE_CNN if (mode, wkind) == ("hard", "c")
        else None)
    assert chunk_budget is None or seen.get("chunked"), case
    return res


def check_cnn_no_active(case, eng, O, wkind):
    """No active model: total still counts the samples, and the all-zero
    vote row predicts class 0, in both modes."""
    world, wins = vote_world(O), vote_windows()
    pos, task_of = slot_index(wins)
    weights = vote_weights(wkind)
    want = torch.stack([per_task(task_of, world["y"][pos] == 0, VOTE_T),
                        per_task(task_of, torch.ones(len(pos)), VOTE_T)])
    assert want[0].sum() > 0 and want[1, EMPTY_TASK] == 0
    for mode in ("hard", "soft"):
        spec = vote_spec(vote_outputs(O, False), weights, task_of,
                         world["y"][pos], VOTE_T, mode)
        assert torch.equal(spec["out"], want), (case, mode)
        got = cnn_vote_run(eng, world, wins, weights, None,
                           mode)(world["y"]).cpu()
        assert torch.equal(got, want), (case, mode, got, want)


def dumped_outputs(eng, world, wins, k, mask):
    """The probabilities the dump tail stores for model k on every slot,
    as vote_multi reads them."""
    from feddrift_amd.ops.cnn_hip import EV_DUMP
    dev = vc._dev()
    tid, off, ln = (t.to(dev) for t in wins)
    chunks = []
    eng._x_arena, eng._y_arena = world["x"].to(dev), world["y"].to(dev)
    eng._eval_sweep(world["gp"].to(dev), torch.full_like(tid, k), tid, off,
                    ln, VOTE_T, EV_DUMP,
                    x_mask=None if mask is None else mask.to(dev),
                    dump_sink=lambda stid, sy, p: chunks.append(p.cpu()))
    torch.cuda.synchronize()
    return torch.cat(chunks)


def check_peaked_probs(case, eng, O, masked, wkind="a"):
    """The dump of the peaked world against float64 at 8 x its own err32
    (it is larger than the err32 behind CNN_PROB_TOL), and the soft votes
    formed from that dump in fp32 at 8 x theirs."""
    world, wins = vote_world(O), vote_windows()
    _, task_of = slot_index(wins)
    masks = vote_masks() if masked else None
    outs = vote_outputs(O, masked)
    weights = vote_weights(wkind)
    live = [k for k in range(VOTE_M) if k != DEAD]
    dump = torch.zeros(outs.shape, dtype=torch.float32)
    for k in live:
        dump[k] = dumped_outputs(eng, world, wins, k,
                                 None if masks is None else masks[k])
    perr = (dump[live].double() - outs[live]).abs().max().item()
    vc.record(case, "peaked prob", PEAKED_PROB_ERR32[O], perr,
              PEAKED_PROB_TOL[O])
    verr = (votes_fp32(dump, weights, task_of).double()
            - vote_rows(outs, weights, task_of, "soft")).abs().max().item()
    vc.record(case, "soft votes", VOTE_ERR32[O], verr, VOTE_TOL[O])
    assert perr <= PEAKED_PROB_TOL[O], (case, perr)
    assert verr <= VOTE_TOL[O], (case, verr)


def votes_fp32(out32, weights, task_of):
    """sum w * softmax(output) accumulated in fp32, model by model."""
    M, S, O = out32.shape
    ws = slot_weights(weights, task_of, M).float()
    votes = torch.zeros(S, O)
    for m in range(M):
        if bool((ws[:, m] != 0).any()):
            votes += ws[:, m, None] * torch.softmax(out32[m], 1)
    return votes


# --------------------------------------------------------------------------
# err32 of the peaked worlds (CPU only)
# --------------------------------------------------------------------------

def measure_vote_err32(Os=(10, 62)):
    """-> {O: (prob err32, vote err32)}, the constants PEAKED_PROB_ERR32
    and VOTE_ERR32, with the near-tie and sensitivity figures of every
    case printed."""
    res = {}
    pos, task_of = slot_index(vote_windows())
    live = [k for k in range(VOTE_M) if k != DEAD]
    for O in Os:
        perr = verr = 0.0
        for masked in (False, True):
            outs = vote_outputs(O, masked)
            o32 = model_outputs(vote_world(O), pos,
                                vote_masks() if masked else None,
                                torch.float32)
            e = (o32[live].double() - outs[live]).abs().max().item()
            perr = max(perr, e)
            print(f"O={O} mask={int(masked)} prob err32={e:.3e}")
            for wkind in "abc":
                w = vote_weights(wkind)
                v64 = vote_rows(outs, w, task_of, "soft")
                e = (votes_fp32(o32, w, task_of).double() - v64) \
                    .abs().max().item()
                verr = max(verr, e)
                valid = (slot_weights(w, task_of, VOTE_M) != 0).any(1)
                soft = vote_spec(outs, w, task_of, task_of, VOTE_T, "soft")
                hard = vote_spec(outs, w, task_of, task_of, VOTE_T, "hard")
                diff = single_softmax_pred(outs, w, task_of) != soft["pred"]
                ties = exact_top_ties(hard["votes"]) & valid
                near_s = near_slots(outs, w, task_of, "soft", vc.NEAR_TIE_CNN,
                                    SOFT_NEAR_GAP[O], U24)
                near_h = near_slots(outs, w, task_of, "hard", vc.NEAR_TIE_CNN,
                                    SOFT_NEAR_GAP[O], U24)
                print(f"O={O} mask={int(masked)} weights ({wkind}): vote "
                      f"err32={e:.3e}, min soft gap="
                      f"{top_gap(soft['votes'])[valid].min().item():.3e}, "
                      f"near soft {int(near_s.sum())} hard "
                      f"{int(near_h.sum())}, single-softmax differs on "
                      f"{int(diff.sum())}, hard exact ties "
                      f"{int(ties.sum())} of {int(valid.sum())}")
        res[O] = (perr, verr)
        print(f"O={O}: PEAKED_PROB_ERR32={perr:.3e} VOTE_ERR32={verr:.3e}")
    return res


if __name__ == "__main__":
    measure_vote_err32()
