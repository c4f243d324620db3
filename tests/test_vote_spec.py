"""The torch vote paths held to the float64 specification of
tests/vote_cases.py, on a CPU and on float64 inputs, so the comparison is
exact apart from flagged near ties: mlp_torch.ens_vote_multi,
mlp_torch.ens_vote_eval and ModuleEngine.ens_vote_eval with CNN_DropOut.

This is where the vote contract is pinned without a GPU: the soft vote is
softmax of what the model returns (a second softmax for CNN_DropOut, as in
the reference), a tied vote goes to the lowest class, and a vote row of
zeros (no active model) predicts class 0. The conditions that make the GPU
cases of tests/test_gpu_cnn_vote.py sensitive are asserted here too, as
is the recorded err32 of the peaked world.
"""

import copy

import pytest
import torch

import gpu_variant_cases as vc
import vote_cases as vo
from feddrift_amd.models.packed import spec_for
from feddrift_amd.ops import mlp_torch
from feddrift_amd.ops.module_engine import ModuleEngine

# float64 paths: rounding of O(10) operations on O(1) values is below 1e-14;
# 1e-9 is a wide margin that still flags no slot of these inputs
F64_GAP = 1e-9
MLP_M, MLP_DEAD = 5, 1                  # four live voters: 2-2 ties at O = 2
MLP_SHAPES = [("fnn", 8, 5), ("lr", 4, 2)]
WKINDS = ["a", "b", "c", "zero", "zero_rows"]


def mlp_inputs(kind, d, o):
    def make():
        spec = spec_for(kind, d, o)
        x, y, g = vc.mlp_arena(d, o, 800 + d)
        # larger weights saturate lr's sigmoid and the soft vote's softmax
        # to exact 1.0, which ties member outputs exactly
        params = torch.randn(MLP_M, spec.n_params, generator=g) * 0.4
        masks = (torch.rand(MLP_M, d, generator=g) > 0.4).float()
        wins = vo.vote_windows()
        pos, task_of = vo.slot_index(wins)
        outs = {mk: vo.mlp_outputs(spec, params, x, pos,
                                   masks if mk else None)
                for mk in (False, True)}
        return dict(spec=spec, x=x, y=y, params=params, masks=masks,
                    wins=wins, pos=pos, task_of=task_of, outs=outs)
    return vo._cached(("mlp", kind, d, o), make)


def mlp_weights(wkind):
    return vo.vote_weights(wkind, M=MLP_M, dead=MLP_DEAD)


def mlp_check(inp, run, case, mode, wkind, masked, soft_gap=F64_GAP,
              sum_ulp=vo.U53):
    return vo.check_vote(
        case, run, inp["outs"][masked], mlp_weights(wkind), inp["task_of"],
        inp["pos"], inp["y"], vo.VOTE_T, mode, out_gap=F64_GAP,
        soft_gap=soft_gap, sum_ulp=sum_ulp,
        min_tie_share=vo.MIN_TIE_SHARE_MLP if (mode, wkind) == ("hard", "c")
        else None)


@pytest.mark.parametrize("kind,d,o", MLP_SHAPES)
@pytest.mark.parametrize("mode", ["hard", "soft"])
@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("masked", [False, True])
def test_mlp_torch_vote_multi(kind, d, o, mode, wkind, masked):
    inp = mlp_inputs(kind, d, o)
    tid, off, ln = inp["wins"]
    w = mlp_weights(wkind).double()
    masks = inp["masks"].double() if masked else None

    def run(y):
        return mlp_torch.ens_vote_multi(
            inp["spec"], inp["params"].double(), w, inp["x"].double(), y,
            tid, off, ln, vo.VOTE_T, mode=mode, masks=masks)
    mlp_check(inp, run, f"mlp_torch multi {kind}({d},{o}) {mode} ({wkind}) "
              f"mask={int(masked)}", mode, wkind, masked)


@pytest.mark.parametrize("kind,d,o", MLP_SHAPES)
@pytest.mark.parametrize("mode", ["hard", "soft"])
@pytest.mark.parametrize("wkind", WKINDS)
def test_mlp_torch_vote_eval(kind, d, o, mode, wkind):
    """The single-task form, one call per task. It keeps its votes in fp32
    whatever the inputs are, so the soft near-tie threshold is the fp32
    rounding of M accumulations of at most sum |w|, on either side."""
    inp = mlp_inputs(kind, d, o)
    tid, off, ln = inp["wins"]
    w = mlp_weights(wkind).double()

    def run(y):
        out = torch.zeros(2, vo.VOTE_T, dtype=torch.float64)
        for t in range(vo.VOTE_T):
            wins = [(int(o_), int(n)) for ti, o_, n in zip(tid, off, ln)
                    if int(ti) == t]
            c, n = mlp_torch.ens_vote_eval(
                inp["spec"], inp["params"].double(),
                w[t] if w.dim() == 2 else w, inp["x"].double(), y, wins,
                mode=mode, masks=inp["masks"].double())
            out[0, t], out[1, t] = c, n
        return out
    mlp_check(inp, run, f"mlp_torch eval {kind}({d},{o}) {mode} ({wkind})",
              mode, wkind, True, sum_ulp=vo.U24,
              soft_gap=2 * MLP_M * vo.U24 * float(w.abs().sum(-1).max())
              + F64_GAP)


# --------------------------------------------------------------------------
# CNN_DropOut through ModuleEngine, and the CNN cases' own conditions
# --------------------------------------------------------------------------

def small_cnn_slots():
    """A short window list out of the 257 slots of the CNN cases, unmasked:
    the first slots where a single-softmax soft vote with weights (a)
    predicts another class than the specification, and the first slots
    whose unit-weight hard vote is exactly tied, as windows of length 1
    or more (adjacent slots merge) over 3 tasks, one of them empty."""
    def make():
        pos, task_of = vo.slot_index(vo.vote_windows())
        outs = vo.vote_outputs(10, False)
        wa, wc = vo.vote_weights("a"), vo.vote_weights("c")
        soft = vo.vote_spec(outs, wa, task_of, task_of, vo.VOTE_T, "soft")
        diff = vo.single_softmax_pred(outs, wa, task_of) != soft["pred"]
        ties = vo.exact_top_ties(vo.vote_rows(outs, wc, task_of, "hard"))
        sel = torch.cat([diff.nonzero().flatten()[:6],
                         ties.nonzero().flatten()[:6]]).unique()
        p = pos[sel]
        order = p.argsort()
        sel, p = sel[order], p[order]
        wins, task = [], []
        for a in p.tolist():
            if wins and wins[-1][0] + wins[-1][1] == a:
                wins[-1][1] += 1
            else:
                wins.append([a, 1])
                task.append((0, 2)[len(wins) % 2])
        tid = torch.tensor(task)
        off = torch.tensor([w[0] for w in wins])
        ln = torch.tensor([w[1] for w in wins])
        pos2, task_of2 = vo.slot_index((tid, off, ln))
        assert torch.equal(pos2, p)
        return dict(wins=(tid, off, ln), pos=p, task_of=task_of2,
                    outs=outs[:, sel])
    return vo._cached("small cnn", make)


@pytest.mark.parametrize("mode,wkind", [("soft", "a"), ("hard", "c"),
                                        ("hard", "a"), ("soft", "zero"),
                                        ("hard", "zero")])
def test_module_engine_vote_eval(mode, wkind):
    world = vo.vote_world(10)
    s = small_cnn_slots()
    tid, off, ln = s["wins"]
    T = 3
    eng = ModuleEngine(copy.deepcopy(world["proto"]).double(),
                       world["packer"], torch.device("cpu"))
    w = vo.vote_weights(wkind).double()
    gp, x = world["gp"].double(), world["x"].double()

    def run(y):
        out = torch.zeros(2, T, dtype=torch.float64)
        for t in range(T):
            wins = [(int(o_), int(n)) for ti, o_, n in zip(tid, off, ln)
                    if int(ti) == t]
            out[0, t], out[1, t] = eng.ens_vote_eval(gp, w, x, y, wins,
                                                     mode=mode)
        return out
    res = vo.check_vote(
        f"ModuleEngine cnn {mode} ({wkind})", run, s["outs"], w, s["task_of"],
        s["pos"], world["y"], T, mode, out_gap=F64_GAP, soft_gap=F64_GAP,
        sum_ulp=vo.U53,
        min_diff=vo.MIN_SOFTMAX_DIFF if (mode, wkind) == ("soft", "a")
        else None,
        min_tie_share=vo.MIN_TIE_SHARE_CNN if (mode, wkind) == ("hard", "c")
        else None)
    assert res["spec"]["out"][1, 1] == 0


@pytest.mark.parametrize("masked", [False, True])
def test_cnn_case_conditions(masked):
    """What tests/test_gpu_cnn_vote.py relies on at O = 10, with the
    reference alone: the single-softmax vote differs on at least 5 slots
    for soft (a), at least 25 % of slots tie exactly for hard (c), and no
    more than NEAR_TIE_MAX_SHARE of any case's slots are near ties."""
    world = vo.vote_world(10)
    pos, task_of = vo.slot_index(vo.vote_windows())
    outs = vo.vote_outputs(10, masked)

    def no_run(y):
        raise AssertionError("conditions only")
    for mode in ("soft", "hard"):
        for wkind in "abc":
            vo.check_vote(
                f"cnn conditions O=10 {mode} ({wkind}) mask={int(masked)}",
                no_run, outs, vo.vote_weights(wkind), task_of, pos,
                world["y"], vo.VOTE_T, mode, out_gap=vc.NEAR_TIE_CNN,
                soft_gap=vo.SOFT_NEAR_GAP[10],
                min_diff=vo.MIN_SOFTMAX_DIFF if (mode, wkind) == ("soft", "a")
                else None,
                min_tie_share=vo.MIN_TIE_SHARE_CNN
                if (mode, wkind) == ("hard", "c") else None, arenas=())


def test_peaked_world_err32_reproduces():
    """measure_vote_err32 against the recorded constants (fp32 conv sums
    depend on the host's blocking, hence a factor of 2 either way)."""
    perr, verr = vo.measure_vote_err32(Os=(10,))[10]
    for got, rec in ((perr, vo.PEAKED_PROB_ERR32[10]),
                     (verr, vo.VOTE_ERR32[10])):
        assert rec / 2 <= got <= rec * 2, (got, rec)
