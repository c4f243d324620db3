"""Check bodies of tests/test_train_chain_spec.py (CPU) and
tests/test_gpu_train_chain.py (HIP), and the child process of the
256-thread small train kernel (not collected: no test_ prefix).

mlp_train_small_kernel sums an entry's 64 per-lane partials with a wave
reduce-scatter whose result has to equal, bit for bit, the shuffle-down tree
it replaced: level s = 32, 16, ..., 1 adds v[i] + v[i + s] for i < s.
`tree_reduce` is that tree in numpy float32, `scatter_reduce` the butterfly
as the kernel routes it (entry p ends in lane bitrev6(p)); `probe_inputs`
are the two draws the GPU probe runs on.

The end-to-end cases reuse vc.mlp_train_inputs and the bounds
vc.MLP_TRAIN_TOL. Their step lengths cross the kernel's prefetch bound
(8 trips of the block: 512 samples at 64 threads, 2048 at 256; the
256-thread lengths cross the block's stride instead), and zero-length steps
come first, last and twice in a row. Seeds follow the rule of
tests/gpu_variant_cases.py: the first seed from 100 + shape index on whose
draws fp32 torch resolves every case (err32 <= 1e-5, `measure_err32()`, CPU
only); nothing else selects them.

`python tests/train_chain_cases.py CASE` runs one named case in a fresh
process (FEDDRIFT_TRAIN_BS64_MIN_G is latched once per process).
"""

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

import fedprox_cases as fc  # noqa: E402
import gpu_variant_cases as vc  # noqa: E402
from feddrift_amd.models.packed import spec_for  # noqa: E402

# --------------------------------------------------------------------------
# the wave reduce
# --------------------------------------------------------------------------

PROBE_TPS = (6, 8, 22, 38, 58)     # TP of the five template shapes


def shape_tps():
    return tuple(spec_for(k, d, o).n_params for k, d, o in vc.SMALL_SHAPES)


def bitrev6(p):
    return int(f"{p:06b}"[::-1], 2)


def tree_reduce(vals):
    """The shuffle-down tree of one wave on vals [64, TP], float32: lane 0's
    totals."""
    v = np.array(vals, dtype=np.float32, copy=True)
    s = 32
    while s:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    return v[0].copy()


def scatter_reduce(vals):
    """The butterfly as the kernel routes it, lane by lane in float32. At
    level s a lane keeps the entries whose next bit equals its own bit s and
    adds its partner's (lane ^ s) partial to its own. Returns out[p] as held
    by lane bitrev6(p), and asserts that no other lane ends with entry p."""
    vals = np.asarray(vals, dtype=np.float32)
    tp = vals.shape[1]
    held = [{p: vals[l, p] for p in range(tp)} for l in range(64)]
    bit = 0
    for s in (32, 16, 8, 4, 2, 1):
        nxt = []
        for l in range(64):
            mine = 1 if l & s else 0
            keep = {}
            for p, v in held[l].items():
                if (p >> bit) & 1 == mine:
                    keep[p] = np.float32(v + held[l ^ s][p])
            nxt.append(keep)
        held = nxt
        bit += 1
    out = np.zeros(tp, dtype=np.float32)
    for l in range(64):
        assert set(held[l]) <= {bitrev6(l)}, (l, held[l])
        for p, v in held[l].items():
            out[p] = v
    assert sum(len(h) for h in held) == tp
    return out


def left_to_right(vals):
    v = np.asarray(vals, dtype=np.float32)
    acc = np.zeros(v.shape[1], dtype=np.float32)
    for l in range(64):
        acc = acc + v[l]
    return acc


def probe_inputs(tp, seed=0):
    """(order-sensitive draw, routing case), both [64, TP] float32. The draw
    is randn x 10^U[-6, 6]: sums of such terms depend on their order. The
    routing case 64 p + l is exact in float32 whatever the order (all sums
    stay below 2^24), and an entry delivered to the wrong lane, or summed
    over the wrong lanes, misses 64 * 64 p + 2016."""
    rng = np.random.default_rng(1000 * tp + seed)
    wide = (rng.standard_normal((64, tp))
            * 10.0 ** rng.uniform(-6, 6, (64, tp))).astype(np.float32)
    route = (64.0 * np.arange(tp)[None, :]
             + np.arange(64)[:, None]).astype(np.float32)
    return wide, route


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32),
                          np.asarray(b, np.float32).view(np.uint32))


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------

G, E = 6, 4
CHAIN_LENS = (0, 1, 64, 511, 512, 513, 600)         # 64-thread blocks
CHAIN_LENS_256 = (0, 1, 255, 256, 257, 600, 2100)   # 256-thread blocks
MUS = (0.0, 0.1)


def step_table(lens):
    """[G, E] lengths: every length occurs; pair 0 starts with a zero-length
    step, pair 1 ends with one, pair 2 has two in a row, pair 5 is all
    zeros but one step."""
    z, a = lens[0], list(lens[1:])
    assert z == 0 and len(a) >= 5
    t = [[0, a[-1], a[-2], a[-3]],
         [a[-3], a[1], a[0], 0],
         [a[-1], 0, 0, a[-2]],
         [a[0], a[-1], a[-3], a[-4]],
         [a[-4], a[-2], a[1], a[-1]],
         [0, a[2], 0, 0]]
    t = torch.tensor(t)
    assert set(t.view(-1).tolist()) == set(lens)
    return t


def chain_inputs(kind, d, o, lens, masked, seed, e=E):
    inp = vc.mlp_train_inputs(kind, d, o, lens, masked, seed, G=G, E=E)
    inp["ln"] = step_table(lens)[:, :e].contiguous()
    inp["off"] = inp["off"][:, :e].contiguous()
    inp["bcast"] = None
    return inp


def fused_parts(inp, seed):
    """Fused broadcast and partial: K = 3 global rows, one sample_w = 0."""
    P = inp["spec"].n_params
    g = torch.Generator().manual_seed(seed + 7000)
    glob = torch.randn(3, P, generator=g) * 0.4
    model_of = torch.tensor([0, 1, 2, 0, 1, 0])
    sw = torch.rand(G, generator=g) + 0.5
    sw[3] = 0.0
    start = inp["params"].clone()
    start[inp["rows"]] = 0.0       # the kernel stages from in_params instead
    return dict(inp, params=start, bcast=(glob, model_of)), glob, model_of, sw


# first seed from 100 + i that passes the err32 rule (measure_err32())
CHAIN_SEEDS = (100, 101, 102, 103, 104)
CHAIN_SEEDS_256 = (100, 101, 102, 103, 104)
ERR32_MAX = 1e-5


def chain_cases(lens, seeds):
    """(case, kind, d, o, optname, masked, mu, e, fused, seed)"""
    for i, (kind, d, o) in enumerate(vc.SMALL_SHAPES):
        for optname in ("sgd", "adam"):
            for masked in (False, True):
                for mu in MUS:
                    yield (f"chain {kind}({d},{o}) {optname} "
                           f"mask={int(masked)} mu={mu:g}", kind, d, o,
                           optname, masked, mu, E, False, seeds[i])
            yield (f"chain {kind}({d},{o}) {optname} E=1", kind, d, o,
                   optname, False, 0.0, 1, False, seeds[i])
            yield (f"chain {kind}({d},{o}) {optname} fused mu=0.1", kind, d,
                   o, optname, True, 0.1, E, True, seeds[i])


def case_inputs(c, lens):
    case, kind, d, o, optname, masked, mu, e, fused, seed = c
    inp = chain_inputs(kind, d, o, lens, masked, seed, e)
    if fused:
        return fused_parts(inp, seed)
    return inp, None, None, None


def measure_err32(lens=CHAIN_LENS, seeds=CHAIN_SEEDS):
    """Largest err32 per case (CPU only): the seed rule's figure."""
    worst = {}
    for c in chain_cases(lens, seeds):
        inp = case_inputs(c, lens)[0]
        figs = fc.mlp_train_figures(inp, c[4], c[6])[0]
        worst[c[0]] = max(e32 for e32, _ in figs.values())
        print(f"{c[0]} seed={c[-1]} err32={worst[c[0]]:.3e}")
    return worst


def check_chain(c, lens):
    """One launch against float64 under vc.MLP_TRAIN_TOL; untouched rows
    keep their bits; a second launch on equal inputs gives equal bits."""
    case, kind, d, o, optname, masked, mu, e, fused, seed = c
    inp, glob, model_of, sw = case_inputs(c, lens)
    dev = vc._dev()
    P = inp["spec"].n_params

    def run():
        kw = {}
        partial = None
        if fused:
            partial = torch.zeros(3, P + 1, device=dev)
            kw = dict(in_params=glob.to(dev),
                      model_of=model_of.to(torch.int32).to(dev),
                      sample_w=sw.to(dev), partial=partial)
        got = fc.mlp_train_hip(inp, optname, mu, **kw)
        return got, None if partial is None else partial.cpu()

    got, partial = run()
    figs, o64, _ = fc.mlp_train_figures(inp, optname, mu, got)
    for k, (e32, ke) in figs.items():
        vc.record(case, k, e32, ke, vc.MLP_TRAIN_TOL[k])
    rest = torch.ones(inp["R"], dtype=torch.bool)
    rest[inp["rows"]] = False
    assert torch.equal(got[0][rest], inp["params"][rest]), case
    if optname == "adam":
        # zero-length steps skip without advancing t; rows outside `rows`
        # keep their (zero) state
        assert torch.equal(got[1]["t"], o64["t"]), (case, got[1]["t"])
        want_t = (inp["ln"] > 0).sum(1).to(torch.int32)
        assert torch.equal(got[1]["t"][inp["rows"]], want_t), case
        for k in ("m", "v", "vmax"):
            assert not got[1][k][rest].any(), (case, k)
    for k, (e32, ke) in figs.items():
        assert e32 <= ERR32_MAX, (case, k, e32)
        assert ke <= vc.MLP_TRAIN_TOL[k], (case, k, ke, vc.MLP_TRAIN_TOL[k])
    if fused:
        # partial against the float64 weighted sum of the trained replicas
        # (the bound of test_fused_broadcast_and_partial: at most 3 terms)
        reps = got[0][inp["rows"]].double()
        want = torch.zeros(3, P + 1, dtype=torch.float64)
        mag = torch.zeros(3, P + 1, dtype=torch.float64)
        s = sw.double()
        want.index_add_(0, model_of, torch.cat([s[:, None] * reps,
                                                s[:, None]], 1))
        mag.index_add_(0, model_of, torch.cat([(s[:, None] * reps).abs(),
                                               s[:, None]], 1))
        assert ((partial.double() - want).abs()
                <= 2 * 3 * 2.0 ** -24 * mag).all(), case
    again, _ = run()
    fc.assert_same_bits((case, "second launch"), got, again)


def check_carried_rows(kind, d, o, lens, seed):
    """Non-zero Adam state and a rate per row carried into the launch
    (vc.seeded_opt_state): rows outside `rows` keep every bit of params, m,
    v, vmax and t, and two launches agree bit for bit."""
    from feddrift_amd.ops import mlp_hip
    dev = vc._dev()
    inp = chain_inputs(kind, d, o, lens, True, seed)
    spec = inp["spec"]
    g = torch.Generator().manual_seed(seed + 9000)
    opt0 = vc.seeded_opt_state("adam", inp["R"], spec.n_params, g)
    x, y = inp["x"].to(dev), inp["y"].to(dev)
    L = dict(rows=inp["rows"], off=inp["off"], ln=inp["ln"], mask=inp["mask"])
    outs = []
    for _ in range(2):
        p = inp["params"].clone().to(dev)
        opt = vc.opt_to(opt0, dev, torch.float32)
        vc.launch(mlp_hip, spec, p, opt, x, y, L)
        outs.append(vc.snapshot(p, opt))
    before = vc.snapshot(inp["params"], opt0)
    rest = torch.ones(inp["R"], dtype=torch.bool)
    rest[inp["rows"]] = False
    case = f"chain carried {kind}({d},{o})"
    for k in ("param", "m", "v", "vmax", "t", "lr"):
        assert torch.equal(outs[0][k], outs[1][k]), (case, k)
        assert torch.equal(outs[0][k][rest], before[k][rest]), (case, k)
    want_t = before["t"][inp["rows"]] + (inp["ln"] > 0).sum(1).to(torch.int32)
    assert torch.equal(outs[0]["t"][inp["rows"]], want_t), case
    moved = outs[0]["param"][inp["rows"]] != before["param"][inp["rows"]]
    assert moved.any(1).all(), case


def case_chain_bs256():
    """Every 256-thread case, on whatever block size the process was
    started for (the child sets FEDDRIFT_TRAIN_BS64_MIN_G huge)."""
    for c in chain_cases(CHAIN_LENS_256, CHAIN_SEEDS_256):
        check_chain(c, CHAIN_LENS_256)
    for i, (kind, d, o) in enumerate(vc.SMALL_SHAPES):
        check_carried_rows(kind, d, o, CHAIN_LENS_256, CHAIN_SEEDS_256[i])


CASES = {"chain_bs256": case_chain_bs256}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print(f"usage: {argv[0]} {{{'|'.join(CASES)}}}")
        return 2
    CASES[argv[1]]()
    print(f"case {argv[1]} OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
