"""Check bodies of tests/test_gpu_round_ops.py and its child process (not
collected: no test_ prefix).

Step windows in the launch arguments: train_fused given CPU int64 step
tensors packs them into mlp_train_small_kernel's arguments; given device
tensors it reads them from memory as before. Nothing after the window read
differs, so the two launches must agree in every bit of params, m, v, vmax
and t (and of the fused partial, where a slot gets at most two addends: a
float sum of two terms does not depend on their order, one of three does).

`python tests/round_ops_cases.py CASE` runs one named case in a fresh
process (FEDDRIFT_TRAIN_BS64_MIN_G is latched once per process).
"""

import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

import fedprox_cases as fc  # noqa: E402
import gpu_variant_cases as vc  # noqa: E402
import train_chain_cases as tc  # noqa: E402

# --------------------------------------------------------------------------
# step windows in the launch arguments
# --------------------------------------------------------------------------

def train_launch(inp, optname, mu, cpu_steps, fused=None):
    """One train_fused launch; the step tensors stay on the CPU
    (`cpu_steps`) or go to the device. Returns ((params, opt), partial)."""
    from feddrift_amd.ops import mlp_hip
    dev = vc._dev()
    spec = inp["spec"]
    p = inp["params"].clone().to(dev)
    opt = fc.prox_opt(optname, inp["R"], spec.n_params, dev, torch.float32,
                      mu)
    mask = inp["mask"].to(dev) if inp["mask"] is not None else None
    kw, partial = {}, None
    if fused is not None:
        glob, model_of, sw, K = fused
        partial = torch.zeros(K, spec.n_params + 1, device=dev)
        kw = dict(in_params=glob.to(dev),
                  model_of=model_of.to(torch.int32).to(dev),
                  sample_w=sw.to(dev), partial=partial)
    st = (lambda t: t.clone()) if cpu_steps else (lambda t: t.to(dev))
    mlp_hip.train_fused(spec, p, inp["rows"].to(dev), inp["x"].to(dev),
                        inp["y"].to(dev), st(inp["off"]), st(inp["ln"]), opt,
                        x_mask=mask, **kw)
    torch.cuda.synchronize()
    got = (p.cpu(), {k: (v.cpu() if torch.is_tensor(v) else v)
                     for k, v in opt.items()})
    return got, None if partial is None else partial.cpu()


def check_inline_chain(c, lens):
    """A case of tc.chain_cases: device steps against CPU steps, bit for
    bit, and both against float64 under vc.MLP_TRAIN_TOL."""
    case, kind, d, o, optname, masked, mu, e, fused, seed = c
    inp, glob, model_of, sw = tc.case_inputs(c, lens)
    fz = (glob, model_of, sw, 3) if fused else None
    dev_got, dev_part = train_launch(inp, optname, mu, False, fz)
    cpu_got, cpu_part = train_launch(inp, optname, mu, True, fz)
    fc.assert_same_bits((case, "cpu steps"), dev_got, cpu_got)
    for name, got in (("device", dev_got), ("inline", cpu_got)):
        figs, o64, _ = fc.mlp_train_figures(inp, optname, mu, got)
        for k, (e32, ke) in figs.items():
            vc.record(f"{case} {name} steps", k, e32, ke, vc.MLP_TRAIN_TOL[k])
            assert ke <= vc.MLP_TRAIN_TOL[k], (case, name, k, ke)
        if optname == "adam":
            assert torch.equal(got[1]["t"], o64["t"]), (case, name)
    if fused:
        # K = 3 rows over 6 pairs: up to three addends per slot, so the two
        # launches' partials are held to the float64 sum (tc.check_chain's
        # bound), not to each other
        P = inp["spec"].n_params
        reps = cpu_got[0][inp["rows"]].double()
        s = sw.double()
        want = torch.zeros(3, P + 1, dtype=torch.float64)
        mag = torch.zeros(3, P + 1, dtype=torch.float64)
        want.index_add_(0, model_of, torch.cat([s[:, None] * reps,
                                                s[:, None]], 1))
        mag.index_add_(0, model_of, torch.cat([(s[:, None] * reps).abs(),
                                               s[:, None]], 1))
        for part in (dev_part, cpu_part):
            assert ((part.double() - want).abs()
                    <= 2 * 3 * 2.0 ** -24 * mag).all(), case


def inline_cases(lens, seeds):
    """Per shape: adam; shape 0 also sgd, x_mask, mu > 0 and the fused
    launch (the cases of tc.chain_cases with these settings)."""
    want = set()
    for i, (kind, d, o) in enumerate(vc.SMALL_SHAPES):
        want.add(f"chain {kind}({d},{o}) adam mask=0 mu=0")
    kind, d, o = vc.SMALL_SHAPES[0]
    want |= {f"chain {kind}({d},{o}) sgd mask=0 mu=0",
             f"chain {kind}({d},{o}) adam mask=1 mu=0",
             f"chain {kind}({d},{o}) adam mask=0 mu=0.1",
             f"chain {kind}({d},{o}) adam fused mu=0.1"}
    kind, d, o = vc.SMALL_SHAPES[3]
    want.add(f"chain {kind}({d},{o}) adam mask=1 mu=0.1")
    cases = [c for c in tc.chain_cases(lens, seeds) if c[0] in want]
    assert len(cases) == len(want), (len(cases), sorted(want))
    return cases


def check_cap(G, kind="fnn", d=3, o=2, seed=100):
    """G x 4 steps (64: at the cap of 256 entries, 65: over it, the
    binding's own upload): CPU steps and device steps give the same bits,
    the fused partial included (two pairs per model row)."""
    from feddrift_amd.ops import mlp_hip
    E = 4
    inp = vc.mlp_train_inputs(kind, d, o, tc.CHAIN_LENS, True, seed, G=G, E=E)
    inp["bcast"] = None
    spec = inp["spec"]
    assert mlp_hip.inline_steps_ok(spec, G, E) == (G * E <= 256)
    K = (G + 1) // 2
    g = torch.Generator().manual_seed(seed + 7000)
    glob = torch.randn(K, spec.n_params, generator=g) * 0.4
    model_of = torch.arange(G) // 2
    sw = torch.rand(G, generator=g) + 0.5
    sw[3] = 0.0
    start = inp["params"].clone()
    start[inp["rows"]] = 0.0
    inp = dict(inp, params=start)
    fz = (glob, model_of, sw, K)
    dev_got, dev_part = train_launch(inp, "adam", 0.0, False, fz)
    cpu_got, cpu_part = train_launch(inp, "adam", 0.0, True, fz)
    case = f"cap G={G}"
    fc.assert_same_bits(case, dev_got, cpu_got)
    assert torch.equal(dev_part, cpu_part), case
    moved = cpu_got[0][inp["rows"]] != start[inp["rows"]]
    assert moved.any(1).all(), case
    assert (cpu_part[:, -1] > 0).all(), case


def case_inline_bs256():
    for c in inline_cases(tc.CHAIN_LENS_256, tc.CHAIN_SEEDS_256):
        check_inline_chain(c, tc.CHAIN_LENS_256)
    check_cap(64)
    check_cap(65)


CASES = {"inline_bs256": case_inline_bs256}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print(f"usage: {argv[0]} {{{'|'.join(CASES)}}}")
        return 2
    CASES[argv[1]]()
    print(f"case {argv[1]} OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
