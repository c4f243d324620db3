"""upload_compress=topk HIP kernels (ops/hip/compress_kernels.hip) against
the specification (comm/compress.py), bit for bit: replica bits, residual
bits and counts, at the smallest shapes where the kernels can go wrong — row
lengths around the wave, the block stride and the switch length, the long
path forced at tiny P, its chunk and slab seams, tau in each radix digit —
and FLJob on the device. Shared bodies: tests/compress_cases.py."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import compress_cases as cc  # noqa: E402
import krum_cases as kc  # noqa: E402
import secagg_cases as sc  # noqa: E402
from feddrift_amd.comm import compress as spec  # noqa: E402
from feddrift_amd.ops import compress_hip, hip_loader  # noqa: E402

DEV = torch.device("cuda:0")
W, L = compress_hip.wave_max(), compress_hip.row_max()
C, S = compress_hip.chunk(), compress_hip.slab_rows()
CNN_P = 1199882
LONG = dict(switch=0)                      # every row takes the long path


def test_native_extension_has_the_kernels():
    mod = hip_loader.load()
    assert mod.__file__.endswith(".so")
    assert hasattr(mod, "compress_topk")
    assert W == 256 and W % 64 == 0
    assert W < L and 4 * L <= 64 * 1024    # a staged in one block's LDS
    assert C >= 256 and C % 256 == 0
    # the histogram scratch of a default slab stays small
    assert 1 <= S <= 65535 and 4 * S * int(mod.compress_bins()) <= 1 << 24
    assert int(mod.compress_bins()) == 2048


# --------------------------------------------------------------- row kernels

@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, L - 1, L])
def test_row_kernel(P):
    cc.case_shape(DEV, P)


@pytest.mark.parametrize("P", [65, 257])
def test_row_kernel_without_error_feedback(P):
    cc.case_shape(DEV, P, ef=False)


@pytest.mark.parametrize("case", [cc.case_odd_offsets, cc.case_shuffled_rows,
                                  cc.case_three_models],
                         ids=lambda f: f.__name__)
def test_row_kernel_case(case):
    case(DEV)


# ----------------------------------------------------------------- long path

@pytest.mark.parametrize("P", [65, 257])
def test_long_path_is_bit_equal_to_the_row_kernel(P):
    row = cc.case_shape(DEV, P)
    long = cc.case_shape(DEV, P, **LONG)
    for a, b in zip(row, long):
        assert np.array_equal(cc.bits(a[0]), cc.bits(b[0]))
        assert np.array_equal(cc.bits(a[1]), cc.bits(b[1]))
        assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("P", [L + 1, C - 1, C, C + 1])
def test_long_path_edges(P):
    cc.case_shape(DEV, P, **LONG)


@pytest.mark.parametrize("case", [cc.case_odd_offsets, cc.case_shuffled_rows,
                                  cc.case_three_models],
                         ids=lambda f: f.__name__)
def test_long_path_case(case):
    case(DEV, **LONG)


@pytest.mark.parametrize("slab", [1, 2])
def test_slab_seam(slab):
    """Five pairs in slabs of 1 and 2: the histogram rows are reused."""
    got = cc.case_shape(DEV, 257, n_pairs=5, ks=[26], slab=slab, **LONG)
    whole = cc.case_shape(DEV, 257, n_pairs=5, ks=[26], **LONG)
    assert np.array_equal(cc.bits(got[0][0]), cc.bits(whole[0][0]))
    assert np.array_equal(cc.bits(got[0][1]), cc.bits(whole[0][1]))


@pytest.mark.parametrize("ef", [0, 1])
def test_cnn_length_rows(ef):
    """Three pairs at the CNN's P, k = the default ratio's."""
    k = spec.keep_count(0.01, CNN_P)
    cc.case_shape(DEV, CNN_P, ef=bool(ef), ks=[k])


# ------------------------------------------- ties, zeros, non-finite, digits

@pytest.mark.parametrize("pad,over", [(0, {}), (300, {}), (0, LONG),
                                      (300, LONG)],
                         ids=["wave", "block", "long", "long-padded"])
def test_hand_written_rows(pad, over):
    cc.case_hand_rows(DEV, pad=pad, **over)


@pytest.mark.parametrize("P,over", [(65, {}), (300, {}), (300, LONG)],
                         ids=["wave", "block", "long"])
def test_integer_ties(P, over):
    cc.case_integer_ties(DEV, P, **over)


@pytest.mark.parametrize("over", [{}, LONG], ids=["row", "long"])
def test_tau_in_each_digit(over):
    cc.case_digits(DEV, **over)


# ------------------------------------------------------------ calls in a row

@pytest.mark.parametrize("P,over", [(65, {}), (300, {}), (300, LONG)],
                         ids=["wave", "block", "long"])
def test_two_calls(P, over):
    cc.case_two_calls(DEV, P, **over)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
@pytest.mark.parametrize("P,over", [(38, {}), (300, {}), (300, LONG)],
                         ids=["wave", "block", "long"])
def test_no_copy_to_the_host_in_a_steady_state_call(P, over):
    """With the plan's tensors and the scratch in place, a second call runs
    under torch's synchronisation debug mode, in which a synchronising copy
    raises."""
    bank = cc.normal((6, P), 30)
    glob = cc.normal((2, P), 31, 0.5)
    plan = compress_hip.CompressPlan(np.arange(6), np.arange(6) % 2, 2)
    g = torch.from_numpy(glob).to(DEV)
    counts = compress_hip.new_counts(2, DEV)
    k = max(1, P // 10)

    def call():
        b = torch.from_numpy(bank).to(DEV)
        e = torch.zeros_like(b)
        torch.cuda.synchronize()
        return b, e

    b1, e1 = call()
    compress_hip.topk(b1, plan, g, e1, k, counts, **over)
    b2, e2 = call()
    torch.cuda.set_sync_debug_mode("error")
    try:
        compress_hip.topk(b2, plan, g, e2, k, counts, **over)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(b1, b2) and torch.equal(e1, e2)
    want = cc.expected(bank, glob, plan.rows, plan.models,
                       np.zeros_like(bank), k)
    assert np.array_equal(cc.bits(b2), cc.bits(want[0]))
    assert np.array_equal(counts.cpu().numpy(), 2 * want[2])


# -------------------------------------------------------------------- FLJob

@pytest.mark.parametrize("ef", [0, 1])
def test_fljob_mlp_hip_round(tmp_path, ef):
    A, _ = cc.fljob_against_hand_loop(tmp_path, None, 2, ef,
                                      use_hip_kernels="always")
    assert A.device.type == "cuda"


def test_fljob_fused_path_without_a_bound_leaves_the_compressed_bits(
        tmp_path):
    """robust_fused=1, robust_norm_bound=0: the clip pass runs with an
    infinite bound for the weighted sums and rewrites no row."""
    A, _ = cc.fljob_against_hand_loop(tmp_path, None, 2, 1, robust_fused=1,
                                      use_hip_kernels="always")
    assert A.device.type == "cuda"
    assert np.all(A._clip_unbounded.cpu().numpy()[:, 0] == 0)
    assert A._clip_unbounded.cpu().numpy()[:, 1].sum() > 0


def test_fljob_median_on_device(tmp_path):
    cc.fljob_against_hand_loop(tmp_path, None, 1, 1, robust_agg="median",
                               use_hip_kernels="always")


def test_fljob_cnn_engine_round(tmp_path):
    from feddrift_amd.ops.cnn_hip import CnnHipEngine
    A, B = cc.fljob_against_hand_loop(tmp_path, None, 1, 1, make=kc.cnn_job,
                                      n_clients=4, ratio=0.01)
    assert A.device.type == "cuda"
    assert isinstance(A.mod_engine, CnnHipEngine)
    assert A.n_params == CNN_P


def test_fljob_none_is_the_plain_round(tmp_path):
    """upload_compress=none against a job built without the option: no
    residual bank, the fused partial stays in the train launch, and the
    trained rows are bit-equal. That launch adds the weighted sums with
    float atomics, so its global rows repeat only within the bound of
    secagg_cases.mean_and_bound_atomic; under the median, which has a fixed
    summation order, two rounds of global rows are bit-equal as well."""
    A = sc.make_job(tmp_path / "a", n_clients=10, upload_compress="none",
                    use_hip_kernels="always")
    B = sc.make_job(tmp_path / "b", n_clients=10, use_hip_kernels="always")
    assert A.device.type == "cuda" and A._residual is None
    assert not A._compress and not hasattr(A, "_compress_counts")
    ci = A.client_sampling(0)
    K = A.n_models
    plans = []
    for j in (A, B):
        plan = j.algo.plan(j, 0, ci)
        j.train(plan)
        assert j._partial_fused              # the fused partial stays
        plans.append(plan)
    torch.cuda.synchronize()
    assert np.array_equal(cc.bits(A.replicas), cc.bits(B.replicas))
    mean, bound, has = sc.mean_and_bound_atomic(A.replicas,
                                                plans[0].sample_num, K)
    for j, plan in zip((A, B), plans):
        j.algo.aggregate(j, 0, plan, ci)
    torch.cuda.synchronize()
    for j in (A, B):
        gp = j.global_params.double().cpu().numpy()
        for m in range(K):
            if has[m]:
                assert np.all(np.abs(gp[m] - mean[m]) <= bound[m]), m

    A = sc.make_job(tmp_path / "c", n_clients=10, upload_compress="none",
                    robust_agg="median", use_hip_kernels="always")
    B = sc.make_job(tmp_path / "d", n_clients=10, robust_agg="median",
                    use_hip_kernels="always")
    for r in range(2):
        for j in (A, B):
            plan = j.algo.plan(j, r, ci)
            j.train(plan)
            j.algo.aggregate(j, r, plan, ci)
        torch.cuda.synchronize()
        assert np.array_equal(cc.bits(A.replicas), cc.bits(B.replicas))
        assert np.array_equal(cc.bits(A.global_params),
                              cc.bits(B.global_params))
