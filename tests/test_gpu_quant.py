"""upload_compress=quant and topk_quant HIP kernels
(ops/hip/compress_kernels.hip) against the specification
(comm/compress.py:quant_rows), bit for bit: replica bits, residual bits and
counts, at the smallest shapes where the kernels can go wrong — row lengths
around the wave, the block stride and the switch length, the long path
forced at tiny P, its chunk and slab seams, the four-coordinate Philox tail —
and FLJob on the device. Shared bodies: tests/quant_cases.py."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():          # pragma: no cover
    pytest.skip("GPU only", allow_module_level=True)

import compress_cases as cc  # noqa: E402
import krum_cases as kc  # noqa: E402
import quant_cases as qc  # noqa: E402
from feddrift_amd.ops import compress_hip, hip_loader  # noqa: E402

DEV = torch.device("cuda:0")
W, L = compress_hip.wave_max(), compress_hip.row_max()
C = compress_hip.chunk()
CNN_P = 1199882
LONG = dict(switch=0)                      # every row takes the long path
KINDS = ["quant", "topk_quant"]


def same(a, b):
    assert np.array_equal(qc.bits(a[0]), qc.bits(b[0]))
    if a[1] is not None:
        assert np.array_equal(qc.bits(a[1]), qc.bits(b[1]))
    assert np.array_equal(a[2], b[2])


def test_native_extension_has_the_entry_point():
    mod = hip_loader.load()
    assert mod.__file__.endswith(".so")
    assert hasattr(mod, "compress_quant") and hasattr(mod, "compress_topk")
    assert C % 4 == 0                      # a thread's Philox block is whole


# --------------------------------------------------------------- row kernels

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nbits", [2, 8])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, L - 1, L])
def test_row_kernel(P, nbits, kind):
    qc.case_shape(DEV, P, kind, nbits)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [65, 257])
def test_row_kernel_without_error_feedback(P, kind):
    qc.case_shape(DEV, P, kind, 4, ef=False)


# ----------------------------------------------------------------- long path

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ef", [True, False])
@pytest.mark.parametrize("P", [65, 257])
def test_long_path_is_bit_equal_to_the_row_kernel(P, ef, kind):
    same(qc.case_shape(DEV, P, kind, 4, ef=ef),
         qc.case_shape(DEV, P, kind, 4, ef=ef, **LONG))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [C - 1, C, C + 1, 2 * C + 3])
def test_long_path_chunk_seams(P, kind):
    """Also the Philox tail: P % 4 is 3, 0, 1 and 3."""
    qc.case_shape(DEV, P, kind, 8, **LONG)


@pytest.mark.parametrize("kind", KINDS)
def test_slab_seam(kind):
    """Five pairs in slabs of 2: the scale slots and the histogram rows
    are reused."""
    same(qc.case_shape(DEV, 257, kind, 4, n_pairs=5, slab=2, **LONG),
         qc.case_shape(DEV, 257, kind, 4, n_pairs=5, **LONG))


@pytest.mark.parametrize("kind", KINDS)
def test_cnn_length_rows(kind):
    qc.case_shape(DEV, CNN_P, kind, 8, n_pairs=2)


# ------------------------- non-finite, zero, subnormal, FLT_MAX, the clamp

@pytest.mark.parametrize("pad,over", [(0, {}), (300, {}), (0, LONG),
                                      (300, LONG)],
                         ids=["wave", "block", "long", "long-padded"])
def test_hand_written_rows(pad, over):
    qc.case_hand_rows(DEV, pad=pad, **over)


# ------------------------------------------------------------ calls in a row

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,over", [(65, {}), (300, {}), (300, LONG)],
                         ids=["wave", "block", "long"])
def test_two_passes_and_a_large_counter(P, over, kind):
    qc.case_two_calls(DEV, P, kind, **over)


# -------------------------------------------------------------------- FLJob

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ef", [0, 1])
def test_fljob_mlp_hip_rounds(tmp_path, kind, ef):
    A, _, _ = qc.fljob_against_hand_loop(tmp_path, None, 2, kind, ef,
                                         use_hip_kernels="always")
    assert A.device.type == "cuda" and A._compress_ctr == 2


@pytest.mark.parametrize("kind", KINDS)
def test_fljob_cnn_engine_rounds(tmp_path, kind):
    from feddrift_amd.ops.cnn_hip import CnnHipEngine
    A, _, _ = qc.fljob_against_hand_loop(tmp_path, None, 2, kind, 1, nbits=8,
                                         make=kc.cnn_job, n_clients=4,
                                         ratio=0.01)
    assert A.device.type == "cuda"
    assert isinstance(A.mod_engine, CnnHipEngine)
    assert A.n_params == CNN_P


def test_topk_is_what_it_was(tmp_path):
    """The topk bodies of tests/compress_cases.py, unchanged, in the three
    regimes and through FLJob."""
    for P in (65, 257):
        cc.case_shape(DEV, P)
        cc.case_shape(DEV, P, **LONG)
    cc.case_hand_rows(DEV)
    A, _ = cc.fljob_against_hand_loop(tmp_path, None, 2, 1,
                                      use_hip_kernels="always")
    assert A.device.type == "cuda" and A.cfg.upload_compress == "topk"
