"""The entries for the GEMM / conv forms that only the model tape fills (tests/test_gemm_forms_gpu.py) refuse, on the host and
before any device work, what their kernels would get wrong: with null operands and no device each of these calls answers
PEA_E_SHAPE (-3) with the launcher's message, as the glue entries do in tests/test_glue_ops_cpu.py."""
import pytest

from pea_diffusion_amd import _lib


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def refused(L, rc, *needles):
    msg = L.pea_last_error()
    assert rc == -3, (rc, msg)
    for n in needles:
        assert n in msg, msg


def splitk(L, M, N, K, ldc, stride, ksplit=2):
    return L.pea_op_gemm_splitk(None, K, None, K, None, ldc, stride, M, N, K, 1.0, ksplit, None)


def test_splitk_refuses_partials_that_overlap_or_misalign(L):
    M, N, K, ldc = 154, 136, 512, 140
    least = (M - 1) * ldc + N                                       # 21556: the last element of a partial, plus one
    refused(L, splitk(L, M, N, K, ldc, least - 4), b"split-K split_stride=21552", b"overlap")
    refused(L, splitk(L, M, N, K, ldc, 0), b"split_stride=0")
    refused(L, splitk(L, M, N, K, ldc, M * ldc + 6), b"split_stride=21566", b"alignment")
    refused(L, splitk(L, M, N, K, ldc, M * ldc + 8, ksplit=1), b"gemm_splitk: ksplit=1")


def test_tanh_geglu_refuses_the_gradient_form_stash(L):
    refused(L, L.pea_op_gemm_geglu_tanh(None, 128, None, 128, None, None, None, 16, 32, 128, 1, 0, 1, None), b"geglu_tanh", b"erf gate only")


def test_conv_ex_refuses_odd_sides_under_pad_off(L):
    for Hs, Ws in ((7, 12), (8, 11), (5, 5)):
        refused(L, L.pea_op_conv3x3_ex(None, None, 576, None, 64, 1, Hs, Ws, 64, 64, 2, 1, 0, None, None, 0, None),
                b"conv3x3_ex: pad_off", b"Hs=%d Ws=%d" % (Hs, Ws))
    refused(L, L.pea_op_conv3x3_ex(None, None, 576, None, 64, 1, 8, 12, 64, 64, 1, 1, 0, None, None, 0, None), b"pad_off", b"stride=1")


def test_conv_ex_refuses_rows_narrower_than_the_output(L):
    refused(L, L.pea_op_conv3x3_ex(None, None, 576, None, 24, 2, 16, 24, 64, 32, 2, 0, 2, None, None, 0, None), b"conv3x3_ex: ldc=24", b"Cout=32")
    refused(L, L.pea_op_conv3x3_ex(None, None, 512, None, 64, 2, 16, 24, 64, 32, 2, 0, 2, None, None, 0, None), b"ldw=512 vs 9*Cin=576")
    refused(L, L.pea_op_conv3x3_ex(None, None, 576, None, 64, 2, 16, 24, 64, 32, 1, 0, 4, None, None, 0, None), b"act=4")


def test_pack_conv_padded_refuses_a_stored_width_below_the_real_one(L):
    refused(L, L.pea_op_pack_conv_padded(None, None, 16, 32, 16, None), b"pack_conv_padded", b"stored as 16")
