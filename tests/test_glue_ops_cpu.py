"""The glue-kernel entry points refuse a shape their kernel cannot take on the host, before any device work: with null
operands and no device each of these calls answers PEA_E_SHAPE (-3) with its launcher's message (as
test_abi_cpu.py::test_shape_errors_are_reported_without_gpu does for the GEMM)."""
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


def test_maps_refuse_sizes_that_are_not_whole_vectors(L):
    refused(L, L.pea_op_add(None, None, None, 12, None), b"n % 8")
    refused(L, L.pea_op_silu_fwd(None, None, 7, None), b"n % 8")
    refused(L, L.pea_op_silu_bwd(None, None, None, 9, 0, None), b"n % 8")
    refused(L, L.pea_op_gelu_fwd(None, None, 1, None), b"n % 8")
    refused(L, L.pea_op_gelu_bwd(None, None, None, 20, 1, None), b"n % 8")
    refused(L, L.pea_op_accum(None, None, 4, 1, None), b"accum: n % 8")


def test_copy2d_refuses_misaligned_rows(L):
    for ldx, ldy, C in ((40, 56, 20), (36, 56, 24), (40, 60, 24)):
        refused(L, L.pea_op_copy2d(None, ldx, None, ldy, 5, C, 0, None), b"copy2d: alignment")


def test_select_refuses_a_row_pitch_below_the_row(L):
    refused(L, L.pea_op_select_rows(None, None, None, None, 4, 616, 608, None), b"select")
    refused(L, L.pea_op_select_rows_bwd(None, None, None, None, 4, 616, 608, None), b"select")
    refused(L, L.pea_op_select_rows(None, None, None, None, 4, 12, 0, None), b"select")           # per % 8
    refused(L, L.pea_op_select_rows(None, None, None, None, 4, 16, 20, None), b"select")          # ystride % 8


def test_softmax_rows_refuses_ragged_rows(L):
    refused(L, L.pea_op_softmax_rows(None, 3, 12, 16, 1.0, None), b"softmax_rows: cols=12")
    refused(L, L.pea_op_softmax_rows(None, 3, 16, 20, 1.0, None), b"ld=20")
    refused(L, L.pea_op_softmax_rows(None, 0, 16, 16, 1.0, None), b"softmax_rows")


def test_vae_ends_refuse_channel_counts(L):
    for C2 in (3, 7, 0, 10):
        refused(L, L.pea_op_vae_posterior(None, None, None, None, None, None, 1, C2, 16, 1.0, None), b"vae posterior", b"%d moment" % C2)
    for C in (0, 9):
        refused(L, L.pea_op_vae_post_quant(None, None, None, None, 1, C, 16, 1.0, None), b"vae post_quant")


def test_residual_import_refuses_an_unknown_dtype(L):
    refused(L, L.pea_op_residual_import(None, 3, None, 1, 4, 16, 1.0, None), b"residual import: dtype 3")


def test_row_norms_refuse_rows_beyond_the_register_budget(L):
    refused(L, L.pea_op_rmsnorm_fwd(None, None, None, 2, 4104, 1e-6, None), b"rmsnorm: C=4104")
    refused(L, L.pea_op_rmsnorm_fwd(None, None, None, 2, 500, 1e-6, None), b"rmsnorm: C=500")
    refused(L, L.pea_op_layernorm_stats(None, None, 2, 4104, 1e-5, None), b"layernorm: C=4104")


def test_sumpool_and_interleaved_geglu_refuse_partial_vectors(L):
    refused(L, L.pea_op_sumpool2(None, None, 1, 2, 2, 12, 0, None), b"sumpool: C % 8")
    refused(L, L.pea_op_geglu_bwd_il(None, None, None, 5, 6, None), b"geglu: inner % 4")


def test_splitk_reduce_refuses_columns_it_would_drop(L):
    """N % 4 columns used to be dropped without a word (the kernel moves four columns per thread)"""
    refused(L, L.pea_op_splitk_reduce(None, 2, 64, None, 10, 4, 10, 0, None), b"splitk_reduce", b"N=10")
    refused(L, L.pea_op_splitk_reduce(None, 2, 64, None, 14, 4, 12, 0, None), b"ldo=14")
    refused(L, L.pea_op_splitk_reduce(None, 2, 64, None, 8, 4, 12, 0, None), b"ldo=8")            # ldo < N
    refused(L, L.pea_op_splitk_reduce(None, 2, 50, None, 12, 4, 12, 0, None), b"stride=50")
    refused(L, L.pea_op_splitk_reduce(None, 0, 64, None, 12, 4, 12, 0, None), b"nsplit=0")


def test_other_glue_refusals(L):
    refused(L, L.pea_op_colsum_batched(None, None, 1, 16, 12, 12, None, None), b"colsum_batched: C=12")
    refused(L, L.pea_op_embed_tokens(None, None, None, None, None, 1, 4, 12, 10, None), b"embed: width % 8")
    refused(L, L.pea_op_pad_head_vec(None, None, 3, 64, 40, None), b"pad_head_vec")
    refused(L, L.pea_op_nhwc_to_nchw_f32(None, None, 1, 24, 5, 4, 5, None), b"nhwc_to_nchw: depth-to-space 4 x 5 vs HW=24")
    refused(L, L.pea_op_nchw_f32_to_nhwc(None, None, 1, 24, 5, 4, 5, None), b"nchw_to_nhwc: depth-to-space")


def test_kd_loss_tmap_shares_the_refusals_of_kd_loss(L):
    import ctypes as C
    per = (C.c_longlong * 1)(12)
    arr = (C.c_void_p * 1)(None)
    refused(L, L.pea_op_kd_loss_tmap(13, arr, arr, arr, per, None, None, None, None, 16, None, None, 4, 0.1, 0, 1.0, None, None, None),
            b"ntaps=13")
    refused(L, L.pea_op_kd_loss_tmap(1, arr, arr, arr, per, None, None, None, None, 16, None, None, 4, 0.1, 0, 1.0, None, None, None),
            b"tap 0 size % 8")
    refused(L, L.pea_op_kd_loss(1, arr, arr, arr, per, None, None, None, None, 16, None, 4, 0.1, 0, 1.0, None, None, None), b"tap 0 size % 8")
