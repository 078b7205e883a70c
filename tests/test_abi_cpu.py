"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol
include/pea_hip.h declares (no compute call is made without a GPU), and the product path refuses
to run without the HIP extension or a device (no CPU fallback)."""
import ctypes
import os

import pytest

from pea_diffusion_amd import _lib


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_parses_and_all_symbols_exported(built):
    protos = _lib.parse_header()
    assert len(protos) >= 25
    for name in protos:
        assert hasattr(built, name), f"libpea_hip.so does not export {name}"
    for must in ["pea_op_gemm", "pea_op_conv3x3", "pea_op_attention_fwd", "pea_op_attention_bwd", "pea_op_kd_loss",
                 "pea_op_groupnorm_fwd", "pea_op_layernorm_bwd", "pea_last_error"]:
        assert must in protos


def test_library_has_gfx950_code_object():
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"gemm_lcp_kernel" in data


def test_version_and_error_string(built):
    L = _lib.lib()
    assert L.pea_version() >= 100
    assert isinstance(L.pea_last_error(), bytes)


def test_shape_errors_are_reported_without_gpu():
    L = _lib.lib()
    # K not a multiple of 64 is rejected before any device work
    rc = L.pea_op_gemm(None, 8, None, 8, None, 8, 4, 4, 10, 1.0, None, None, 0, 1, 0, None, 0, None, 0, 0, 0, None)
    assert rc == -3 and b"K=10" in L.pea_last_error()


def test_attention_mask_refusals_without_gpu():
    """The attention launchers refuse what no kernel implements before any launch (null operands, no device): a key-length mask
    at a head width other than 64 in the backward, like the forward's own refusal.  A causal mask or a score bias in the
    backward is refused by launch_attention_bwd as well, but no exported entry point can ask for one (pea_op_attention_bwd_masked
    has no such argument), and pea_op_attention_fwd_masked / _text fix nd = 1, so those two refusals are not reachable from
    here; what is reachable is that the masked entries get as far as the launcher's checks and answer PEA_E_SHAPE."""
    import ctypes as C
    L = _lib.lib()
    kv = C.cast((C.c_int * 2)(1, 1), C.c_void_p)                     # never read: the call is refused on the host
    for nd in (2, 3):
        rc = L.pea_op_attention_bwd_masked(None, 64 * nd, None, 64 * nd, None, 64 * nd, None, 64 * nd, None, 64 * nd, None, None,
                                           None, 64 * nd, None, 64 * nd, None, 64 * nd, 2, 1, 8, 8, 0.125, 0, 0, nd, None, 0, kv, None)
        assert rc == -3 and b"key-length masks need head_dim 64" in L.pea_last_error(), L.pea_last_error()
    # without kv_len the same call gets past that check (and is stopped by the next one: no operands)
    rc = L.pea_op_attention_bwd_masked(None, 128, None, 128, None, 128, None, 128, None, 128, None, None,
                                       None, 128, None, 128, None, 128, 2, 1, 8, 8, 0.125, 0, 0, 2, None, 0, None, None)
    assert rc == -3 and b"lse/delta/dO/O required" in L.pea_last_error(), L.pea_last_error()
    # nd = 1 with kv_len: not refused for the mask
    rc = L.pea_op_attention_bwd_masked(None, 64, None, 64, None, 64, None, 64, None, 64, None, None,
                                       None, 64, None, 64, None, 64, 2, 1, 8, 8, 0.125, 0, 0, 1, None, 0, kv, None)
    assert rc == -3 and b"lse/delta/dO/O required" in L.pea_last_error(), L.pea_last_error()
    # the forward entries: an empty problem is refused by the launcher's first check, masks or not
    rc = L.pea_op_attention_fwd_masked(None, 64, None, 64, None, 64, None, 64, None, 2, 1, 0, 8, 0.125, 1, kv, None)
    assert rc == -3 and b"empty problem" in L.pea_last_error()
    rc = L.pea_op_attention_fwd_text(None, 64, None, 64, None, 64, None, 64, None, 2, 1, 8, 0, 0.125, 0, 1, kv, None, None)
    assert rc == -3 and b"empty problem" in L.pea_last_error()
    rc = L.pea_op_attention_fwd_text(None, 60, None, 64, None, 64, None, 64, None, 2, 1, 8, 8, 0.125, 0, 1, kv, None, None)
    assert rc == -3 and b"multiples of 8" in L.pea_last_error()


def test_unet_plan_runs_without_a_device():
    """pea_unet_plan: the host-side tape builder + memory planner needs no GPU (known answer: SDXL parameter total)"""
    import ctypes as C
    from pea_diffusion_amd import config as pc
    L = _lib.lib()
    c = pc.to_c(pc.sdxl_config())
    n_ops, n_w, npar, wb, ab, gb = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
    assert L.pea_unet_plan(C.byref(c), 4, 128, 128, 77, 1, C.byref(n_ops), C.byref(n_w), C.byref(npar), C.byref(wb),
                           C.byref(ab), C.byref(gb)) == 0
    assert npar.value == 2_567_463_684 and n_ops.value > 800 and ab.value > gb.value > 10e9
    c2 = pc.to_c(pc.ssd1b_config())
    assert L.pea_unet_plan(C.byref(c2), 4, 128, 128, 77, 1, None, None, C.byref(npar), None, None, None) == 0
    assert npar.value == 1_300_195_844


def test_host_runtime_under_asan():
    """SURVEY 5 sanitizer row: the host half of every translation unit built with -fsanitize=address
    (--offload-host-only; GPU ASAN is unavailable on this pool) and driven through the C ABI's error paths and the
    tape builder / planner by tests/abi_asan_driver.c."""
    import subprocess
    r = subprocess.run(["make", "-C", _lib.CSRC, "-j8", "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(_lib.CSRC, "build_asan", "abi_asan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert r.returncode == 0 and "all host checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr


def test_scratch_plan_runs_without_a_device():
    """pea_unet_plan_scratch (round 5): what a context allocates beside its arenas, host only.  A dead-row context (B + n_t
    samples, the same bwd_batch) never needs more of any buffer class in total than the 2B merged context it borrows from; an
    inference context needs only the GroupNorm partials."""
    import ctypes as C
    from pea_diffusion_amd import config as pc
    L = _lib.lib()
    c = pc.to_c(pc.sdxl_config())

    def scratch(B, flags, bwd):
        v = C.c_longlong()
        assert L.pea_unet_plan_scratch(C.byref(c), B, 128, 128, 77, flags, bwd, C.byref(v)) == 0, L.pea_last_error()
        return v.value
    full, dre, infer = scratch(8, 1, 4), scratch(6, 1, 4), scratch(8, 0, 0)
    assert 0.3e9 < full < 4e9, full                    # the FF d(pre-activation) buffer alone is 4 x 4096 x 10240 x 2 bytes
    assert dre <= full
    assert 0 < infer < 64e6 and infer < full
    assert L.pea_unet_plan_scratch(C.byref(c), 8, 128, 128, 77, 1, 4, None) == -1       # NULL output: argument error, not a crash


def test_stacked_grad_entry_points_reject_null_handles():
    import ctypes as C
    L = _lib.lib()
    rows, cols = C.c_longlong(), C.c_int()
    assert L.pea_unet_stacked_grad(None, 0, None, C.byref(rows), C.byref(cols), None) == -1
    assert L.pea_unet_stacked_layout(None, 0, 0, None, 0, None, None) == -1
    assert L.pea_trainer_backward_context(None, None) == -1



def test_clean_build_from_sources_only(tmp_path):
    """`build()` proven from clean every round: the sources (csrc/*.hip, *.h, the Makefile, include/pea_hip.h) copied to an empty
    directory -- no .o, no .so -- compile for gfx950 with the Makefile's own flags and link, warnings stay at the one known
    unroll remark, and the fresh library exports exactly the header's prototypes.  (The tree the driver's build() runs in
    carries prebuilt objects, so there `make` is a dependency check; this is the full compile, ~1-2 min on 8 cores.)"""
    import glob
    import shutil
    import subprocess
    root = _lib.ROOT
    csrc = tmp_path / "pea_diffusion_amd" / "csrc"
    csrc.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(root, "include", "pea_hip.h"), tmp_path / "include" / "pea_hip.h")
    for f in glob.glob(os.path.join(_lib.CSRC, "*.hip")) + glob.glob(os.path.join(_lib.CSRC, "*.h")) + [os.path.join(_lib.CSRC, "Makefile")]:
        shutil.copy(f, csrc / os.path.basename(f))
    assert not list(csrc.glob("*.o"))
    r = subprocess.run(["make", "-C", str(csrc), "-j8"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    warnings = [ln for ln in r.stderr.splitlines() if "warning:" in ln]
    assert len(warnings) <= 2 and all("loop not unrolled" in w for w in warnings), warnings[:10]
    so = tmp_path / "pea_diffusion_amd" / "libpea_hip.so"
    assert so.exists() and so.stat().st_size > 3_000_000
    L = ctypes.CDLL(str(so))
    protos = _lib.parse_header(str(tmp_path / "include" / "pea_hip.h"))
    for name in protos:
        assert hasattr(L, name), f"clean build does not export {name}"
    nm = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T pea_" in ln}
    assert exported == set(protos), (sorted(exported - set(protos)), sorted(set(protos) - exported))


def test_training_plan_refuses_attention_token_counts_the_backward_cannot_take():
    """an SD1.5 UNet at a 56 x 104 latent has a 7 x 13 = 91-token mid block: the attention backward needs query counts in
    multiples of 4, so a training plan (PEA_UNET_GRAD) is refused when it is built; the inference plan is not"""
    import ctypes as C
    from pea_diffusion_amd import config as pc
    L = _lib.lib()
    c = pc.to_c(pc.sd15_config())
    assert L.pea_unet_plan(C.byref(c), 1, 56, 104, 77, 1, None, None, None, None, None, None) != 0
    assert b"91 tokens" in L.pea_last_error()
    assert L.pea_unet_plan(C.byref(c), 1, 56, 104, 77, 0, None, None, None, None, None, None) == 0
    assert L.pea_unet_plan(C.byref(c), 1, 64, 104, 77, 1, None, None, None, None, None, None) == 0      # 8 x 13 = 104 tokens
