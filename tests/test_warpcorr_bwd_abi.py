"""CPU-only checks of the fused warp + correlation backward's C ABI (pwc_warp_corr81_bwd): declared, bound, and its argument
validation runs before any launch, so it answers without a device."""
import ctypes
import os

from conftest import REPO


def test_symbols_in_header_and_binding():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    for name in ("pwc_warp_corr81_bwd", "pwc_warp_corr81_bwd_workspace_bytes"):
        assert name + "(" in text
        assert name in _lib.SIGNATURES
    assert "#define PWC_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    assert _lib.load().pwc_abi_version() == 13


def test_workspace_query():
    from opticalflow_amd import _lib
    lib = _lib.load()
    # int64 grad_c2 accumulators, the two maxima, the grad_flo partial sums of the two 16-channel chunks
    assert lib.pwc_warp_corr81_bwd_workspace_bytes(16, 32, 112, 256) == 16 * 32 * 112 * 256 * 8 + 16 + 16 * 2 * 2 * 112 * 256 * 4
    assert lib.pwc_warp_corr81_bwd_workspace_bytes(16, 32, 112, 256) > 0
    for bad in ((0, 32, 112, 256), (16, 0, 112, 256), (16, 32, -1, 256), (16, 32, 112, 0)):
        assert lib.pwc_warp_corr81_bwd_workspace_bytes(*bad) == -1


def _call(lib, ptrs, B=1, C=32, H=16, W=32, flags=2, strides=None, ws_bytes=None):
    plane = H * W
    st = strides or (C * plane, C * plane, 2 * plane, 81 * plane, 81 * plane)
    need = lib.pwc_warp_corr81_bwd_workspace_bytes(max(B, 1), max(C, 1), max(H, 1), max(W, 1))
    return lib.pwc_warp_corr81_bwd(*ptrs[:8], B, C, H, W, 5.0, 0, 0.9999, 1.0, flags, 0.1, *st, ptrs[8],
                                   need if ws_bytes is None else ws_bytes, None)


def test_entry_rejects_bad_arguments_without_device():
    from opticalflow_amd import _lib
    lib = _lib.load()
    fake = [ctypes.c_void_p(4096 * (i + 1)) for i in range(9)]      # c1 c2 flo y gy gc1 gc2 gflo workspace (never dereferenced)
    for i in (0, 1, 4, 5, 6):                                         # required operands
        p = list(fake)
        p[i] = None
        assert _call(lib, p) == -1 and b"null pointer" in lib.pwc_last_error()
    p = list(fake)
    p[3] = None                                                       # y is needed for the LeakyReLU mask ...
    assert _call(lib, p) == -1
    p = list(fake)
    p[8] = None                                                       # ... and the workspace for the warp's scatter
    assert _call(lib, p) == -1
    p = list(fake)
    p[7] = None                                                       # grad_flo with a flow
    assert _call(lib, p) == -1
    for shape in ((0, 32, 16, 32), (1, 0, 16, 32), (1, 32, 0, 32), (1, 32, 16, -4)):
        B, C, H, W = shape
        assert _call(lib, fake, B, C, H, W) == -1 and b"bad shape" in lib.pwc_last_error()
    assert _call(lib, fake, strides=(8, 32 * 512, 1024, 81 * 512, 81 * 512)) == -1
    assert b"batch stride" in lib.pwc_last_error()
    assert _call(lib, fake, ws_bytes=64) == -1 and b"workspace" in lib.pwc_last_error()
    odd = list(fake)
    odd[0] = ctypes.c_void_p(4098)                                    # 2-byte aligned operand: not taken (the caller falls back)
    assert _call(lib, odd) == -2
