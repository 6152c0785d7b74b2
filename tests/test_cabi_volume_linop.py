"""C-ABI checks of the dgs_volume_*_linop entry points (include/dgs_volume.h: the *_ops entries plus
function 5, the constant-coefficient linear operator, bit 5 of the mask, with its ten coefficients
as a host pointer) that need no GPU: the names are declared and exported, the workspace sizing, and
the argument errors that return before any device work."""
import ctypes
import os
import re

import pytest

from conftest import PKG_ROOT, REPO

HEADER = os.path.join(REPO, "include", "dgs_volume.h")
LIB = os.path.join(PKG_ROOT, "diff_gaussian_sampling", "libdgs.so")
DGS_ERR_ARG, DGS_ERR_BUFFER = 1, 4
NAMES = ["dgs_volume_workspace_size_linop", "dgs_volume_forward_linop", "dgs_volume_backward_linop",
         "dgs_volume_backward_samples_linop"]
VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
F10 = ctypes.c_float * 10
COEF = F10(0.7, 0.011, -0.006, 0.009, 1.1e-4, -0.4e-4, 0.3e-4, 0.8e-4, 0.5e-4, -0.9e-4)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdgs.so is not built (python diff-gaussian-sampling_amd/build.py)")
    lib = ctypes.CDLL(LIB)
    lib.dgs_last_error.restype = ctypes.c_char_p
    return lib


def _linop_calls(lib):
    """the three calls with every pointer NULL except the coefficients, the binning and the pointer
    array: (mask, P, N, C, binning, bytes, ptrs, coef) -> rc"""
    fwd = lib.dgs_volume_forward_linop
    fwd.restype, fwd.argtypes = I, [I, VP] + [I] * 3 + [VP] * 5 + [SZ, VP, VP, I]
    bwd = lib.dgs_volume_backward_linop
    bwd.restype, bwd.argtypes = I, [I, VP] + [I] * 3 + [VP] * 6 + [SZ] + [VP] * 4 + [SZ, VP, I]
    sg = lib.dgs_volume_backward_samples_linop
    sg.restype, sg.argtypes = I, [I, VP] + [I] * 3 + [VP] * 6 + [SZ] + [VP] * 2 + [SZ, VP, I]
    ptrs = (VP * 6)()
    cf = ctypes.cast(COEF, VP)
    return (lambda m, P, N, C, b=None, n=0, p=ptrs, k=cf: fwd(m, k, P, N, C, None, None, None, None, b, n, p, None, 0),
            lambda m, P, N, C, b=None, n=0, p=ptrs, k=cf: bwd(m, k, P, N, C, None, None, None, None, p, b, n, None, None,
                                                             None, None, 0, None, 0),
            lambda m, P, N, C, b=None, n=0, p=ptrs, k=cf: sg(m, k, P, N, C, None, None, None, None, p, b, n, None, None,
                                                            0, None, 0))


def _older_calls(lib, suffix, nptr):
    """the *_ops / *_fused / *_multi calls as tests/test_cabi_volume_ops.py makes them"""
    fwd = getattr(lib, "dgs_volume_forward" + suffix)
    fwd.restype, fwd.argtypes = I, [I] * 4 + [VP] * 5 + [SZ, VP, VP, I]
    bwd = getattr(lib, "dgs_volume_backward" + suffix)
    bwd.restype, bwd.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 4 + [SZ, VP, I]
    sg = getattr(lib, "dgs_volume_backward_samples" + ("" if suffix == "_multi" else suffix))
    sg.restype, sg.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 2 + [SZ, VP, I]
    ptrs = (VP * nptr)()
    return (lambda m, P, N, C: fwd(m, P, N, C, None, None, None, None, None, 0, ptrs, None, 0),
            lambda m, P, N, C: bwd(m, P, N, C, None, None, None, None, ptrs, None, 0, None, None, None, None, 0, None, 0),
            lambda m, P, N, C: sg(m, P, N, C, None, None, None, None, ptrs, None, 0, None, None, 0, None, 0))


def test_names_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    assert re.search(r"#define\s+DGS_VOLUME_FN_OPERATOR\s+5\b", text)


def test_workspace_size(lib):
    ws, ops = lib.dgs_volume_workspace_size_linop, lib.dgs_volume_workspace_size_ops
    for f in (ws, ops):
        f.restype, f.argtypes = SZ, [I] * 5
    P, N = 10, 100
    assert ws(32, P, N, 3, 1) == N * 3 * 4  # one unique component
    assert ws(32, P, N, 9, 1) == N * 9 * 4  # the operator alone: any C
    assert ws(35, P, N, 1, 1) == N * 5 * 1 * 4  # 1 + 3 + 1
    assert ws(35, P, N, 4, 1) == N * 5 * 4 * 4
    assert ws(33, P, N, 2, 1) == N * 2 * 2 * 4 and ws(34, P, N, 2, 1) == N * 4 * 2 * 4
    for mask, C in ((32, 1), (32, 3), (32, 9), (33, 2), (35, 1), (35, 4), (7, 3), (19, 1)):
        assert ws(mask, P, N, C, 0) == 0  # the forward needs none
    assert ws(35, P, N, 5, 1) == 0  # several functions above the limit: the caller's fallback
    for mask in (0, 36, 40, 48, 64, 63, -1):
        for C in (1, 3):
            assert ws(mask, P, N, C, 1) == 0, mask
    for mask in range(1, 32):  # below 32: the *_ops sizes
        for C in (1, 3, 5):
            assert ws(mask, P, N, C, 1) == ops(mask, P, N, C, 1), (mask, C)
            assert ws(mask, P, N, C, 0) == ops(mask, P, N, C, 0) == 0
    assert ws(19, P, N, 1, 1) > 0 and ws(7, P, N, 3, 1) > 0


def test_argument_errors_before_device_work(lib):
    fake = ctypes.create_string_buffer(512)  # (never read: the calls return before any device work)
    short = ctypes.create_string_buffer(16)
    nan = F10(*([0.0] * 9 + [float("nan")]))
    inf = F10(*([float("inf")] + [0.0] * 9))
    for call in _linop_calls(lib):
        for mask in (0, 36, 40, 48, 64, 63, -1, 20):
            for C in (1, 3):
                assert call(mask, 10, 10, C, ctypes.cast(fake, VP), 512) == DGS_ERR_ARG, mask
                assert b"mask" in lib.dgs_last_error()
        for mask in (33, 34, 35):  # the operator with others above DGS_VOLUME_FUSED_MAX_C
            assert call(mask, 10, 10, 5, ctypes.cast(fake, VP), 512) == DGS_ERR_ARG
            assert b"C <= 4" in lib.dgs_last_error()
        for mask, C in ((32, 1), (32, 9), (35, 3)):  # coef NULL or not finite, before the binning is looked at
            assert call(mask, 10, 10, C, ctypes.cast(fake, VP), 512, k=None) == DGS_ERR_ARG
            assert b"coef" in lib.dgs_last_error()
            for bad in (nan, inf):
                assert call(mask, 10, 10, C, ctypes.cast(fake, VP), 512, k=ctypes.cast(bad, VP)) == DGS_ERR_ARG
                assert b"coef" in lib.dgs_last_error()
        assert call(32, 10, 10, 9) == DGS_ERR_BUFFER  # NULL binning; the operator alone takes any C
        for mask, C in ((32, 1), (32, 3), (33, 2), (35, 1), (35, 4), (7, 3), (19, 1)):
            assert call(mask, 10, 10, C) == DGS_ERR_BUFFER
            assert call(mask, 10, 10, C, ctypes.cast(short, VP), 16) == DGS_ERR_BUFFER
        assert call(7, 10, 10, 3, k=None) == DGS_ERR_BUFFER  # below 32 coef may be NULL
        assert call(35, -1, 10, 2) == DGS_ERR_ARG
        for mask, C in ((32, 3), (35, 1), (34, 4), (7, 3)):  # NULL outs / dL_douts
            assert call(mask, 10, 10, C, ctypes.cast(fake, VP), 512, None) == DGS_ERR_ARG


def test_version_is_unchanged(lib):
    lib.dgs_version.restype = I
    assert lib.dgs_version() == 12


@pytest.mark.parametrize("suffix,nptr", [("_multi", 4), ("_fused", 4), ("_ops", 5)])
def test_older_entries_still_refuse_the_operator(lib, suffix, nptr):
    """the *_multi, *_samples, *_fused and *_ops entries keep their masks"""
    ws = getattr(lib, "dgs_volume_workspace_size" + suffix)
    ws.restype, ws.argtypes = SZ, [I] * 5
    for call in _older_calls(lib, suffix, nptr):
        for C in (1, 3):
            for mask in (32, 33, 35):
                assert call(mask, 10, 10, C) == DGS_ERR_ARG
                assert b"mask" in lib.dgs_last_error()
                assert ws(mask, 10, 100, C, 1) == 0
