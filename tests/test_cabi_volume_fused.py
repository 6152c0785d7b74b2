"""C-ABI checks of the fused D = 3 entry points for multi-channel fields (include/dgs_volume.h,
dgs_volume_*_fused: several functions at 2 <= C <= DGS_VOLUME_FUSED_MAX_C in one walk) that need
no GPU: the names are declared and exported, the workspace sizing, and the argument errors that
return before any device work."""
import ctypes
import os
import re

import pytest

from conftest import PKG_ROOT, REPO

HEADER = os.path.join(REPO, "include", "dgs_volume.h")
LIB = os.path.join(PKG_ROOT, "diff_gaussian_sampling", "libdgs.so")
DGS_ERR_ARG, DGS_ERR_BUFFER = 1, 4
NAMES = ["dgs_volume_workspace_size_fused", "dgs_volume_forward_fused", "dgs_volume_backward_fused",
         "dgs_volume_backward_samples_fused"]
VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdgs.so is not built (python diff-gaussian-sampling_amd/build.py)")
    lib = ctypes.CDLL(LIB)
    lib.dgs_last_error.restype = ctypes.c_char_p
    return lib


def _calls(lib):
    """the three calls with every pointer NULL except the binning: (mask, P, N, C, binning, bytes) -> rc"""
    fwd = lib.dgs_volume_forward_fused
    fwd.restype, fwd.argtypes = I, [I] * 4 + [VP] * 5 + [SZ, VP, VP, I]
    bwd = lib.dgs_volume_backward_fused
    bwd.restype, bwd.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 4 + [SZ, VP, I]
    sg = lib.dgs_volume_backward_samples_fused
    sg.restype, sg.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 2 + [SZ, VP, I]
    ptrs = (VP * 4)()
    return (lambda m, P, N, C, b=None, n=0: fwd(m, P, N, C, None, None, None, None, b, n, ptrs, None, 0),
            lambda m, P, N, C, b=None, n=0: bwd(m, P, N, C, None, None, None, None, ptrs, b, n, None, None, None,
                                                None, 0, None, 0),
            lambda m, P, N, C, b=None, n=0: sg(m, P, N, C, None, None, None, None, ptrs, b, n, None, None, 0, None, 0))


def test_names_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    assert re.search(r"#define\s+DGS_VOLUME_FUSED_MAX_C\s+4\b", text)


def test_workspace_size(lib):
    ws = lib.dgs_volume_workspace_size_fused
    multi = lib.dgs_volume_workspace_size_multi
    for f in (ws, multi):
        f.restype, f.argtypes = SZ, [I] * 5
    P = 10
    assert ws(7, P, 100, 3, 1) == 100 * 10 * 3 * 4  # 1 + 3 + 6 unique components, 3 channels
    assert ws(15, P, 100, 4, 1) == 100 * 20 * 4 * 4
    assert ws(3, P, 100, 2, 1) == 100 * 4 * 2 * 4
    for f in range(4):
        for C in (1, 3):
            assert ws(1 << f, P, 100, C, 1) == multi(1 << f, P, 100, C, 1) > 0
    for mask in range(1, 16):
        assert ws(mask, P, 100, 1, 1) == multi(mask, P, 100, 1, 1) > 0
    for mask, C in ((1, 1), (3, 1), (7, 3), (15, 4), (8, 3)):
        assert ws(mask, P, 100, C, 0) == 0  # the forward needs none
    assert ws(3, P, 100, 5, 1) == 0  # several functions above the limit: the caller's fallback


def test_argument_errors_before_device_work(lib):
    for call in _calls(lib):
        for mask in (0, 16):
            for C in (1, 3):
                assert call(mask, 10, 10, C) == DGS_ERR_ARG
                assert b"mask" in lib.dgs_last_error()
        assert call(3, 10, 10, 5) == DGS_ERR_ARG  # several functions above DGS_VOLUME_FUSED_MAX_C
        msg = lib.dgs_last_error()
        assert b"C <= 4" in msg and b"per-function" in msg, msg
        short = ctypes.create_string_buffer(16)
        for mask, C in ((3, 2), (15, 4), (3, 1), (4, 3)):  # the new path and the two it forwards
            assert call(mask, 10, 10, C) == DGS_ERR_BUFFER  # NULL binning
            assert call(mask, 10, 10, C, ctypes.cast(short, VP), 16) == DGS_ERR_BUFFER
        assert call(3, -1, 10, 2) == DGS_ERR_ARG


def test_multi_entries_keep_their_contract(lib):
    """the *_multi entries still refuse several functions at C > 1: callers pick their fallback by it"""
    fwd = lib.dgs_volume_forward_multi
    fwd.restype, fwd.argtypes = I, [I] * 4 + [VP] * 5 + [SZ, VP, VP, I]
    assert fwd(3, 10, 10, 2, None, None, None, None, None, 0, (VP * 4)(), None, 0) == DGS_ERR_ARG
    assert b"per-function" in lib.dgs_last_error()
    multi = lib.dgs_volume_workspace_size_multi
    multi.restype, multi.argtypes = SZ, [I] * 5
    assert multi(7, 10, 100, 3, 1) == 0


def test_version_is_unchanged(lib):
    lib.dgs_version.restype = I
    assert lib.dgs_version() == 12
