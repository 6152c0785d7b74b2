"""C-ABI checks of the dgs_volume_*_ops entry points (include/dgs_volume.h: the *_fused entries plus
function 4, the trace of the laplacian, bit 4 of the mask) that need no GPU: the names are declared
and exported, the workspace sizing, and the argument errors that return before any device work."""
import ctypes
import os
import re

import pytest

from conftest import PKG_ROOT, REPO

HEADER = os.path.join(REPO, "include", "dgs_volume.h")
LIB = os.path.join(PKG_ROOT, "diff_gaussian_sampling", "libdgs.so")
DGS_ERR_ARG, DGS_ERR_BUFFER = 1, 4
NAMES = ["dgs_volume_workspace_size_ops", "dgs_volume_forward_ops", "dgs_volume_backward_ops",
         "dgs_volume_backward_samples_ops"]
VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdgs.so is not built (python diff-gaussian-sampling_amd/build.py)")
    lib = ctypes.CDLL(LIB)
    lib.dgs_last_error.restype = ctypes.c_char_p
    return lib


def _calls(lib, suffix, nptr=5):
    """the three calls with every pointer NULL except the binning and the pointer array:
    (mask, P, N, C, binning, bytes, ptrs) -> rc"""
    fwd = getattr(lib, "dgs_volume_forward" + suffix)
    fwd.restype, fwd.argtypes = I, [I] * 4 + [VP] * 5 + [SZ, VP, VP, I]
    bwd = getattr(lib, "dgs_volume_backward" + suffix)
    bwd.restype, bwd.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 4 + [SZ, VP, I]
    sg = getattr(lib, "dgs_volume_backward_samples" + ("" if suffix == "_multi" else suffix))
    sg.restype, sg.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 2 + [SZ, VP, I]
    ptrs = (VP * nptr)()
    return (lambda m, P, N, C, b=None, n=0, p=ptrs: fwd(m, P, N, C, None, None, None, None, b, n, p, None, 0),
            lambda m, P, N, C, b=None, n=0, p=ptrs: bwd(m, P, N, C, None, None, None, None, p, b, n, None, None, None,
                                                        None, 0, None, 0),
            lambda m, P, N, C, b=None, n=0, p=ptrs: sg(m, P, N, C, None, None, None, None, p, b, n, None, None, 0,
                                                       None, 0))


def test_names_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    assert re.search(r"#define\s+DGS_VOLUME_FN_LAPLACIAN_TRACE\s+4\b", text)


def test_workspace_size(lib):
    ws, fused = lib.dgs_volume_workspace_size_ops, lib.dgs_volume_workspace_size_fused
    for f in (ws, fused):
        f.restype, f.argtypes = SZ, [I] * 5
    P = 10
    assert ws(16, P, 100, 3, 1) == 100 * 3 * 4  # one unique component
    assert ws(16, P, 100, 9, 1) == 100 * 9 * 4  # the trace alone: any C
    assert ws(19, P, 100, 1, 1) == 100 * 5 * 4  # 1 + 3 + 1
    assert ws(27, P, 100, 4, 1) == 100 * 15 * 4 * 4  # 1 + 3 + 10 + 1, 4 channels
    for mask in range(1, 16):
        for C in (1, 3, 5):
            assert ws(mask, P, 100, C, 1) == fused(mask, P, 100, C, 1)
        assert ws(mask, P, 100, 1, 1) > 0
    for mask, C in ((16, 1), (16, 3), (16, 9), (19, 1), (27, 4), (7, 3)):
        assert ws(mask, P, 100, C, 0) == 0  # the forward needs none
    assert ws(19, P, 100, 5, 1) == 0  # several functions above the limit: the caller's fallback
    for mask in (0, 32, 20, 31):
        assert ws(mask, P, 100, 1, 1) == 0


def test_argument_errors_before_device_work(lib):
    fake = ctypes.create_string_buffer(512)  # (never read: the calls return before any device work)
    for call in _calls(lib, "_ops"):
        for mask in (0, 32, 20, 31):
            for C in (1, 3):
                assert call(mask, 10, 10, C) == DGS_ERR_ARG
                assert b"mask" in lib.dgs_last_error()
        assert call(19, 10, 10, 5) == DGS_ERR_ARG  # the trace with others above DGS_VOLUME_FUSED_MAX_C
        assert b"C <= 4" in lib.dgs_last_error()
        assert call(16, 10, 10, 9) == DGS_ERR_BUFFER  # NULL binning; the trace alone takes any C
        short = ctypes.create_string_buffer(16)
        for mask, C in ((16, 1), (16, 3), (19, 1), (27, 4), (7, 3), (3, 1)):
            assert call(mask, 10, 10, C) == DGS_ERR_BUFFER
            assert call(mask, 10, 10, C, ctypes.cast(short, VP), 16) == DGS_ERR_BUFFER
        assert call(19, -1, 10, 2) == DGS_ERR_ARG
        for mask, C in ((16, 3), (19, 1), (25, 4), (7, 3)):  # NULL outs / dL_douts
            assert call(mask, 10, 10, C, ctypes.cast(fake, VP), 512, None) == DGS_ERR_ARG


def test_version_is_unchanged(lib):
    lib.dgs_version.restype = I
    assert lib.dgs_version() == 12


@pytest.mark.parametrize("suffix", ["_multi", "_fused"])
def test_older_entries_still_refuse_the_trace(lib, suffix):
    """the *_multi, *_samples and *_fused entries keep their masks 1..15"""
    for call in _calls(lib, suffix, nptr=4):
        for C in (1, 3):
            assert call(16, 10, 10, C) == DGS_ERR_ARG
            assert b"mask" in lib.dgs_last_error()
            assert call(19, 10, 10, C) == DGS_ERR_ARG
            assert b"mask" in lib.dgs_last_error()
