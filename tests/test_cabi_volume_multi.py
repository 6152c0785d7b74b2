"""C-ABI checks of the fused D = 3 entry points (include/dgs_volume.h, dgs_volume_*_multi) that
need no GPU: the names are declared and exported, the workspace sizing, and the argument errors
that return before any device work."""
import ctypes
import os
import re

import pytest

from conftest import PKG_ROOT, REPO

HEADER = os.path.join(REPO, "include", "dgs_volume.h")
LIB = os.path.join(PKG_ROOT, "diff_gaussian_sampling", "libdgs.so")
DGS_ERR_ARG, DGS_ERR_BUFFER = 1, 4
NAMES = ["dgs_volume_workspace_size_multi", "dgs_volume_forward_multi", "dgs_volume_backward_multi"]
VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdgs.so is not built (python diff-gaussian-sampling_amd/build.py)")
    lib = ctypes.CDLL(LIB)
    lib.dgs_last_error.restype = ctypes.c_char_p
    return lib


def _bind(lib):
    ws = lib.dgs_volume_workspace_size_multi
    ws.restype, ws.argtypes = SZ, [I] * 5
    fwd = lib.dgs_volume_forward_multi
    fwd.restype, fwd.argtypes = I, [I] * 4 + [VP] * 5 + [SZ, VP, VP, I]
    bwd = lib.dgs_volume_backward_multi
    bwd.restype, bwd.argtypes = I, [I] * 4 + [VP] * 6 + [SZ] + [VP] * 4 + [SZ, VP, I]
    return ws, fwd, bwd


def _fwd(fwd, mask, P, N, C, binning=None, nbytes=0):
    outs = (VP * 4)()
    return fwd(mask, P, N, C, None, None, None, None, binning, nbytes, outs, None, 0)


def _bwd(bwd, mask, P, N, C, binning=None, nbytes=0):
    dls = (VP * 4)()
    return bwd(mask, P, N, C, None, None, None, None, dls, binning, nbytes, None, None, None, None, 0, None, 0)


def test_names_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n


def test_workspace_size(lib):
    ws, _, _ = _bind(lib)
    single = lib.dgs_volume_workspace_size
    single.restype, single.argtypes = SZ, [I] * 5
    assert ws(15, 10, 100, 1, 1) == 100 * 20 * 4  # 1 + 3 + 6 + 10 unique components
    assert ws(5, 10, 100, 1, 1) == 100 * 7 * 4
    for f in range(4):
        for C in (1, 3):
            assert ws(1 << f, 10, 100, C, 1) == single(f, 10, 100, C, 1) > 0
    for mask in (1, 3, 8, 15):
        assert ws(mask, 10, 100, 1, 0) == 0  # the forward needs none


def test_argument_errors_before_device_work(lib):
    _, fwd, bwd = _bind(lib)
    for call in (lambda *a, **k: _fwd(fwd, *a, **k), lambda *a, **k: _bwd(bwd, *a, **k)):
        for mask in (0, 16):
            assert call(mask, 10, 10, 1) == DGS_ERR_ARG
            assert b"mask" in lib.dgs_last_error()
        assert call(3, 10, 10, 2) == DGS_ERR_ARG  # several functions need C = 1
        assert b"per-function" in lib.dgs_last_error()
        assert call(3, 10, 10, 1) == DGS_ERR_BUFFER  # NULL binning
        assert call(4, 10, 10, 2) == DGS_ERR_BUFFER  # a single bit takes any C: next check is the binning
        short = ctypes.create_string_buffer(16)
        assert call(15, 10, 10, 1, ctypes.cast(short, VP), 16) == DGS_ERR_BUFFER


def test_version_is_unchanged(lib):
    lib.dgs_version.restype = I
    assert lib.dgs_version() == 12
