"""C-ABI checks of the D = 3 sample-gradient entry points (include/dgs_volume.h,
dgs_volume_sample_grad_workspace_size / dgs_volume_backward_samples) that need no GPU: the names are
declared and exported, the workspace sizing, and the argument errors that return before any device
work."""
import ctypes
import os
import re

import pytest

from conftest import PKG_ROOT, REPO

HEADER = os.path.join(REPO, "include", "dgs_volume.h")
LIB = os.path.join(PKG_ROOT, "diff_gaussian_sampling", "libdgs.so")
DGS_OK, DGS_ERR_ARG, DGS_ERR_BUFFER = 0, 1, 4
NAMES = ["dgs_volume_sample_grad_workspace_size", "dgs_volume_backward_samples"]
VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdgs.so is not built (python diff-gaussian-sampling_amd/build.py)")
    lib = ctypes.CDLL(LIB)
    lib.dgs_last_error.restype = ctypes.c_char_p
    return lib


def _bind(lib):
    ws = lib.dgs_volume_sample_grad_workspace_size
    ws.restype, ws.argtypes = SZ, [I] * 4
    sg = lib.dgs_volume_backward_samples
    sg.restype, sg.argtypes = I, [I] * 4 + [VP] * 6 + [SZ, VP, VP, SZ, VP, I]
    return ws, sg


def _call(sg, mask, P, N, C, binning=None, nbytes=0, dls=True, wbytes=0):
    """every device pointer NULL: a call that got past the checks would fault, not return"""
    d = (VP * 4)() if dls else None
    return sg(mask, P, N, C, None, None, None, None, d, binning, nbytes, None, None, wbytes, None, 0)


def test_names_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n


def test_workspace_size(lib):
    """The lanes keep their dL rows in registers: no workspace for any mask or size, so there is no
    short workspace to refuse; a caller that sizes and passes one all the same is accepted (the
    checks below run with workspace_bytes 0 and 64)."""
    ws, _ = _bind(lib)
    for mask in range(0, 17):
        for C in (1, 3, 9):
            assert ws(mask, 10, 100, C) == 0


def test_argument_errors_before_device_work(lib):
    ws, sg = _bind(lib)
    for wbytes in (ws(15, 10, 10, 1), 64):
        for mask in (0, 16):
            assert _call(sg, mask, 10, 10, 1, wbytes=wbytes) == DGS_ERR_ARG
            assert b"mask" in lib.dgs_last_error()
        assert _call(sg, 3, 10, 10, 2, wbytes=wbytes) == DGS_ERR_ARG  # several functions need C = 1
        assert b"per-function" in lib.dgs_last_error()
        assert _call(sg, 1, 10, 10, 0, wbytes=wbytes) == DGS_ERR_ARG  # C = 0
        assert b"sizes" in lib.dgs_last_error()
        assert _call(sg, 1, -1, 10, 1, wbytes=wbytes) == DGS_ERR_ARG
        assert _call(sg, 3, 10, 10, 1, wbytes=wbytes) == DGS_ERR_BUFFER  # NULL binning
        assert b"binning" in lib.dgs_last_error()
        assert _call(sg, 4, 10, 10, 2, wbytes=wbytes) == DGS_ERR_BUFFER  # a single bit takes any C
        short = ctypes.create_string_buffer(16)
        assert _call(sg, 15, 10, 10, 1, ctypes.cast(short, VP), 16, wbytes=wbytes) == DGS_ERR_BUFFER
    full = ctypes.create_string_buffer(4096)  # long enough for the header check: the next checks
    assert _call(sg, 1, 10, 10, 1, ctypes.cast(full, VP), 4096, dls=False) == DGS_ERR_ARG
    assert b"dL_douts" in lib.dgs_last_error()
    assert _call(sg, 2, 10, 10, 1, ctypes.cast(full, VP), 4096) == DGS_ERR_ARG  # no output to write
    assert b"dL_dsamples" in lib.dgs_last_error()
    assert _call(sg, 2, 10, 0, 1, ctypes.cast(full, VP), 4096) == DGS_OK  # N = 0: nothing to do


def test_version_is_unchanged(lib):
    lib.dgs_version.restype = I
    assert lib.dgs_version() == 12
