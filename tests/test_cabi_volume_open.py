"""C-ABI checks of dgs_volume_preprocess_axes (include/dgs_volume.h: the binning of a D = 3 field with
a choice of the wrap per axis) through tools/dgs_ctypes.py.  Without a GPU: the name is declared and
exported, a mask outside 0..7 returns DGS_ERR_ARG before any device work, the ABI version is
unchanged.  On the GPU: a binning made through the C entry drives the other entries (which take the
axes from the binning with their argument lists unchanged) to the reference of
tests/volume_open_ref.py within SURVEY 8c, periodic = 7 is dgs_volume_preprocess bit for bit, and
dgs_volume_count_pairs follows the binning's axes."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

HEADER = os.path.join(REPO, "include", "dgs_volume.h")
LIB = os.path.join(PKG_ROOT, "diff_gaussian_sampling", "libdgs.so")
DGS_ERR_ARG = 1
RTOL, ATOL = 1e-5, 1e-6
VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdgs.so is not built (python diff-gaussian-sampling_amd/build.py)")
    lib = ctypes.CDLL(LIB)
    lib.dgs_last_error.restype = ctypes.c_char_p
    return lib


def test_name_is_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bdgs_volume_preprocess_axes\s*\(\s*int\s+periodic\s*,", text)
    assert hasattr(lib, "dgs_volume_preprocess_axes")


def test_bad_mask_is_an_argument_error_before_device_work(lib):
    f = lib.dgs_volume_preprocess_axes
    f.restype, f.argtypes = I, [I] * 3 + [VP] * 3 + [ALLOC_FN, VP, VP, I]
    called = []

    def alloc(ctx, which, nbytes):
        called.append(which)
        return None

    cb = ALLOC_FN(alloc)
    fake = ctypes.cast(ctypes.create_string_buffer(64), VP)  # (never read)
    for bad in (-1, 8, 15, 1 << 20):
        assert f(bad, 1, 1, fake, fake, fake, cb, None, None, 0) == DGS_ERR_ARG, bad
        assert b"periodic" in lib.dgs_last_error()
    assert not called


def test_version_is_unchanged(lib):
    lib.dgs_version.restype = I
    assert lib.dgs_version() == 12


@pytest.mark.gpu
def test_c_entry_drives_the_other_entries(dgs):
    """periodic = 3 and 0 on the seam field: the gaussian, the derivative and the operator through
    dgs_volume_*_linop, which never hear of the axes"""
    import torch

    import dgs_ctypes
    from test_volume_open_ref import seam_case
    from helpers import close
    from volume_open_ref import OP, OpenCase
    base = seam_case()
    m, v, c, s = base.dev()
    codes = [0, 1, OP]
    for mask in (3, 0):
        case = OpenCase(base, mask)
        buf = dgs_ctypes.volume_preprocess_axes(m, c, s, mask, False)
        dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
        outs = dgs_ctypes.volume_forward_linop(codes, case.coef, m, v, c, s, buf, False)
        grads = dgs_ctypes.volume_backward_linop(codes, case.coef, m, v, c, s, dls, buf, False)
        ds = dgs_ctypes.volume_samples_backward_linop(codes, case.coef, m, v, c, s, dls, buf, False)
        torch.cuda.synchronize()
        for f, o in zip(codes, outs):
            close(o.cpu().numpy().reshape(case.N, -1, 1), case.fwd(f), RTOL, ATOL, f"C ABI periodic {mask} fn{f} forward")
        for k, name in enumerate(("dmeans", "dvalues", "dconics")):
            close(grads[k].cpu().numpy(), sum(case.bwd(f)[k] for f in codes), RTOL, ATOL, f"C ABI periodic {mask} {name}")
        close(ds.cpu().numpy(), sum(case.sref(f) for f in codes), RTOL, ATOL, f"C ABI periodic {mask} dsamples")
        sure, last = case.live_pairs()  # (tests/test_gpu_volume_open.py, test_pair_counts_with_every_axis_open)
        assert sure <= dgs_ctypes.volume_count_pairs(m, c, s, buf)[1] <= sure + last


@pytest.mark.gpu
def test_periodic_7_is_dgs_volume_preprocess(dgs):
    import torch

    import dgs_ctypes
    from test_volume_open_ref import seam_case
    base = seam_case()
    m, v, c, s = base.dev()
    codes = [0, 1, 2, 3]
    dls = [torch.from_numpy(base.dL[f]).to(m.device) for f in codes]
    res = []
    for periodic in (None, 7):  # None: dgs_volume_preprocess
        buf = dgs_ctypes.volume_preprocess_axes(m, c, s, periodic, False)
        res.append(dgs_ctypes.volume_forward_fused(codes, m, v, c, s, buf, False, entry="multi")
                   + list(dgs_ctypes.volume_backward_fused(codes, m, v, c, s, dls, buf, False, entry="multi"))
                   + [dgs_ctypes.volume_samples_backward_fused(codes, m, v, c, s, dls, buf, False, entry="multi")]
                   + [torch.tensor(dgs_ctypes.volume_count_pairs(m, c, s, buf))])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b) and torch.isfinite(a.double()).all()
    assert res[0][0].abs().max() > 0 and res[0][-1][1] > 0
    with pytest.raises(RuntimeError, match="periodic"):
        dgs_ctypes.volume_preprocess_axes(m, c, s, 8, False)
    with pytest.raises(RuntimeError, match="periodic"):
        dgs_ctypes.volume_preprocess_axes(m, c, s, -1, False)
