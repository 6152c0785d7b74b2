"""The reference of open axes (tests/volume_open_ref.py), on the CPU.

1. Under mask 7 (every axis periodic) the patched reference is bit for bit the unpatched one, and the
   patch is gone after the block, also when the block raises.
2. At mask 3 (axis 2 open) the reference gradients of means, values, conics and samples equal torch
   float64 autograd of `volume_sample_grad_ref.torch_forward` (tolerances of
   tests/test_volume_linop_ref.py), on a field whose pairs reach |m - s| > 1 on axis 2, where the
   wrapped and the open X differ; the outputs differ from the all-periodic ones.
3. The margin check, as tests/test_volume_linop_ref.py makes it: for every field and mask the GPU
   tests compare on (tests/test_gpu_volume_open.py: the parity and the big-Gaussian field at C = 3,
   masks 3 and 0; the seam field at C = 1, every mask) the reference's own float32 serial order of
   the `balanced` operator's forward and sample gradient lies within 0.9 of the SURVEY 8c bound,
   |d| <= 1e-5 |ref| + 1e-6 max|ref|, so no GPU comparison is left out.  Measured: parity forward
   0.064, sample gradient 0.079; big-Gaussian forward at most 0.172, sample gradient 0.272; seam
   forward at most 0.031, sample gradient at most 0.130.  With DGS_MARGINS set the shares are recorded.
4. The GPU tests can tell the feature from its absence: for every such field and mask but 7 at least
   one reference output differs from the all-periodic reference by more than the bound (parity 42 of
   6000 at mask 3; big-Gaussian 943 and 2661 of 3600 at masks 3 and 0; seam 20 and 240 of 1500), so
   a build that ignores the axes fails their parity.  The same on the gaussian for the other compared
   fields, parity at C = 1 and 9 and big-Gaussian at C = 1; on the chunk case the two references
   coincide (no pair crosses a seam), which is printed and not asserted.
5. What float32 costs on the big-Gaussian field per function, since the GPU tests also compare the
   four functions there: a plain float32 order (float32 a = A X and terms, added serially) of the
   forward and of dL_dvalues against the float64 reference, at masks 3 and 0.  At C = 1 every function
   stays below 0.6 of the bound and at C = 3 the gaussian, the derivative and the third derivative
   below 0.81, so those are compared.  The laplacian at C = 3 is not (its share is recorded, not
   asserted): its dL_dvalues takes 1.14 of the bound in float32 itself, with every axis periodic as well (the nearly singular conic of
   `_with_big`, whose a = A X cancels), so that comparison would test the field and not a kernel.
"""
import numpy as np
import pytest
import torch

import volume_linop_ref as lr
import volume_sample_grad_ref as vr
import volume_trace_ref as tr
from helpers import margin_of, record_margin
from oracle import volume as vo
from test_gpu_volume_multi import Case, _field, _with_big
from test_gpu_volume_multi_c import _parity
from volume_open_ref import OP, OpenCase, open_axes

RTOL, ATOL = 1e-5, 1e-6
BAL = lr.SETS["balanced"]


def seam_case():
    """the construction of test_gpu_volume_multi.test_fused_seams_and_images (C = 1): means at the
    seams of axes 0 and 1 and at 2.5..3.5, samples at -3.2..-2.8 (on an open axis simply far away)"""
    rng = np.random.default_rng(2)
    means, values, _, conics = _field(400, 1, 2)
    means[:100, 0] = np.float32(0.999)
    means[100:200, 1] = np.float32(-0.999)
    means[200:220] = rng.uniform(2.5, 3.5, (20, 3)).astype(np.float32)
    samples = vo.samples3(1500, seed=3)
    samples[:300, 0] = np.float32(-0.998)
    samples[300:400] = rng.uniform(-3.2, -2.8, (100, 3)).astype(np.float32)
    return Case(means, values, conics, samples)


def edge_field():
    """the 50 / 65 field of the edge-size tests with mean 0 and sample 0 placed across the seam of axis
    2, 0.06 apart through it, so that the (1, 1) and the (50, 65) case feel the axes"""
    means, values, _, conics = _field(50, 1, 1)
    samples = vo.samples3(65, seed=1)
    means[0] = np.array([0.3, -0.2, 0.97], np.float32)
    samples[0] = np.array([0.3, -0.2, -0.97], np.float32)
    return means, values, conics, samples


def big_case(C):
    means, values, _, conics = _field(600, C, 7)
    return Case(means, values, _with_big(conics), vo.samples3(1200, seed=8))


_fields = {}


def field(name):
    """the three fields of the GPU comparisons, built once"""
    if name not in _fields:
        _fields[name] = {"parity": lambda: _parity(3), "big": lambda: big_case(3), "seam": seam_case}[name]()
    return _fields[name]


# every (field, mask) the GPU tests compare on
COMPARED = [("parity", 3), ("parity", 0), ("big", 3), ("big", 0)] + [("seam", m) for m in range(8)]
_open = {}


def opened(name, mask):
    if (name, mask) not in _open:
        _open[(name, mask)] = OpenCase(field(name), mask)
    return _open[(name, mask)]


def _small(C=2, seed=5):
    means, values, _, conics = vo.gaussians3(40, C, seed=seed, scale=3.0)
    return means, values, conics, vo.samples3(60, seed=21)


def test_mask_7_is_the_unpatched_reference():
    m, v, c, s = _small()
    dL = [np.random.default_rng(f).normal(size=(60, 3 ** f, 2)) for f in range(4)]
    dL1 = np.random.default_rng(9).normal(size=(60, 2))

    def everything():
        res = []
        for f in range(4):
            res += [vo.forward(f, m, v, c, s), *vo.backward(f, m, v, c, s, dL[f]), vr.dsamples(f, m, v, c, s, dL[f])]
        res += [tr.forward(m, v, c, s), *tr.backward(m, v, c, s, dL1), tr.dsamples(m, v, c, s, dL1)]
        res += [lr.forward(BAL, m, v, c, s), lr.forward(BAL, m, v, c, s, np.float32), *lr.backward(BAL, m, v, c, s, dL1),
                lr.dsamples(BAL, m, v, c, s, dL1)]
        return res

    orig = vo._wrap
    plain = everything()
    with open_axes(7):
        assert vo._wrap is not orig
        patched = everything()
    assert vo._wrap is orig
    for a, b in zip(plain, patched):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    with pytest.raises(RuntimeError):
        with open_axes((True, False, True)):
            raise RuntimeError("inside")
    assert vo._wrap is orig


@pytest.mark.parametrize("function", [0, 1, 2, 3])
def test_reference_gradients_match_autograd_at_mask_3(function):
    P, N, C = 40, 60, 2
    means, values, conics, samples = _small(C)
    samples[0] = means[0]  # an exact hit
    means[:10, 2] = np.float32(0.9) + np.float32(0.2) * np.arange(10, dtype=np.float32)  # 0.9 .. 2.7
    samples[1:20, 2] = np.float32(-0.95)
    far = np.abs(means[:, None, 2] - samples[None, :, 2]) > 1.0
    assert far.sum() > 100  # pairs with |m - s| > 1 on the open axis
    dL = np.random.default_rng(3).normal(size=(N, 3 ** function, C))
    with open_axes(3):
        m, v, c, s = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (means, values, conics, samples))
        out = vr.torch_forward(function, m, v, c, s)
        ref = vo.forward(function, means, values, conics, samples)
        (out * torch.tensor(dL)).sum().backward()
        dm, dv, dc = vo.backward(function, means, values, conics, samples, dL)
        ds = vr.dsamples(function, means, values, conics, samples, dL)
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    for name, got, want in (("means", dm, m.grad), ("values", dv, v.grad), ("conics", dc, c.grad), ("samples", ds, s.grad)):
        want = want.numpy()
        assert np.abs(want).max() > 0, name
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max(), err_msg=name)
    periodic = vo.forward(function, means, values, conics, samples)
    assert (np.abs(ref - periodic) > RTOL * np.abs(periodic) + ATOL * np.abs(periodic).max()).any()


@pytest.mark.parametrize("name,mask", COMPARED)
def test_float32_order_leaves_room_under_the_bound(name, mask):
    case = opened(name, mask)
    args = (case.coef, case.means, case.values, case.conics, case.samples)
    with open_axes(mask):
        serial = lr.forward(*args, np.float32)
        sserial = lr.dsamples(*args, case.dL[OP], np.float32)
    for what, got, ref in (("forward", serial, case.fwd(OP)[:, 0, :]), ("dsamples", sserial, case.sref(OP))):
        share = margin_of(got, ref, RTOL, ATOL)
        record_margin(f"open axes {name} C{case.C} periodic mask {mask} balanced {what} [float32 serial order vs float64]",
                      share, RTOL, ATOL, int(ref.size))
        print(name, mask, what, share)
        assert share <= 0.9, (name, mask, what, share)


@pytest.mark.parametrize("name,mask", [nm for nm in COMPARED if nm[1] != 7])
def test_open_reference_differs_from_the_periodic_one(name, mask):
    ref, base = opened(name, mask).fwd(OP), opened(name, 7).fwd(OP)
    bound = RTOL * np.abs(base) + ATOL * np.abs(base).max()
    n = int((np.abs(ref - base) > bound).sum())
    print(name, mask, n, "of", ref.size, float(np.abs(ref - base).max() / np.abs(base).max()))
    assert n >= 1, (name, mask)


def _float32_shares(base, mask, f):
    """(forward, dL_dvalues): one float32 order of the sums, as a share of the 8c bound"""
    f32 = np.float32
    case = OpenCase(base, mask)
    with open_axes(mask):
        X, G, _ = vo._pairs(base.means, base.conics, base.samples)
    X, G = X.astype(f32), G.astype(f32)
    A = vo._amat(base.conics.astype(np.float64)).astype(f32)
    t = vo._terms(f, np.einsum("pij,pnj->pni", A, X).astype(f32), A).astype(f32)  # [P, N, KU]
    um, v = vo.umap(f), base.values.astype(f32)
    out = np.zeros((base.N, len(um), base.C))
    dv = np.zeros((base.means.shape[0], base.C))
    hs = np.zeros((base.N, t.shape[-1], base.C), f32)
    for k, u in enumerate(um):
        hs[:, u, :] += base.dL[f].reshape(base.N, len(um), base.C)[:, k, :]
    for ch in range(base.C):
        out[:, :, ch] = np.cumsum((v[:, ch][:, None, None] * (G[..., None] * t)).astype(f32), axis=0, dtype=f32)[-1][:, um]
        p = np.zeros(G.shape, f32)
        for u in range(t.shape[-1]):
            p = (p + hs[None, :, u, ch] * t[..., u]).astype(f32)
        dv[:, ch] = np.cumsum((G * p).astype(f32), axis=1, dtype=f32)[:, -1]
    return margin_of(out, case.fwd(f), RTOL, ATOL), margin_of(dv, case.bwd(f)[1], RTOL, ATOL)


@pytest.mark.parametrize("mask", [3, 0])
@pytest.mark.parametrize("C", [1, 3])
def test_float32_order_on_the_big_field_per_function(C, mask):
    base = big_case(C)
    for f in range(4):
        fwd, dv = _float32_shares(base, mask, f)
        record_margin(f"open axes big C{C} periodic mask {mask} fn{f} forward [float32 serial order vs float64]", fwd,
                      RTOL, ATOL, base.N * 3 ** f * C)
        record_margin(f"open axes big C{C} periodic mask {mask} fn{f} dvalues [float32 serial order vs float64]", dv,
                      RTOL, ATOL, base.means.shape[0] * C)
        print(C, mask, f, fwd, dv)
        if (f, C) != (2, 3):  # (the laplacian at C = 3, which the GPU tests leave out, is recorded only)
            assert fwd <= 0.9 and dv <= 0.9, (C, mask, f, fwd, dv)


# the other fields the GPU tests compare on at masks 3 and 0: (field, C)
OTHER = [("parity", 1), ("parity", 9), ("big", 1), ("chunk", 1), ("chunk", 3)]


@pytest.mark.parametrize("mask", [3, 0])
@pytest.mark.parametrize("name,C", OTHER)
def test_open_reference_differs_on_the_other_compared_fields(name, C, mask):
    """check 4 for the parity field at C = 1 and 9 and the big-Gaussian field at C = 1, on the gaussian
    (one oracle forward each).  The chunk case is printed and not asserted: no pair of that field
    crosses a seam (0 outputs differ at either mask), so its GPU comparison checks the 64-wide batches
    under an open binning and cannot tell the axes; the fields above and the seam field do that.  The
    edge-size fields have a pair placed across a seam (edge_field, checked below)."""
    from test_gpu_volume_multi_c import _chunk_case
    base = {"parity": lambda: _parity(C), "big": lambda: big_case(C), "chunk": lambda: _chunk_case(C)}[name]()
    ref, per = OpenCase(base, mask).fwd(0), OpenCase(base, 7).fwd(0)
    n = int((np.abs(ref - per) > RTOL * np.abs(per) + ATOL * np.abs(per).max()).sum())
    print(name, C, mask, n, "of", ref.size)
    assert n >= 1 or name == "chunk", (name, C, mask)


@pytest.mark.parametrize("mask", [3, 0])
@pytest.mark.parametrize("P,N", [(1, 1), (50, 65)])
def test_open_reference_differs_on_the_edge_fields(P, N, mask):
    means, values, conics, samples = edge_field()
    base = Case(means[:P], values[:P], conics[:P], samples[:N])
    ref, per = OpenCase(base, mask).fwd(0), OpenCase(base, 7).fwd(0)
    assert np.abs(per[0]).max() > 1e-6 * np.abs(values[0]).max()  # the pair across the seam is live when periodic
    assert (np.abs(ref - per) > RTOL * np.abs(per) + ATOL * np.abs(per).max()).any()
