"""GPU parity of the fused D = 3 functions of a multi-channel field (dgs_volume_*_fused: several
functions at 2 <= C <= 4 in one walk of the candidates, forward, backward and the sample-position
gradient; DESIGN.md 4.8, "fused functions at C = 2..4").

Authority: the brute-force oracle (oracle/volume.py) and tests/volume_sample_grad_ref.py.  Bound:
SURVEY 8c, |d| <= 1e-5 |ref| + 1e-6 max|ref|, for the outputs and for the gradients of the summed
loss.  Fields and upstream gradients are those of tests/test_gpu_volume_multi.py with C passed to
oracle.volume.gaussians3: function f's upstream gradient is scaled by 0.01**f, which keeps the four
functions' gradient maxima within a factor of 4.1 of each other at C = 2, 3 and 4 on the parity
case (dmeans 2.7 / 1.8 / 3.4, dvalues 2.4 / 1.2 / 2.0, dconics 1.7 / 2.6 / 4.1; asserted <= 10
below), so the bound on the sum sees every function.  The oracle runs once per case and module."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import volume_sample_grad_ref as vr
from helpers import close, margin_of, record_margin
from oracle import volume as vo
from test_gpu_volume_multi import MULTI_MASKS, Case, _codes, _field, _with_big

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
NAMES = ("gaussian", "derivative", "laplacian", "third")
DGS_ERR_ARG = 1


def _sref(case, f):
    """the reference sample gradient of function f of a Case, computed once"""
    cache = case.__dict__.setdefault("_sg", {})
    if f not in cache:
        cache[f] = vr.dsamples(f, case.means, case.values, case.conics, case.samples, case.dL[f])
        cache[f].setflags(write=False)
    return cache[f]


_cases = {}


def _parity(C):
    """the parity case of tests/test_gpu_volume_multi.py at C channels"""
    if C not in _cases:
        means, values, _, conics = vo.gaussians3(1000, C, seed=3, scale=0.009 * 1000 ** (1 / 3))
        _cases[C] = Case(means, values, conics, vo.samples3(2000, seed=12))
    return _cases[C]


@pytest.fixture(scope="module")
def big_case():
    means, values, _, conics = _field(600, 3, 7)
    return Case(means, values, _with_big(conics), vo.samples3(1200, seed=8))


def _chunk_case(C, cluster_last=False):
    """150 Gaussians and 200 samples inside one grid cell next to a sparse remainder
    (test_gpu_volume_multi.test_fused_chunk_boundaries); cluster_last: the cluster's samples are the
    last by index"""
    rng = np.random.default_rng(21)
    means, values, _, conics = _field(250, C, 5)
    samples = vo.samples3(330, seed=13)
    centre = np.array([0.31, -0.22, 0.47])
    means[:150] = (centre + rng.uniform(-0.002, 0.002, (150, 3))).astype(np.float32)
    samples[:200] = (centre + rng.uniform(-0.002, 0.002, (200, 3))).astype(np.float32)
    if cluster_last:
        samples = np.ascontiguousarray(samples[::-1])
    return Case(means, values, conics, samples)


def _run(case, codes, debug=False, dL=None, sgrad=True):
    """fused forward, backward and sample gradient through the extension on one binning; numpy"""
    from diff_gaussian_sampling import _C
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, debug)
    outs = _C.volume_forward_multi(list(codes), m, v, c, s, buf, debug)
    dL = case.dL if dL is None else dL
    dls = [torch.from_numpy(dL[f]).to(m.device) for f in codes]
    grads = tuple(g.cpu().numpy() for g in _C.volume_backward_multi(list(codes), m, v, c, s, dls, buf, debug))
    ds = _C.volume_samples_backward(list(codes), m, v, c, s, dls, buf, debug).cpu().numpy() if sgrad else None
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], grads, ds


def _check(case, codes, what, debug=False, sgrad=True):
    outs, grads, ds = _run(case, codes, debug, sgrad=sgrad)
    for f, o in zip(codes, outs):
        assert o.shape == (case.N,) + (3,) * f + (case.C,)
        close(o.reshape(case.N, 3 ** f, case.C), case.fwd(f), RTOL, ATOL, f"{what} {tuple(codes)} fn{f} forward")
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        ref = sum(case.bwd(f)[k] for f in codes)
        assert grads[k].shape == ref.shape
        close(grads[k], ref, RTOL, ATOL, f"{what} {tuple(codes)} {name}")
    if sgrad:
        _check_sgrad(case, codes, ds, what)
    return outs, grads, ds


def _check_sgrad(case, codes, ds, what):
    ref = sum(_sref(case, f) for f in codes)
    assert ds.shape == (case.N, 3)
    if os.environ.get("DGS_MARGINS") and case.means.shape[0] and case.N:
        # what float32 itself costs: one serial float32 order of the same sum
        serial = vr.dsamples_multi(codes, case.means, case.values, case.conics, case.samples,
                                   [case.dL[f] for f in codes], dtype=np.float32)
        record_margin(f"{what} {tuple(codes)} dsamples [float32 serial order vs float64]", margin_of(serial, ref, RTOL, ATOL),
                      RTOL, ATOL, int(ref.size))
    close(ds, ref, RTOL, ATOL, f"{what} {tuple(codes)} dsamples")


# ---- 1. parity of every fused mask
@pytest.mark.parametrize("C", [2, 3, 4])
def test_upstream_scaling_balances_the_functions(C):
    """From the oracle alone: with dL_f scaled by 0.01**f no function's gradient is more than 10x
    another's, so the bound on the summed gradient sees every function."""
    case = _parity(C)
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        mx = [float(np.abs(case.bwd(f)[k]).max()) for f in range(4)]
        print(C, name, mx, max(mx) / min(mx))
        assert max(mx) <= 10.0 * min(mx), (name, mx)


@pytest.mark.parametrize("mask", MULTI_MASKS)
def test_fused_parity_c3(dgs, mask):
    _check(_parity(3), _codes(mask), "parity C3", sgrad=False)


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("mask", [7, 15])
def test_fused_parity_partial_and_full_block(dgs, mask, C):
    _check(_parity(C), _codes(mask), f"parity C{C}", sgrad=False)


# ---- 2. an output does not depend on the mask, and is the single call's
def test_fused_forward_is_mask_independent_and_bitwise_the_single_calls(dgs, big_case):
    from diff_gaussian_sampling import _C
    for case in (_parity(3), big_case):
        m, v, c, s = case.dev()
        buf = _C.volume_preprocess(m, c, s, False)
        got = {codes: _C.volume_forward_multi(list(codes), m, v, c, s, buf, False)
               for codes in ((0, 1), (1, 2), (0, 1, 2, 3))}
        full = dict(zip((0, 1, 2, 3), got[(0, 1, 2, 3)]))
        for codes in ((0, 1), (1, 2)):
            for f, o in zip(codes, got[codes]):
                assert torch.equal(o, full[f]), (codes, f, float((o - full[f]).abs().max()))
        for f in range(4):  # the roundings of k_vol_forward<FN, 4>
            single = _C.volume_forward(f, m, v, c, s, buf, False)
            assert torch.equal(full[f], single), (f, float((full[f] - single).abs().max()))


# ---- 3. the sample gradient
@pytest.mark.parametrize("mask,C", [(3, 3), (7, 3), (12, 3), (15, 3), (7, 2), (7, 4)])
def test_fused_sample_gradient(dgs, mask, C):
    from diff_gaussian_sampling import _C
    case, codes = _parity(C), _codes(mask)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
    ds = _C.volume_samples_backward(codes, m, v, c, s, dls, buf, False)
    assert ds.dtype == torch.float32
    _check_sgrad(case, codes, ds.cpu().numpy(), f"sgrad C{C}")


def test_sgrad_upstream_scaling_balances_the_functions():
    mx = [float(np.abs(_sref(_parity(3), f)).max()) for f in range(4)]
    print("per-function max |dsamples|", mx)
    assert max(mx) <= 10.0 * min(mx), mx


# ---- 4. the every-sample class
@pytest.mark.parametrize("codes", [(0, 3), (0, 1, 2, 3)])
def test_fused_big_gaussians(dgs, big_case, codes):
    """wide, ill-conditioned, indefinite (power > 0 skipped) and nearly singular conics: the fused
    big-Gaussian backward writes their rows once, as the sum over the mask"""
    _check(big_case, codes, "big C3")


# ---- 5. seams and far images
def test_fused_seams_and_images(dgs):
    """the construction of test_gpu_volume_multi.test_fused_seams_and_images at C = 2"""
    rng = np.random.default_rng(2)
    means, values, _, conics = _field(400, 2, 2)
    means[:100, 0] = np.float32(0.999)
    means[100:200, 1] = np.float32(-0.999)
    means[200:220] = rng.uniform(2.5, 3.5, (20, 3)).astype(np.float32)  # far outside: images
    samples = vo.samples3(1500, seed=3)
    samples[:300, 0] = np.float32(-0.998)
    samples[300:400] = rng.uniform(-3.2, -2.8, (100, 3)).astype(np.float32)
    _check(Case(means, values, conics, samples), (0, 1, 2), "seams C2")


# ---- 6. chunk boundaries
def test_fused_chunk_boundaries(dgs):
    """several 64-wide batches with a partial last one, in the lane = sample and the lane = Gaussian
    loop nests"""
    _check(_chunk_case(3), (0, 1, 2, 3), "chunks C3")


# ---- 7. edge sizes
def test_fused_edge_sizes(dgs):
    means, values, _, conics = _field(50, 2, 1)
    samples = vo.samples3(40, seed=1)
    for P, N in ((0, 40), (50, 0), (1, 1), (50, 1)):
        case = Case(means[:P], values[:P], conics[:P], samples[:N])
        outs, grads, ds = _check(case, (0, 1, 2, 3), f"edge P{P} N{N} C2")
        if P == 0:
            assert not ds.any() and not any(o.any() for o in outs)
        if N == 0:
            assert not any(g.any() for g in grads)


# ---- 8. the row past the end
def test_fused_padded_channels_are_never_read(dgs):
    """C = 3 with the last sample by index among the staged candidates and NaN bit patterns behind
    hs in an oversized workspace: a padded channel that was read and multiplied by 0 (instead of
    selected to 0) would put NaN into the gradients of the Gaussians that meet that sample."""
    from diff_gaussian_sampling import _C
    import dgs_ctypes
    case, codes = _chunk_case(3, cluster_last=True), (0, 1, 2, 3)
    N, C = case.N, 3
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
    need = dgs_ctypes.volume_workspace_size_fused(15, 250, N, C, 1)
    assert need == N * 20 * C * 4
    work = torch.full((need // 4 + 4096,), float("nan"), device=m.device).view(torch.uint8)
    torch.cuda.synchronize()
    grads = dgs_ctypes.volume_backward_fused(codes, m, v, c, s, dls, buf, False, workspace=work)
    torch.cuda.synchronize()
    tail = work.view(torch.float32)[need // 4:]
    assert torch.isnan(tail).all()  # nothing written behind hs either
    # the last sample's pairs are live: its Gaussians' gradients are not zero
    G = vo._pairs(case.means, case.conics, case.samples[N - 1:])[1]
    assert (np.asarray(G) > 0).sum() >= 100
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        g = grads[k].cpu().numpy()
        assert np.isfinite(g).all(), name
        close(g, sum(case.bwd(f)[k] for f in codes), RTOL, ATOL, f"padded channels C3 {name}")


# ---- 9. locality of a non-finite upstream gradient
@pytest.mark.parametrize("hot", [0, 1, 2])
def test_fused_nonfinite_dl_stays_local(dgs, hot):
    """dL = +inf at one sample for one function of mask 7 at C = 3: every other sample's dL_dsamples
    is bit for bit unchanged, and the Gaussians with a non-finite gradient row are those of the
    per-function calls added (the same pair set)."""
    from diff_gaussian_sampling import _C
    case, codes, j = _parity(3), (0, 1, 2), 1234
    inf = [x.copy() for x in case.dL]
    inf[hot][j] = np.inf
    _, g0, ds0 = _run(case, codes)
    _, g1, ds1 = _run(case, codes, dL=inf)
    keep = np.arange(case.N) != j
    assert np.isfinite(ds0).all() and ds0[j].any()
    assert not np.isfinite(ds1[j]).all()
    assert np.array_equal(ds0[keep], ds1[keep])
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    sep = None
    for f in codes:
        g = _C.volume_backward(f, m, v, c, s, buf, torch.from_numpy(inf[f]).to(m.device), False)
        sep = g if sep is None else tuple(a + b for a, b in zip(sep, g))
    bad_sep = np.zeros(case.means.shape[0], bool)
    bad = np.zeros(case.means.shape[0], bool)
    for a, b, fin in zip(g1, sep, g0):
        assert np.isfinite(fin).all()
        bad |= ~np.isfinite(a).all(axis=1)
        bad_sep |= ~np.isfinite(b.cpu().numpy()).all(axis=1)
    assert 0 < bad.sum() < bad.size
    assert np.array_equal(bad, bad_sep), (bad.sum(), bad_sep.sum())
    for a, fin in zip(g1, g0):  # the other Gaussians' rows: bit for bit the finite run's
        assert np.array_equal(a[~bad], fin[~bad])


# ---- 10. loud on stale input
def test_fused_stale_buffer_is_loud(dgs):
    from diff_gaussian_sampling import _C
    dev = torch.device("cuda:0")
    means, values, _, conics = (torch.from_numpy(x).to(dev) for x in _field(100, 3, 1))
    s = torch.from_numpy(vo.samples3(200)).to(dev)
    codes = [0, 1, 2, 3]

    def all_nan(m, buf, cs):
        outs = _C.volume_forward_multi(cs, m, values, conics, s, buf, False)
        dls = [torch.ones_like(o) for o in outs]
        res = list(outs) + list(_C.volume_backward_multi(cs, m, values, conics, s, dls, buf, False))
        res.append(_C.volume_samples_backward(cs, m, values, conics, s, dls, buf, False))
        return [bool(torch.isnan(t).all()) and t.numel() > 0 for t in res], [bool(torch.isfinite(t).all()) for t in res]

    other = _C.volume_preprocess(means, conics, s[:100].contiguous(), False)  # a binning of other sizes
    assert all(all_nan(means, other, codes)[0])
    buf = _C.volume_preprocess(means, conics, s, False)
    assert all(all_nan(means, buf, codes)[1])  # fresh: finite
    means[7, 0] += 1e-3  # changed in place after the binning
    assert all(all_nan(means, buf, codes)[0])
    assert all(all_nan(means, buf, [1, 3])[0])


# ---- 11. repeatable
def test_fused_repeatable_and_debug(dgs, big_case):
    codes = (0, 1, 2, 3)
    a, ga, sa = _run(big_case, codes)
    b, gb, sb = _run(big_case, codes)
    d, gd, sd = _run(big_case, codes, debug=True)
    for x, y, z in zip(a + list(ga) + [sa], b + list(gb) + [sb], d + list(gd) + [sd]):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- 12. the C entries through ctypes
def test_fused_ctypes_is_the_extension(dgs):
    from diff_gaussian_sampling import _C
    import dgs_ctypes
    means, values, _, conics = _field(500, 3, 9)
    case = Case(means, values, conics, vo.samples3(800, seed=15))
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    dl = lambda codes, C: [torch.from_numpy(np.ascontiguousarray(case.dL[f][:, :, :C])).to(m.device) for f in codes]
    # mask 7 at C = 3: the extension's call
    codes = [0, 1, 2]
    ext = (list(_C.volume_forward_multi(codes, m, v, c, s, buf, False))
           + list(_C.volume_backward_multi(codes, m, v, c, s, dl(codes, 3), buf, False))
           + [_C.volume_samples_backward(codes, m, v, c, s, dl(codes, 3), buf, False)])
    got = (dgs_ctypes.volume_forward_fused(codes, m, v, c, s, buf, False)
           + list(dgs_ctypes.volume_backward_fused(codes, m, v, c, s, dl(codes, 3), buf, False))
           + [dgs_ctypes.volume_samples_backward_fused(codes, m, v, c, s, dl(codes, 3), buf, False)])
    torch.cuda.synchronize()
    for a, b in zip(ext, got):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # a single bit at C = 3 and several functions at C = 1: the *_multi entries' launches
    v1 = v[:, :1].contiguous()
    for codes, vv, C in (([2], v, 3), ([0, 1, 2], v1, 1)):
        for entry_results in zip(*[
                (dgs_ctypes.volume_forward_fused(codes, m, vv, c, s, buf, False, entry=e)
                 + list(dgs_ctypes.volume_backward_fused(codes, m, vv, c, s, dl(codes, C), buf, False, entry=e))
                 + [dgs_ctypes.volume_samples_backward_fused(codes, m, vv, c, s, dl(codes, C), buf, False, entry=e)])
                for e in ("fused", "multi")]):
            a, b = entry_results
            assert torch.isfinite(a).all() and torch.equal(a, b)
    # several functions above the limit
    v5 = torch.cat([v, v[:, :2]], 1).contiguous()
    outs = (ctypes.c_void_p * 4)()
    rc = dgs_ctypes._lib.dgs_volume_forward_fused(3, 500, 800, 5, m.data_ptr(), v5.data_ptr(), c.data_ptr(),
                                                  s.data_ptr(), buf.data_ptr(), buf.numel(), outs, None, 0)
    assert rc == DGS_ERR_ARG and b"C <= 4" in dgs_ctypes._lib.dgs_last_error()
    with pytest.raises(RuntimeError, match="C <= 4"):
        dgs_ctypes.volume_backward_fused([0, 1], m, v5, c, s, dl([0, 1], 3), buf, False,
                                         workspace=torch.empty(16, dtype=torch.uint8, device=m.device))


# ---- 13. autograd through VolumeSampler
def test_fused_sampler_autograd(dgs):
    from diff_gaussian_sampling.volume import VolumeSampler
    dev = torch.device("cuda:0")
    P, N, C = 500, 600, 3
    means, values, covs, conics = _field(P, C, 8)
    samples = vo.samples3(N, seed=8)
    case = Case(means, values, conics, samples)
    w = [torch.from_numpy(x).to(dev).reshape((N,) + (3,) * f + (C,)) for f, x in enumerate(case.dL)]
    m, v, cv, c, s = (torch.from_numpy(x).to(dev) for x in (means, values, covs, conics, samples))
    for t in (m, v, c, s):
        t.requires_grad_(True)
    vs = VolumeSampler(False, sample_grad=True)
    vs.preprocess(m, v, cv, c, s)
    outs = vs.sample_gaussians_multi("gaussian", "derivative", "laplacian")
    assert [o.shape for o in outs] == [x.shape for x in w[:3]]
    sum((outs[f] * w[f]).sum() for f in (0, 2)).backward()  # the derivative's output unused
    for f in range(3):
        close(outs[f].detach().cpu().numpy().reshape(N, 3 ** f, C), case.fwd(f), RTOL, ATOL, f"autograd C3 fn{f} forward")
    for k, (name, t) in enumerate((("dmeans", m), ("dvalues", v), ("dconics", c))):
        close(t.grad.cpu().numpy(), sum(case.bwd(f)[k] for f in (0, 2)), RTOL, ATOL, f"autograd C3 {name}")
    close(s.grad.cpu().numpy(), sum(_sref(case, f) for f in (0, 2)), RTOL, ATOL, "autograd C3 dsamples")
    # the moving-collocation-point loop: an in-place step, the sampler re-bins
    binned = vs.binning
    with torch.no_grad():
        s -= (0.01 / float(s.grad.abs().max())) * s.grad
        s.grad = None
    moved = s.detach().cpu().numpy()
    assert np.abs(moved - samples).max() > 1e-3
    g, lap = vs.sample_gaussians_multi("gaussian", "laplacian")
    assert vs.binning is not binned
    ((g * w[0]).sum() + (lap * w[2]).sum()).backward()
    close(lap.detach().cpu().numpy().reshape(N, 9, C), vo.forward(2, means, values, conics, moved), RTOL, ATOL,
          "laplacian C3 after the step")
    ref = vr.dsamples_multi((0, 2), means, values, conics, moved, [case.dL[0], case.dL[2]])
    close(s.grad.cpu().numpy(), ref, RTOL, ATOL, "dsamples C3 after the step")

    # C = 5 with two functions: the per-function fallback, as before
    means, values, covs, conics = _field(200, 5, 9)
    case5 = Case(means, values, conics, vo.samples3(300, seed=9))
    m, v, cv, c, s = (torch.from_numpy(x).to(dev) for x in (means, values, covs, conics, case5.samples))
    for t in (m, v, c):
        t.requires_grad_(True)
    vs = VolumeSampler(False)
    vs.preprocess(m, v, cv, c, s)
    g, d = vs.sample_gaussians_multi("gaussian", "derivative")
    w5 = [torch.from_numpy(case5.dL[f]).to(dev).reshape(o.shape) for f, o in ((0, g), (1, d))]
    ((g * w5[0]).sum() + (d * w5[1]).sum()).backward()
    close(d.detach().cpu().numpy().reshape(300, 3, 5), case5.fwd(1), RTOL, ATOL, "fallback C5 derivative")
    for k, (name, t) in enumerate((("dmeans", m), ("dvalues", v), ("dconics", c))):
        close(t.grad.cpu().numpy(), sum(case5.bwd(f)[k] for f in (0, 1)), RTOL, ATOL, f"fallback C5 {name}")
