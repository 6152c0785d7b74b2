"""GPU parity of the D = 3 sample-position gradient (dgs_volume_backward_samples,
_C.volume_samples_backward, VolumeSampler(sample_grad=True)) against the float64
brute-force reference tests/volume_sample_grad_ref.py (every pair of every Gaussian; pinned against
autograd by tests/test_volume_sample_grad_ref.py).

Bound: SURVEY 8c as tests/test_gpu_volume.py, |d| <= 1e-5 |ref| + 1e-6 max|ref|.  Fields are
oracle.volume.gaussians3 / samples3 at test_gpu_volume.py's scale 0.009 P^(1/3).  Where several
functions share a loss, function f's upstream gradient is scaled by 0.01**f as in
tests/test_gpu_volume_multi.py, so that the bound on the sum sees every function."""
import ctypes
import os

import numpy as np
import pytest
import torch

import volume_sample_grad_ref as vr
from helpers import close, margin_of, record_margin
from oracle import volume as vo

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
NAMES = ("gaussian", "derivative", "laplacian", "third")


def _field(P, C, seed):
    return vo.gaussians3(P, C, seed=seed, scale=0.009 * max(P, 1) ** (1.0 / 3.0))


def _codes(mask):
    return [f for f in range(4) if (mask >> f) & 1]


def _dL(N, f, C, seed=5, scale=1.0):
    return (np.random.default_rng(seed).normal(size=(N, 3 ** f, C)) * scale).astype(np.float32)


def _dev(*xs):
    d = torch.device("cuda:0")
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(d) for x in xs)


def _sg(codes, means, values, conics, samples, dLs, debug=False, buf=None):
    """_C.volume_samples_backward on a fresh binning (or `buf`); numpy [N, 3]"""
    from diff_gaussian_sampling import _C
    m, v, c, s = _dev(means, values, conics, samples)
    if buf is None:
        buf = _C.volume_preprocess(m, c, s, debug)
    ds = _C.volume_samples_backward(list(codes), m, v, c, s, list(_dev(*dLs)), buf, debug)
    torch.cuda.synchronize()
    assert ds.shape == (samples.shape[0], 3) and ds.dtype == torch.float32
    return ds.cpu().numpy()


def _check(codes, means, values, conics, samples, dLs, what, debug=False):
    got = _sg(codes, means, values, conics, samples, dLs, debug)
    ref = vr.dsamples_multi(codes, means, values, conics, samples, dLs)
    assert np.abs(ref).max() > 0, what
    if os.environ.get("DGS_MARGINS"):  # what float32 itself costs: one serial float32 order of the same sum
        serial = vr.dsamples_multi(codes, means, values, conics, samples, dLs, dtype=np.float32)
        record_margin(what + " [float32 serial order vs float64]", margin_of(serial, ref, RTOL, ATOL), RTOL, ATOL,
                      int(ref.size))
    close(got, ref, RTOL, ATOL, what)
    return got, ref


# ---- 1. parity
@pytest.mark.parametrize("function", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [1, 3])
def test_sgrad_parity(dgs, function, C):
    means, values, _, conics = _field(1000, C, function)
    samples = vo.samples3(2000, seed=11 + C)
    _check([function], means, values, conics, samples, [_dL(2000, function, C)], f"parity fn{function} C{C} dsamples")


# ---- 2. channel blocks: at C = 9 the first launch stores and the later ones add (the laplacian
# takes 8 + 1 channels, the third 4 + 4 + 1)
@pytest.mark.parametrize("function", [2, 3])
def test_sgrad_channel_blocks(dgs, function):
    means, values, _, conics = _field(800, 9, 3)
    samples = vo.samples3(1500, seed=9)
    _check([function], means, values, conics, samples, [_dL(1500, function, 9)], f"blocks fn{function} C9 dsamples")


# ---- 3. every mask at C = 1
_mask_case = {}


def _masks_case():
    if not _mask_case:
        means, values, _, conics = _field(600, 1, 3)
        samples = vo.samples3(1200, seed=12)
        dLs = [_dL(1200, f, 1, seed=7 + f, scale=0.01 ** f) for f in range(4)]
        refs = [vr.dsamples(f, means, values, conics, samples, dLs[f]) for f in range(4)]
        for r in refs:
            r.setflags(write=False)
        _mask_case.update(inputs=(means, values, conics, samples), dLs=dLs, refs=refs)
    return _mask_case


def test_sgrad_upstream_scaling_balances_the_functions():
    """From the reference alone: no function's gradient is more than 10x another's."""
    mx = [float(np.abs(r).max()) for r in _masks_case()["refs"]]
    print("per-function max |dsamples|", mx)
    assert max(mx) <= 10.0 * min(mx), mx


@pytest.mark.parametrize("mask", range(1, 16))
def test_sgrad_every_mask(dgs, mask):
    case = _masks_case()
    codes = _codes(mask)
    got = _sg(codes, *case["inputs"], [case["dLs"][f] for f in codes])
    ref = sum(case["refs"][f] for f in codes)
    close(got, ref, RTOL, ATOL, f"mask {mask} dsamples")
    if len(codes) == 1:  # one code or a one-element list: the same entry, the same bits
        from diff_gaussian_sampling.volume import preprocess_volume, sample_volume, sample_volume_multi
        m, v, c, s = _dev(*case["inputs"])
        dL = _dev(case["dLs"][codes[0]])[0]
        buf = preprocess_volume(m, c, s)
        s1, s2 = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
        out = sample_volume(codes[0], m, v, c, s1, buf, sample_grad=True)
        (out * dL.reshape(out.shape)).sum().backward()
        (out2,) = sample_volume_multi(codes, m, v, c, s2, buf, sample_grad=True)
        (out2 * dL.reshape(out2.shape)).sum().backward()
        assert torch.equal(s1.grad, s2.grad)
        assert np.array_equal(s1.grad.cpu().numpy(), got)


# ---- 4. big Gaussians
@pytest.mark.parametrize("function", [0, 3])
def test_sgrad_big_gaussians(dgs, function):
    means, values, _, conics = _field(600, 2, 7)
    conics[0] = [4.0, 0.0, 0.0, 4.0, 0.0, 4.0]  # sigma 0.5: wide
    conics[1] = [1e4, 0.0, 0.0, 1e-1, 0.0, 1e4]  # cond 1e5
    conics[2] = [30.0, 0.0, 0.0, -5.0, 0.0, 30.0]  # indefinite
    conics[3] = [2000.0, 1999.0, 0.0, 2000.0, 0.0, 50.0]  # nearly singular
    samples = vo.samples3(1200, seed=8)
    _check([function], means, values, conics, samples, [_dL(1200, function, 2)], f"big fn{function} C2 dsamples")


# ---- 5. seams and images
@pytest.mark.parametrize("function", [0, 1])
def test_sgrad_seams_and_images(dgs, function):
    rng = np.random.default_rng(2)
    means, values, _, conics = _field(400, 1, 2)
    means[:100, 0] = np.float32(0.999)
    means[100:200, 1] = np.float32(-0.999)
    means[200:220] = rng.uniform(2.5, 3.5, (20, 3)).astype(np.float32)  # far outside: images
    samples = vo.samples3(1500, seed=3)
    samples[:300, 0] = np.float32(-0.998)
    samples[300:400] = rng.uniform(-3.2, -2.8, (100, 3)).astype(np.float32)
    _check([function], means, values, conics, samples, [_dL(1500, function, 1, seed=function)],
           f"seams fn{function} dsamples")


# ---- 6. chunk boundaries
@pytest.mark.parametrize("C", [1, 3, 9])
def test_sgrad_chunk_boundaries(dgs, C):
    """150 Gaussians and 200 samples in one cell: three 64-wide lane batches with a partial last
    one, and a candidate row of several staged batches."""
    rng = np.random.default_rng(21)
    means, values, _, conics = _field(250, C, 5)
    samples = vo.samples3(330, seed=13)
    centre = np.array([0.31, -0.22, 0.47])
    means[:150] = (centre + rng.uniform(-0.002, 0.002, (150, 3))).astype(np.float32)
    samples[:200] = (centre + rng.uniform(-0.002, 0.002, (200, 3))).astype(np.float32)
    for f in range(4):
        _check([f], means, values, conics, samples, [_dL(330, f, C, seed=f)], f"chunks fn{f} C{C} dsamples")


# ---- 7. edge sizes
def test_sgrad_edge_sizes(dgs):
    means, values, _, conics = _field(50, 2, 1)
    samples = vo.samples3(40, seed=1)
    got = _sg([2], means, values, conics, samples[:0], [_dL(0, 2, 2)])
    assert got.shape == (0, 3)
    got = _sg([2], means[:0], values[:0], conics[:0], samples, [_dL(40, 2, 2)])
    assert got.shape == (40, 3) and not got.any()
    _check([2], means[:1], values[:1], conics[:1], means[:1] + np.float32(0.004), [_dL(1, 2, 2)], "P = N = 1 dsamples")
    # a sample with no Gaussian within its cut: exactly 0
    means = np.array([[0.5, 0.5, 0.5], [0.52, 0.5, 0.48], [0.5, 0.47, 0.5]], np.float32)
    conics = np.tile(np.array([1e4, 0, 0, 1e4, 0, 1e4], np.float32), (3, 1))
    values = np.ones((3, 1), np.float32)
    samples = np.array([[0.505, 0.5, 0.5], [-0.5, -0.5, -0.5]], np.float32)
    for codes in ([1], [0, 1, 2, 3]):
        dLs = [_dL(2, f, 1) for f in codes]
        got, ref = _check(codes, means, values, conics, samples, dLs, f"lonely sample {codes} dsamples")
        assert not ref[1].any() and not got[1].any() and got[0].all()


# ---- 8. stale guard
def test_sgrad_stale_guard(dgs):
    from diff_gaussian_sampling import _C
    means, values, _, conics = _field(400, 1, 2)
    samples = vo.samples3(500, seed=2)
    m, v, c, s = _dev(means, values, conics, samples)
    v3 = torch.cat([v, v, v], 1).contiguous()
    dL1, dL3 = _dev(_dL(500, 1, 1), _dL(500, 1, 3))
    other = _C.volume_preprocess(m, c, s[:400].contiguous(), False)  # a binning of other sizes
    buf = _C.volume_preprocess(m, c, s, False)
    m2, s2 = m.clone(), s.clone()
    m2[7, 0] += 1e-3
    s2[7, 0] += 1e-3
    for vv, dL in ((v, dL1), (v3, dL3)):
        ok = _C.volume_samples_backward([1], m, vv, c, s, [dL], buf, False)
        assert torch.isfinite(ok).all()
        for mm, ss, bb in ((m, s, other), (m2, s, buf), (m, s2, buf)):
            ds = _C.volume_samples_backward([1], mm, vv, c, ss, [dL], bb, False)
            assert ds.shape == (500, 3) and torch.isnan(ds).all()
        again = _C.volume_samples_backward([1], m, vv, c, s, [dL], buf, False)  # the binned tensors: fine again
        assert torch.equal(again, ok)


# ---- 9. repeatability and debug
@pytest.mark.parametrize("codes,C", [([3], 1), ([0, 1, 2, 3], 1), ([3], 9)])
def test_sgrad_repeatable_and_debug(dgs, codes, C):
    means, values, _, conics = _field(700, C, 6)
    samples = vo.samples3(900, seed=6)
    dLs = [_dL(900, f, C, seed=f) for f in codes]
    a = _sg(codes, means, values, conics, samples, dLs)
    b = _sg(codes, means, values, conics, samples, dLs)
    d = _sg(codes, means, values, conics, samples, dLs, debug=True)
    assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(a, d)


# ---- 10. locality
@pytest.mark.parametrize("codes,C", [([0, 1, 2, 3], 1), ([2], 1), ([3], 3), ([3], 9)])
def test_sgrad_locality(dgs, codes, C):
    """dL = +inf at one sample: every other sample's gradient is bit for bit the finite run's (a
    lane's dL stays in its registers: nothing leaks through the staging or the channel-block add)."""
    means, values, _, conics = _field(500, C, 4)
    samples = vo.samples3(700, seed=4)
    dLs = [_dL(700, f, C, seed=f) for f in codes]
    fin = _sg(codes, means, values, conics, samples, dLs)
    k = 333
    hot = [d.copy() for d in dLs]
    for d in hot:
        d[k] = np.inf
    got = _sg(codes, means, values, conics, samples, hot)
    keep = np.arange(700) != k
    assert np.isfinite(fin).all() and fin[k].any()
    assert not np.isfinite(got[k]).all()
    assert np.array_equal(got[keep], fin[keep])


# ---- 11. translation identity on the GPU
@pytest.mark.parametrize("function", [0, 3])
def test_sgrad_translation_identity(dgs, function):
    """sum_n ds_n (new call) = -sum_p dmeans_p (_C.volume_backward), within the sum of the 8c bounds
    of the summed entries, taken from the references' values."""
    from diff_gaussian_sampling import _C
    means, values, _, conics = _field(1000, 3, function)
    samples = vo.samples3(2000, seed=14)
    dL = _dL(2000, function, 3)
    m, v, c, s, d = _dev(means, values, conics, samples, dL)
    buf = _C.volume_preprocess(m, c, s, False)
    ds = _C.volume_samples_backward([function], m, v, c, s, [d], buf, False).double().cpu().numpy()
    dm = _C.volume_backward(function, m, v, c, s, buf, d, False)[0].double().cpu().numpy()
    rs = vr.dsamples(function, means, values, conics, samples, dL)
    rm = vo.backward(function, means, values, conics, samples, dL)[0]
    bound = vr.bound8c(rs, RTOL, ATOL).sum(0) + vr.bound8c(rm, RTOL, ATOL).sum(0)
    err = np.abs(ds.sum(0) + dm.sum(0))
    print("translation identity fn", function, "err / bound", err / bound)
    assert (err <= bound).all(), (err, bound)


# ---- 12. autograd with sample_grad=True
def _sampler_inputs(P, N, C, seed):
    means, values, covs, conics = _field(P, C, seed)
    samples = vo.samples3(N, seed=seed)
    return means, values, covs, conics, samples


@pytest.mark.parametrize("function", [0, 1, 2, 3])
def test_sampler_sample_grad_autograd(dgs, function, monkeypatch):
    from diff_gaussian_sampling import _C
    from diff_gaussian_sampling.volume import VolumeSampler
    means, values, covs, conics, samples = _sampler_inputs(400, 600, 2, 30 + function)
    calls = []
    real = _C.volume_samples_backward
    monkeypatch.setattr(_C, "volume_samples_backward", lambda *a: calls.append(1) or real(*a))
    method = ("sample_gaussians", "sample_gaussians_derivative", "sample_gaussians_laplacian",
              "sample_gaussians_third_derivative")[function]
    dL = _dL(600, function, 2)

    def run(sampler, samples_need_grad):
        m, v, cv, c, s = _dev(means, values, covs, conics, samples)
        for t in (m, v, c):
            t.requires_grad_(True)
        s.requires_grad_(samples_need_grad)
        sampler.preprocess(m, v, cv, c, s)
        out = getattr(sampler, method)()
        (out * _dev(dL)[0].reshape(out.shape)).sum().backward()
        return m, v, c, s, out

    m0, v0, c0, s0, _ = run(VolumeSampler(False), False)  # the default sampler, detached samples
    assert s0.grad is None and not calls
    m1, v1, c1, s1, _ = run(VolumeSampler(False, sample_grad=True), False)  # opted in, nothing to do
    assert s1.grad is None and not calls
    vs = VolumeSampler(False, sample_grad=True)
    m, v, c, s, out = run(vs, True)
    assert len(calls) == 1
    for a, b, d in zip((m, v, c), (m0, v0, c0), (m1, v1, c1)):
        assert torch.equal(a.grad, b.grad) and torch.equal(a.grad, d.grad)
    ref = vr.dsamples(function, means, values, conics, samples, dL)
    close(s.grad.cpu().numpy(), ref, RTOL, ATOL, f"autograd fn{function} dsamples")
    if function != 2:
        return
    # the moving-collocation-point loop: an in-place step, the sampler re-bins
    with torch.no_grad():
        s -= (0.01 / float(s.grad.abs().max())) * s.grad
        s.grad = None
    moved = s.detach().cpu().numpy()
    assert np.abs(moved - samples).max() > 1e-3
    out = getattr(vs, method)()
    (out * _dev(dL)[0].reshape(out.shape)).sum().backward()
    close(out.detach().cpu().numpy().reshape(600, 9, 2), vo.forward(2, means, values, conics, moved), RTOL, ATOL,
          "laplacian after the step")
    close(s.grad.cpu().numpy(), vr.dsamples(2, means, values, conics, moved, dL), RTOL, ATOL,
          "dsamples after the step")


@pytest.mark.parametrize("C", [1, 2])
def test_sampler_sample_grad_multi_with_unused_output(dgs, C, monkeypatch):
    """sample_gaussians_multi with an output the loss does not use: one sample-gradient call over
    the outputs whose gradient is not None (C = 1: one fused walk; C = 2: the per-function calls
    added), equal to the reference of the two used functions."""
    from diff_gaussian_sampling import _C
    from diff_gaussian_sampling.volume import VolumeSampler
    means, values, covs, conics, samples = _sampler_inputs(400, 600, C, 41)
    seen = []
    real = _C.volume_samples_backward
    monkeypatch.setattr(_C, "volume_samples_backward", lambda codes, *a: seen.append(list(codes)) or real(codes, *a))
    dLs = {f: _dL(600, f, C, seed=7 + f, scale=0.01 ** f) for f in (0, 2)}

    def run(sampler, samples_need_grad):
        m, v, cv, c, s = _dev(means, values, covs, conics, samples)
        for t in (m, v, c):
            t.requires_grad_(True)
        s.requires_grad_(samples_need_grad)
        sampler.preprocess(m, v, cv, c, s)
        g, _unused, lap = sampler.sample_gaussians_multi("gaussian", "derivative", "laplacian")
        ((g * _dev(dLs[0])[0].reshape(g.shape)).sum() + (lap * _dev(dLs[2])[0].reshape(lap.shape)).sum()).backward()
        return m, v, c, s

    m0, v0, c0, s0 = run(VolumeSampler(False), False)
    assert not seen
    m, v, c, s = run(VolumeSampler(False, sample_grad=True), True)
    # one call; autograd hands an unused output a zero gradient unless it is None (then it is left out)
    assert len(seen) == 1 and {0, 2} <= set(seen[0]) <= {0, 1, 2}
    for a, b in zip((m, v, c), (m0, v0, c0)):
        assert torch.equal(a.grad, b.grad)
    ref = vr.dsamples_multi((0, 2), means, values, conics, samples, [dLs[0], dLs[2]])
    close(s.grad.cpu().numpy(), ref, RTOL, ATOL, f"autograd multi C{C} dsamples")


def test_sample_grad_multi_backward_leaves_none_gradients_out(dgs, monkeypatch):
    """An output whose incoming gradient is None is left out of both backward calls; all None
    returns (None,) * 7 without a call (the rule of _SampleVolumeMulti)."""
    from types import SimpleNamespace
    from diff_gaussian_sampling import _C
    from diff_gaussian_sampling.volume import _SampleVolumeMultiSG
    means, values, _, conics, samples = _sampler_inputs(200, 300, 1, 43)
    m, v, c, s = _dev(means, values, conics, samples)
    seen = []
    real = _C.volume_samples_backward
    monkeypatch.setattr(_C, "volume_samples_backward", lambda codes, *a: seen.append(list(codes)) or real(codes, *a))
    dLs = [_dL(300, f, 1, seed=7 + f, scale=0.01 ** f) for f in (0, 2)]
    g0, g2 = _dev(*dLs)
    ctx = SimpleNamespace(saved_tensors=(m, v, c, s, _C.volume_preprocess(m, c, s, False)), codes=(0, 1, 2), debug=False,
                          needs_input_grad=(False, True, True, True, True, False, False))
    assert _SampleVolumeMultiSG.backward(ctx, None, None, None) == (None,) * 7 and not seen
    out = _SampleVolumeMultiSG.backward(ctx, g0, None, g2)
    assert seen == [[0, 2]] and out[0] is None and out[5] is None and out[6] is None
    close(out[4].cpu().numpy(), vr.dsamples_multi((0, 2), means, values, conics, samples, dLs), RTOL, ATOL,
          "live outputs only dsamples")
    ctx.needs_input_grad = (False, True, True, True, False, False, False)
    assert _SampleVolumeMultiSG.backward(ctx, g0, None, g2)[4] is None and len(seen) == 1


# ---- 13. ctypes
@pytest.mark.parametrize("mask,C", [(4, 1), (15, 1), (8, 9)])
def test_sgrad_ctypes_is_the_extension(dgs, mask, C):
    from diff_gaussian_sampling import _C
    lib = ctypes.CDLL(os.path.join(os.path.dirname(_C.__file__), "libdgs.so"))
    VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.dgs_volume_backward_samples.argtypes = [I] * 4 + [VP] * 6 + [SZ, VP, VP, SZ, VP, I]
    lib.dgs_volume_sample_grad_workspace_size.restype = SZ
    lib.dgs_volume_sample_grad_workspace_size.argtypes = [I] * 4
    codes = _codes(mask)
    means, values, _, conics = _field(500, C, 9)
    samples = vo.samples3(800, seed=15)
    m, v, c, s = _dev(means, values, conics, samples)
    dls = _dev(*[_dL(800, f, C, seed=f, scale=0.01 ** f) for f in codes])
    buf = _C.volume_preprocess(m, c, s, False)
    ext = _C.volume_samples_backward(codes, m, v, c, s, list(dls), buf, False)
    torch.cuda.synchronize()  # (the call below runs on the null stream)
    ws = lib.dgs_volume_sample_grad_workspace_size(mask, 500, 800, C)
    work = torch.empty(max(ws, 4), dtype=torch.uint8, device=m.device)
    ptrs = (VP * 4)()
    for f, d in zip(codes, dls):
        ptrs[f] = d.data_ptr()
    ds = torch.full((800, 3), float("nan"), device=m.device)
    assert lib.dgs_volume_backward_samples(mask, 500, 800, C, *(t.data_ptr() for t in (m, v, c, s)), ptrs,
                                           buf.data_ptr(), buf.numel(), ds.data_ptr(), work.data_ptr(), ws,
                                           None, 0) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(ds).all() and torch.equal(ds, ext)
