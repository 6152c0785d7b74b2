"""GPU parity of the trace of the laplacian of a D = 3 field (function 4, "laplacian_trace":
dgs_volume_*_ops, _C.volume_*_ops, VolumeSampler.sample_gaussians_laplacian_trace; DESIGN.md 4.8,
"Trace Laplacian"), alone at any C and fused with the gaussian, the derivative and the third
derivative at C <= 4: forward, the gradients of means, values and conics, and the sample gradient.

Authority: tests/volume_trace_ref.py, the brute-force oracle's laplacian contracted (and its
gradients for an upstream gradient placed on the diagonal); for the other functions the oracle and
tests/volume_sample_grad_ref.py.  Bound: SURVEY 8c, |d| <= 1e-5 |ref| + 1e-6 max|ref|, max|ref| over
the contracted reference, for the outputs and for the gradients of the summed loss.  Fields and
upstream gradients are those of tests/test_gpu_volume_multi.py / test_gpu_volume_multi_c.py; the
trace's upstream gradient (normal, seed 11) is scaled by 0.01**2 as function 2's is, which keeps
every function's gradient maxima within a factor of 10 of the others' (asserted below), so the
bound on a sum sees every function.  The oracle runs once per case and module."""
import os
import sys

import numpy as np
import pytest
import torch

import volume_sample_grad_ref as vr
import volume_trace_ref as tr
from helpers import close, margin_of, record_margin
from oracle import volume as vo
from test_gpu_volume_multi import Case, _field, _with_big
from test_gpu_volume_multi_c import _chunk_case, _parity

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
T = 4  # the trace's code
TRACE_MASKS = [17, 18, 19, 24, 25, 26, 27]  # the trace with a non-empty subset of {0, 1, 3}


def _codes(mask):
    return [f for f in range(5) if (mask >> f) & 1]


def _k(f):
    return 1 if f == T else 3 ** f


def _shape(N, f, C):
    return (N, C) if f == T else (N,) + (3,) * f + (C,)


class TCase(Case):
    """A Case with function 4: its upstream gradient dL[4] [N, C] and the contracted references
    (fwd(4) is [N, 1, C]).  of(case) shares the arrays and the oracle's cached results."""

    def __init__(self, means, values, conics, samples):
        super().__init__(means, values, conics, samples)
        self.dL = self.dL + [(np.random.default_rng(7 + T).normal(size=(self.N, self.C)) * 0.01 ** 2).astype(np.float32)]
        self._sg = {}

    @classmethod
    def of(cls, case):
        t = cls(case.means, case.values, case.conics, case.samples)
        t._fwd, t._bwd = case._fwd, case._bwd
        t._sg = case.__dict__.setdefault("_sg", {})
        return t

    def fwd(self, f):
        if f == T and f not in self._fwd:
            self._fwd[f] = tr.forward(self.means, self.values, self.conics, self.samples)[:, None, :]
            self._fwd[f].setflags(write=False)
        return self._fwd[f] if f == T else super().fwd(f)

    def bwd(self, f):
        if f == T and f not in self._bwd:
            self._bwd[f] = tr.backward(self.means, self.values, self.conics, self.samples, self.dL[T])
            for g in self._bwd[f]:
                g.setflags(write=False)
        return self._bwd[f] if f == T else super().bwd(f)

    def sref(self, f):
        if f not in self._sg:
            a = (self.means, self.values, self.conics, self.samples, self.dL[f])
            self._sg[f] = tr.dsamples(*a) if f == T else vr.dsamples(f, *a)
            self._sg[f].setflags(write=False)
        return self._sg[f]

    def sref32(self, codes):
        """one float32 serial order of the summed sample gradient"""
        out = np.zeros((self.N, 3), np.float32)
        for f in codes:
            a = (self.means, self.values, self.conics, self.samples, self.dL[f])
            out = out + (tr.dsamples(*a, dtype=np.float32) if f == T else vr.dsamples(f, *a, dtype=np.float32))
        return out


_tcases = {}


def _tparity(C):
    if ("parity", C) not in _tcases:
        _tcases[("parity", C)] = TCase.of(_parity(C))
    return _tcases[("parity", C)]


def _tbig(C):
    if ("big", C) not in _tcases:
        means, values, _, conics = _field(600, C, 7)
        _tcases[("big", C)] = TCase(means, values, _with_big(conics), vo.samples3(1200, seed=8))
    return _tcases[("big", C)]


def _run(case, codes, debug=False, dL=None, sgrad=True):
    """forward, backward and sample gradient through the _ops bindings on one binning; numpy"""
    from diff_gaussian_sampling import _C
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, debug)
    outs = _C.volume_forward_ops(list(codes), m, v, c, s, buf, debug)
    dL = case.dL if dL is None else dL
    dls = [torch.from_numpy(dL[f]).to(m.device) for f in codes]
    grads = tuple(g.cpu().numpy() for g in _C.volume_backward_ops(list(codes), m, v, c, s, dls, buf, debug))
    ds = _C.volume_samples_backward_ops(list(codes), m, v, c, s, dls, buf, debug).cpu().numpy() if sgrad else None
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], grads, ds


def _check(case, codes, what, debug=False, sgrad=True):
    outs, grads, ds = _run(case, codes, debug, sgrad=sgrad)
    for f, o in zip(codes, outs):
        assert o.shape == _shape(case.N, f, case.C)
        ref = case.fwd(f)
        if f == T and os.environ.get("DGS_MARGINS") and case.means.shape[0] and case.N:
            serial = tr.forward(case.means, case.values, case.conics, case.samples, np.float32)
            record_margin(f"{what} {tuple(codes)} fn4 forward [float32 serial order vs float64]",
                          margin_of(serial, ref[:, 0, :], RTOL, ATOL), RTOL, ATOL, int(ref.size))
        close(o.reshape(case.N, _k(f), case.C), ref, RTOL, ATOL, f"{what} {tuple(codes)} fn{f} forward")
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        ref = sum(case.bwd(f)[k] for f in codes)
        assert grads[k].shape == ref.shape
        close(grads[k], ref, RTOL, ATOL, f"{what} {tuple(codes)} {name}")
    if sgrad:
        ref = sum(case.sref(f) for f in codes)
        assert ds.shape == (case.N, 3)
        if os.environ.get("DGS_MARGINS") and case.means.shape[0] and case.N:
            record_margin(f"{what} {tuple(codes)} dsamples [float32 serial order vs float64]",
                          margin_of(case.sref32(codes), ref, RTOL, ATOL), RTOL, ATOL, int(ref.size))
        close(ds, ref, RTOL, ATOL, f"{what} {tuple(codes)} dsamples")
    return outs, grads, ds


# ---- 1. the trace alone
@pytest.mark.parametrize("C", [1, 3, 9])
def test_trace_single_parity(dgs, C):
    """C = 3: a partial channel block of 4; C = 9: a full block of 8 and a block of one channel"""
    _check(_tparity(C), (T,), f"trace parity C{C}")


# ---- 2. the fused masks
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_upstream_scaling_balances_the_functions(C):
    """From the references alone: with dL_f scaled by 0.01**f (the trace as function 2) no function's
    gradient is more than 10x another's, so the bound on a summed gradient sees every function."""
    case = _tparity(C)
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        mx = [float(np.abs(case.bwd(f)[k]).max()) for f in (0, 1, 3, T)]
        print(C, name, mx, max(mx) / min(mx))
        assert max(mx) <= 10.0 * min(mx), (name, mx)
    if C == 3:
        mx = [float(np.abs(case.sref(f)).max()) for f in (0, 1, 3, T)]
        print(C, "dsamples", mx, max(mx) / min(mx))
        assert max(mx) <= 10.0 * min(mx), mx


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mask", TRACE_MASKS)
def test_trace_fused_parity(dgs, mask, C):
    _check(_tparity(C), _codes(mask), f"trace fused parity C{C}", sgrad=(C == 3 or mask in (19, 27)))


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("mask", [19, 27])
def test_trace_fused_parity_partial_and_full_block(dgs, mask, C):
    _check(_tparity(C), _codes(mask), f"trace fused parity C{C}")


# ---- 3. bitwise invariants
@pytest.mark.parametrize("C", [1, 3])
def test_fused_outputs_are_bitwise_the_single_calls(dgs, C):
    """every output of a fused trace mask, the trace's included, on the parity and the big field"""
    from diff_gaussian_sampling import _C
    for case in (_tparity(C), _tbig(C)):
        m, v, c, s = case.dev()
        buf = _C.volume_preprocess(m, c, s, False)
        single = {f: _C.volume_forward(f, m, v, c, s, buf, False) for f in (0, 1, 3)}
        single[T] = _C.volume_forward_ops([T], m, v, c, s, buf, False)[0]
        assert torch.isfinite(single[T]).all() and single[T].abs().max() > 0
        for mask in TRACE_MASKS:
            codes = _codes(mask)
            for f, o in zip(codes, _C.volume_forward_ops(codes, m, v, c, s, buf, False)):
                assert torch.equal(o, single[f]), (C, mask, f, float((o - single[f]).abs().max()))


def test_masks_below_16_are_the_fused_entry(dgs):
    """dgs_volume_*_ops with a mask below 16 (five-pointer arrays) against dgs_volume_*_fused"""
    from diff_gaussian_sampling import _C
    import dgs_ctypes
    case = _tparity(3)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    v1 = v[:, :1].contiguous()
    for codes, vv, C in (([0, 1, 2], v, 3), ([2], v, 3), ([0, 1, 2, 3], v1, 1), ([1], v1, 1)):
        dls = [torch.from_numpy(np.ascontiguousarray(case.dL[f][:, :, :C])).to(m.device) for f in codes]
        res = {}
        for e in ("ops", "fused"):
            res[e] = (dgs_ctypes.volume_forward_fused(codes, m, vv, c, s, buf, False, entry=e)
                      + list(dgs_ctypes.volume_backward_fused(codes, m, vv, c, s, dls, buf, False, entry=e))
                      + [dgs_ctypes.volume_samples_backward_fused(codes, m, vv, c, s, dls, buf, False, entry=e)])
        torch.cuda.synchronize()
        for a, b in zip(res["ops"], res["fused"]):
            assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b), codes
        mask = sum(1 << f for f in codes)
        assert (dgs_ctypes.volume_workspace_size_ops(mask, 1000, 2000, C, 1)
                == dgs_ctypes.volume_workspace_size_fused(mask, 1000, 2000, C, 1))


def test_trace_repeatable_and_debug(dgs):
    for case, codes in ((_tbig(3), (0, 1, 3, T)), (_tbig(3), (T,)), (_tbig(1), (0, 1, T))):
        a, ga, sa = _run(case, codes)
        b, gb, sb = _run(case, codes)
        d, gd, sd = _run(case, codes, debug=True)
        for x, y, z in zip(a + list(ga) + [sa], b + list(gb) + [sb], d + list(gd) + [sd]):
            assert np.isfinite(x).all()
            assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- 4. special fields and sizes
@pytest.mark.parametrize("codes", [(T,), (0, 3, T), (0, 1, 3, T)])
def test_trace_big_gaussians(dgs, codes):
    """wide, ill-conditioned, indefinite (power > 0 skipped) and nearly singular conics at C = 3"""
    _check(_tbig(3), codes, "trace big C3")


def test_trace_big_gaussians_c1(dgs):
    """The C = 1 kernels (k_vol_backward_big_m) on the same field: the outputs and the parameters'
    gradients.  The sample gradient is not compared on this field at C = 1: the reference's own
    float32 serial order of it is 1.06 of the bound there (one sample next to the nearly singular
    conic; profiles/volume_trace_margins.json), so the field, not a kernel, decides that check.  The
    C = 3 field above, where that order is within the bound, carries the sample gradient."""
    case = _tbig(1)
    if os.environ.get("DGS_MARGINS"):  # the figure above, from the references alone
        record_margin("trace big C1 (4,) dsamples [float32 serial order vs float64]",
                      margin_of(case.sref32((T,)), case.sref(T), RTOL, ATOL), RTOL, ATOL, case.N * 3)
    _check(case, (T,), "trace big C1", sgrad=False)
    _check(case, (0, 1, T), "trace big C1", sgrad=False)


@pytest.mark.parametrize("codes", [(T,), (0, 1, T)])
def test_trace_seams_and_images(dgs, codes):
    """the construction of test_gpu_volume_multi_c.test_fused_seams_and_images at C = 2"""
    if "seams" not in _tcases:
        rng = np.random.default_rng(2)
        means, values, _, conics = _field(400, 2, 2)
        means[:100, 0] = np.float32(0.999)
        means[100:200, 1] = np.float32(-0.999)
        means[200:220] = rng.uniform(2.5, 3.5, (20, 3)).astype(np.float32)  # far outside: images
        samples = vo.samples3(1500, seed=3)
        samples[:300, 0] = np.float32(-0.998)
        samples[300:400] = rng.uniform(-3.2, -2.8, (100, 3)).astype(np.float32)
        _tcases["seams"] = TCase(means, values, conics, samples)
    _check(_tcases["seams"], codes, "trace seams C2")


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_trace_chunk_boundaries(dgs, C, last):
    """150 Gaussians and 200 samples in one cell (several 64-wide batches with a partial last one, in
    the lane = sample and the lane = Gaussian nests), the cluster's samples first and then last"""
    case = TCase.of(_chunk_case(C, cluster_last=last))
    _check(case, (T,), f"trace chunks C{C}")
    _check(case, (0, 1, 3, T), f"trace chunks C{C}")


@pytest.mark.parametrize("C", [1, 3])
def test_trace_edge_sizes(dgs, C):
    means, values, _, conics = _field(50, C, 1)
    samples = vo.samples3(65, seed=1)
    for P, N in ((0, 40), (50, 0), (1, 1), (50, 65)):
        case = TCase(means[:P], values[:P], conics[:P], samples[:N])
        for codes in ((T,), (0, 1, T)):
            outs, grads, ds = _check(case, codes, f"trace edge P{P} N{N} C{C}")
            if P == 0:
                assert not ds.any() and not any(o.any() for o in outs)
            if N == 0:
                assert not any(g.any() for g in grads)


# ---- 5. the row past the end
@pytest.mark.parametrize("codes", [(T,), (0, 1, T)])
def test_trace_padded_channels_are_never_read(dgs, codes):
    """C = 3 with the last sample by index among the staged candidates and NaN bit patterns behind
    hs in an oversized workspace: a padded channel that was read (and multiplied by 0 instead of
    selected to 0) would put NaN into the gradients of the Gaussians that meet that sample."""
    from diff_gaussian_sampling import _C
    import dgs_ctypes
    case = TCase.of(_chunk_case(3, cluster_last=True))
    N, C, mask = case.N, 3, sum(1 << f for f in codes)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
    need = dgs_ctypes.volume_workspace_size_ops(mask, 250, N, C, 1)
    assert need == N * (1 if mask == 16 else 5) * C * 4
    work = torch.full((need // 4 + 4096,), float("nan"), device=m.device).view(torch.uint8)
    torch.cuda.synchronize()
    grads = dgs_ctypes.volume_backward_fused(codes, m, v, c, s, dls, buf, False, entry="ops", workspace=work)
    torch.cuda.synchronize()
    assert torch.isnan(work.view(torch.float32)[need // 4:]).all()  # nothing written behind hs either
    G = vo._pairs(case.means, case.conics, case.samples[N - 1:])[1]
    assert (np.asarray(G) > 0).sum() >= 100  # the last sample's pairs are live
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        g = grads[k].cpu().numpy()
        assert np.isfinite(g).all(), name
        close(g, sum(case.bwd(f)[k] for f in codes), RTOL, ATOL, f"trace padded channels C3 {tuple(codes)} {name}")


# ---- 6. locality of a non-finite upstream gradient
@pytest.mark.parametrize("codes", [(T,), (0, 1, T)])
def test_trace_nonfinite_dl_stays_local(dgs, codes):
    """dL = +inf in the trace's upstream gradient at one sample (C = 3): every other sample's
    dL_dsamples is bit for bit unchanged, and the Gaussians with a non-finite gradient row are among
    those whose pair set holds that sample (G > 0 by the oracle) and include every one of them whose
    G is far from the flush (G > 1e-30)."""
    case, j = _tparity(3), 1234
    inf = [x.copy() for x in case.dL]
    inf[T][j] = np.inf
    _, g0, ds0 = _run(case, codes)
    _, g1, ds1 = _run(case, codes, dL=inf)
    keep = np.arange(case.N) != j
    assert np.isfinite(ds0).all() and ds0[j].any()
    assert not np.isfinite(ds1[j]).all()
    assert np.array_equal(ds0[keep], ds1[keep])
    G = np.asarray(vo._pairs(case.means, case.conics, case.samples[j:j + 1])[1])[:, 0]
    bad = np.zeros(case.means.shape[0], bool)
    for a, fin in zip(g1, g0):
        assert np.isfinite(fin).all()
        bad |= ~np.isfinite(a).all(axis=1)
    assert 0 < bad.sum() < bad.size
    assert not (bad & ~(G > 0)).any(), int((bad & ~(G > 0)).sum())
    assert bad[G > 1e-30].all()
    for a, fin in zip(g1, g0):  # the other Gaussians' rows: bit for bit the finite run's
        assert np.array_equal(a[~bad], fin[~bad])


# ---- 7. loud on stale input
def test_trace_stale_buffer_is_loud(dgs):
    from diff_gaussian_sampling import _C
    dev = torch.device("cuda:0")
    means, values, _, conics = (torch.from_numpy(x).to(dev) for x in _field(100, 3, 1))
    s = torch.from_numpy(vo.samples3(200)).to(dev)

    def all_nan(m, buf, cs, vals=values):
        outs = _C.volume_forward_ops(cs, m, vals, conics, s, buf, False)
        dls = [torch.ones_like(o) for o in outs]
        res = list(outs) + list(_C.volume_backward_ops(cs, m, vals, conics, s, dls, buf, False))
        res.append(_C.volume_samples_backward_ops(cs, m, vals, conics, s, dls, buf, False))
        return [bool(torch.isnan(t).all()) and t.numel() > 0 for t in res], [bool(torch.isfinite(t).all()) for t in res]

    v1, v9 = values[:, :1].contiguous(), torch.cat([values] * 3, 1).contiguous()
    runs = (([0, 1, T], values), ([T], values), ([0, 1, T], v1), ([T], v1), ([T], v9))
    other = _C.volume_preprocess(means, conics, s[:100].contiguous(), False)  # a binning of other sizes
    buf = _C.volume_preprocess(means, conics, s, False)
    for cs, vals in runs:
        assert all(all_nan(means, other, cs, vals)[0]), cs
        assert all(all_nan(means, buf, cs, vals)[1]), cs  # fresh: finite
    means[7, 0] += 1e-3  # changed in place after the binning
    for cs, vals in runs:
        assert all(all_nan(means, buf, cs, vals)[0]), cs


# ---- 8. the Python routing
def test_trace_python_routing(dgs):
    from diff_gaussian_sampling import _C
    from diff_gaussian_sampling.volume import FUNCTION_CODES, sample_volume, sample_volume_multi
    assert FUNCTION_CODES["laplacian_trace"] == T
    case = _tparity(3)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    with pytest.raises(RuntimeError):
        _C.volume_forward_multi([T], m, v, c, s, buf, False)  # the older bindings keep refusing it
    with pytest.raises(RuntimeError):
        _C.volume_forward(T, m, v, c, s, buf, False)
    single = sample_volume("laplacian_trace", m, v, c, s, buf)
    assert single.shape == (case.N, 3)
    lap, trc, g = sample_volume_multi(("laplacian", "laplacian_trace", "gaussian"), m, v, c, s, buf)
    assert lap.shape == (case.N, 3, 3, 3) and trc.shape == (case.N, 3) and g.shape == (case.N, 3)
    assert torch.equal(trc, single)
    assert torch.equal(lap, _C.volume_forward(2, m, v, c, s, buf, False))
    assert torch.equal(g, _C.volume_forward(0, m, v, c, s, buf, False))
    # the GPU trace against the contraction of the GPU laplacian, within the bound
    contracted = lap.diagonal(dim1=1, dim2=2).sum(-1).cpu().numpy()
    close(trc.cpu().numpy(), contracted, RTOL, ATOL, "trace vs contracted GPU laplacian C3")
    # both at once in the backward: the trace's own call added to the fused rest
    codes = (2, T, 0)
    dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
    grads = _C.volume_backward_ops(list(codes), m, v, c, s, dls, buf, False)
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        close(grads[k].cpu().numpy(), sum(case.bwd(f)[k] for f in codes), RTOL, ATOL, f"trace + laplacian C3 {name}")
    ds = _C.volume_samples_backward_ops(list(codes), m, v, c, s, dls, buf, False)
    close(ds.cpu().numpy(), sum(case.sref(f) for f in codes), RTOL, ATOL, "trace + laplacian C3 dsamples")


def test_trace_fallback_above_four_channels(dgs):
    """several functions with the trace at C = 5: every function on its own, gradients added"""
    if "c5" not in _tcases:
        means, values, _, conics = _field(200, 5, 9)
        _tcases["c5"] = TCase(means, values, conics, vo.samples3(300, seed=9))
    _check(_tcases["c5"], (0, 1, T), "trace fallback C5")


# ---- 9. autograd through VolumeSampler
def test_trace_sampler_autograd(dgs):
    from diff_gaussian_sampling.volume import VolumeSampler
    dev = torch.device("cuda:0")
    P, N, C = 500, 600, 3
    means, values, covs, conics = _field(P, C, 8)
    samples = vo.samples3(N, seed=8)
    case = TCase(means, values, conics, samples)
    w = {f: torch.from_numpy(case.dL[f]).to(dev).reshape(_shape(N, f, C)) for f in (0, 1, T)}

    def leaves(smp):
        ts = [torch.from_numpy(x).to(dev) for x in (means, values, covs, conics, smp)]
        for t in (ts[0], ts[1], ts[3], ts[4]):
            t.requires_grad_(True)
        return ts

    # the single call
    m, v, cv, c, s = leaves(samples)
    vs = VolumeSampler(False, sample_grad=True)
    vs.preprocess(m, v, cv, c, s)
    out = vs.sample_gaussians_laplacian_trace()
    assert out.shape == (N, C)
    (out * w[T]).sum().backward()
    close(out.detach().cpu().numpy()[:, None, :], case.fwd(T), RTOL, ATOL, "autograd trace C3 forward")
    for k, (name, t) in enumerate((("dmeans", m), ("dvalues", v), ("dconics", c))):
        close(t.grad.cpu().numpy(), case.bwd(T)[k], RTOL, ATOL, f"autograd trace C3 {name}")
    close(s.grad.cpu().numpy(), case.sref(T), RTOL, ATOL, "autograd trace C3 dsamples")

    # the residual's three functions, the derivative's output unused
    m, v, cv, c, s = leaves(samples)
    vs = VolumeSampler(False, sample_grad=True)
    vs.preprocess(m, v, cv, c, s)
    outs = dict(zip((0, 1, T), vs.sample_gaussians_multi("gaussian", "derivative", "laplacian_trace")))
    assert [tuple(outs[f].shape) for f in (0, 1, T)] == [_shape(N, f, C) for f in (0, 1, T)]
    sum((outs[f] * w[f]).sum() for f in (0, T)).backward()
    for f in (0, 1, T):
        close(outs[f].detach().cpu().numpy().reshape(N, _k(f), C), case.fwd(f), RTOL, ATOL, f"autograd C3 fn{f} forward")
    for k, (name, t) in enumerate((("dmeans", m), ("dvalues", v), ("dconics", c))):
        close(t.grad.cpu().numpy(), sum(case.bwd(f)[k] for f in (0, T)), RTOL, ATOL, f"autograd C3 {name}")
    close(s.grad.cpu().numpy(), sum(case.sref(f) for f in (0, T)), RTOL, ATOL, "autograd C3 dsamples")

    # an in-place step of the means: the sampler re-bins
    binned = vs.binning
    with torch.no_grad():
        m -= (0.005 / float(m.grad.abs().max())) * m.grad
        for t in (m, v, c, s):
            t.grad = None
    moved = m.detach().cpu().numpy()
    assert np.abs(moved - means).max() > 1e-3
    g, trc = vs.sample_gaussians_multi("gaussian", "laplacian_trace")
    assert vs.binning is not binned
    ((g * w[0]).sum() + (trc * w[T]).sum()).backward()
    after = TCase(moved, values, conics, samples)
    close(trc.detach().cpu().numpy()[:, None, :], after.fwd(T), RTOL, ATOL, "trace C3 after the step")
    close(m.grad.cpu().numpy(), sum(after.bwd(f)[0] for f in (0, T)), RTOL, ATOL, "dmeans C3 after the step")
    close(s.grad.cpu().numpy(), sum(after.sref(f) for f in (0, T)), RTOL, ATOL, "dsamples C3 after the step")

    # without sample_grad, samples that require a gradient raise
    m, v, cv, c, s = leaves(samples)
    vs = VolumeSampler(False)
    vs.preprocess(m, v, cv, c, s)
    with pytest.raises(NotImplementedError):
        vs.sample_gaussians_laplacian_trace()
    with pytest.raises(NotImplementedError):
        vs.sample_gaussians_multi("gaussian", "laplacian_trace")
