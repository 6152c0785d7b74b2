"""GPU parity of the constant-coefficient linear operator of a D = 3 field (function 5:
dgs_volume_*_linop, _C.volume_*_linop, diff_gaussian_sampling.volume.LinearOperator; DESIGN.md 4.8,
"Linear operator"), alone at any C and fused with the gaussian and the derivative at C <= 4: forward,
the gradients of means, values and conics, and the sample gradient.

Authority: tests/volume_linop_ref.py, the brute-force oracle's gaussian, derivative and laplacian
combined (and their gradients for the lifted upstream gradient); for the other functions the oracle
and tests/volume_sample_grad_ref.py.  Bound: SURVEY 8c, |d| <= 1e-5 |ref| + 1e-6 max|ref|, max|ref|
over the operator's reference, for the outputs and for the gradients of the summed loss.  The
coefficient sets are volume_linop_ref.SETS; tests/test_volume_linop_ref.py shows on the CPU that the
reference's own float32 order stays within 0.9 of the bound for every set and field compared here
(forward at most 0.51, sample gradient at most 0.46), so no comparison is left out.  Fields and the
upstream gradients of functions 0 and 1 are those of tests/test_gpu_volume_multi_c.py (dL_f scaled by
0.01**f); the operator's is normal, seed 12, unscaled: the `balanced` set weighs u, grad u and the
Hessian by about 1, 0.01 and 0.01**2, which keeps every function's gradient maxima within a factor
of 10 of the others' (asserted below).  The oracle runs once per function, field and module."""
import os
import sys

import numpy as np
import pytest
import torch

import volume_linop_ref as lr
import volume_sample_grad_ref as vr
from helpers import close
from oracle import volume as vo
from test_gpu_volume_multi import Case, _field, _with_big
from test_gpu_volume_multi_c import _chunk_case, _parity

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
OP, T = 5, 4  # the operator's code, the trace's
OP_MASKS = [33, 34, 35]  # the operator with a non-empty subset of {0, 1}
BAL = lr.SETS["balanced"]


def _codes(mask):
    return [f for f in range(6) if (mask >> f) & 1]


def _k(f):
    return 1 if f >= T else 3 ** f


def _shape(N, f, C):
    return (N, C) if f >= T else (N,) + (3,) * f + (C,)


class LCase(Case):
    """A Case with function 5 for one coefficient set: its upstream gradient dL[5] [N, C] and the
    combined references (fwd(5) is [N, 1, C]).  of(case, coef) shares the arrays and the oracle's
    cached per-function results, so the oracle's forward runs once per field."""

    def __init__(self, means, values, conics, samples, coef=BAL):
        super().__init__(means, values, conics, samples)
        self.coef = [float(x) for x in np.asarray(coef, np.float32)]
        self.dL = self.dL + [None, lr.op_dL(self.N, self.C)]
        self._sg, self._op = {}, {}

    @classmethod
    def of(cls, case, coef=BAL):
        t = cls(case.means, case.values, case.conics, case.samples, coef)
        t._fwd, t._bwd = case._fwd, case._bwd
        t._sg = case.__dict__.setdefault("_sg", {})
        return t

    def _empty(self):
        return self.means.shape[0] == 0 or self.N == 0

    def fwd(self, f):
        if f != OP:
            return super().fwd(f)
        if "fwd" not in self._op:
            o = (np.zeros((self.N, self.C)) if self._empty() or not lr.parts(self.coef)
                 else lr.combine(self.coef, {g: super(LCase, self).fwd(g) for g in lr.parts(self.coef)}))
            self._op["fwd"] = o[:, None, :]
            self._op["fwd"].setflags(write=False)
        return self._op["fwd"]

    def bwd(self, f):
        if f != OP:
            return super().bwd(f)
        if "bwd" not in self._op:
            self._op["bwd"] = lr.backward(self.coef, self.means, self.values, self.conics, self.samples, self.dL[OP])
        return self._op["bwd"]

    def sref(self, f):
        if f == OP:
            if "sg" not in self._op:
                self._op["sg"] = lr.dsamples(self.coef, self.means, self.values, self.conics, self.samples, self.dL[OP])
            return self._op["sg"]
        if f not in self._sg:
            self._sg[f] = vr.dsamples(f, self.means, self.values, self.conics, self.samples, self.dL[f])
            self._sg[f].setflags(write=False)
        return self._sg[f]


_lcases = {}


def _lparity(C, name="balanced"):
    if ("parity", C, name) not in _lcases:
        _lcases[("parity", C, name)] = LCase.of(_parity(C), lr.SETS[name])
    return _lcases[("parity", C, name)]


def _lbig(C, name="balanced"):
    if ("big", C) not in _lcases:
        means, values, _, conics = _field(600, C, 7)
        _lcases[("big", C)] = Case(means, values, _with_big(conics), vo.samples3(1200, seed=8))
    if ("big", C, name) not in _lcases:
        _lcases[("big", C, name)] = LCase.of(_lcases[("big", C)], lr.SETS[name])
    return _lcases[("big", C, name)]


def _run(case, codes, debug=False, dL=None, sgrad=True, coef=None):
    """forward, backward and sample gradient through the _linop bindings on one binning; numpy"""
    from diff_gaussian_sampling import _C
    coef = case.coef if coef is None else coef
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, debug)
    outs = _C.volume_forward_linop(list(codes), coef, m, v, c, s, buf, debug)
    dL = case.dL if dL is None else dL
    dls = [torch.from_numpy(dL[f]).to(m.device) for f in codes]
    grads = tuple(g.cpu().numpy() for g in _C.volume_backward_linop(list(codes), coef, m, v, c, s, dls, buf, debug))
    ds = (_C.volume_samples_backward_linop(list(codes), coef, m, v, c, s, dls, buf, debug).cpu().numpy()
          if sgrad else None)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], grads, ds


def _check(case, codes, what, debug=False):
    outs, grads, ds = _run(case, codes, debug)
    for f, o in zip(codes, outs):
        assert o.shape == _shape(case.N, f, case.C)
        close(o.reshape(case.N, _k(f), case.C), case.fwd(f), RTOL, ATOL, f"{what} {tuple(codes)} fn{f} forward")
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        ref = sum(case.bwd(f)[k] for f in codes)
        assert grads[k].shape == ref.shape
        close(grads[k], ref, RTOL, ATOL, f"{what} {tuple(codes)} {name}")
    ref = sum(case.sref(f) for f in codes)
    assert ds.shape == (case.N, 3)
    close(ds, ref, RTOL, ATOL, f"{what} {tuple(codes)} dsamples")
    return outs, grads, ds


# ---- 1. the operator alone
@pytest.mark.parametrize("C", [1, 3, 9])
def test_operator_single_parity_balanced(dgs, C):
    """C = 3: a partial channel block of 4; C = 9: a full block of 8 and a block of one channel"""
    outs, _, _ = _check(_lparity(C), (OP,), f"linop balanced parity C{C}")
    assert np.abs(outs[0]).max() > 0


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", ["lap_xy", "heat", "wave"])
def test_operator_single_parity_pde_sets(dgs, name, C):
    _check(_lparity(C, name), (OP,), f"linop {name} parity C{C}")


# ---- 2. the index mapping
def test_one_hot_coefficients_are_the_components(dgs):
    """the ten one-hot sets at C = 2: each output is the matching unique component of the GPU's own
    gaussian / derivative / laplacian (an off-diagonal w twice it) and of the oracle's, within the
    bound; a wrong packed order or a missing factor 2 fails here"""
    from diff_gaussian_sampling import _C
    if "onehot" not in _lcases:
        means, values, _, conics = _field(300, 2, 4)
        _lcases["onehot"] = Case(means, values, conics, vo.samples3(500, seed=5))
    base = _lcases["onehot"]
    m, v, c, s = base.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    own = [_C.volume_forward(f, m, v, c, s, buf, False).cpu().numpy().reshape(base.N, 3 ** f, 2) for f in range(3)]
    # coefficient q -> (function, full component, factor)
    comp = [(0, 0, 1), (1, 0, 1), (1, 1, 1), (1, 2, 1), (2, 0, 1), (2, 1, 2), (2, 2, 2), (2, 4, 1), (2, 5, 2), (2, 8, 1)]
    for q, (f, full, factor) in enumerate(comp):
        coef = [0.0] * 10
        coef[q] = 1.0
        out = _C.volume_forward_linop([OP], coef, m, v, c, s, buf, False)[0].cpu().numpy()
        assert np.abs(out).max() > 0
        close(out, factor * own[f][:, full, :].astype(np.float64), RTOL, ATOL, f"linop one-hot {q} vs the GPU's fn{f}")
        close(out, factor * base.fwd(f)[:, full, :], RTOL, ATOL, f"linop one-hot {q} vs the oracle's fn{f}")
        close(out, LCase.of(base, coef).fwd(OP)[:, 0, :], RTOL, ATOL, f"linop one-hot {q} vs the reference")


# ---- 3. the fused masks
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_upstream_scaling_balances_the_functions(C):
    """From the references alone: with dL_f scaled by 0.01**f and the balanced operator's unscaled, no
    function's gradient is more than 10x another's, so the bound on a summed gradient sees every one."""
    case = _lparity(C)
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        mx = [float(np.abs(case.bwd(f)[k]).max()) for f in (0, 1, OP)]
        print(C, name, mx, max(mx) / min(mx))
        assert max(mx) <= 10.0 * min(mx), (name, mx)
    mx = [float(np.abs(case.sref(f)).max()) for f in (0, 1, OP)]
    print(C, "dsamples", mx, max(mx) / min(mx))
    assert max(mx) <= 10.0 * min(mx), mx


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mask", OP_MASKS)
def test_operator_fused_parity(dgs, mask, C):
    _check(_lparity(C), _codes(mask), f"linop fused parity C{C}")


@pytest.mark.parametrize("C", [2, 4])
def test_operator_fused_parity_partial_and_full_block(dgs, C):
    _check(_lparity(C), _codes(35), f"linop fused parity C{C}")


@pytest.mark.parametrize("C", [1, 3])
def test_fused_outputs_are_bitwise_the_single_calls(dgs, C):
    """every output of a fused operator mask, the operator's included, on the parity and the big field"""
    from diff_gaussian_sampling import _C
    for case in (_lparity(C), _lbig(C)):
        m, v, c, s = case.dev()
        buf = _C.volume_preprocess(m, c, s, False)
        single = {f: _C.volume_forward(f, m, v, c, s, buf, False) for f in (0, 1)}
        single[OP] = _C.volume_forward_linop([OP], case.coef, m, v, c, s, buf, False)[0]
        assert torch.isfinite(single[OP]).all() and single[OP].abs().max() > 0
        for mask in OP_MASKS:
            codes = _codes(mask)
            for f, o in zip(codes, _C.volume_forward_linop(codes, case.coef, m, v, c, s, buf, False)):
                assert torch.equal(o, single[f]), (C, mask, f, float((o - single[f]).abs().max()))


# ---- 4. the trace
@pytest.mark.parametrize("C", [1, 3])
def test_identity_w_is_the_trace_within_the_bound(dgs, C):
    """W = I against "laplacian_trace" on the GPU (another order of the same roundings: not bitwise)"""
    from diff_gaussian_sampling import _C
    case = _lparity(C)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    coef = [0.0] * 4 + [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    op = _C.volume_forward_linop([OP], coef, m, v, c, s, buf, False)[0].cpu().numpy()
    trace = _C.volume_forward_ops([T], m, v, c, s, buf, False)[0].cpu().numpy()
    assert np.abs(trace).max() > 0
    close(op, trace.astype(np.float64), RTOL, ATOL, f"linop W = I vs the GPU trace C{C}")


# ---- 5. the coefficients are the call's
@pytest.mark.parametrize("C", [1, 3])
def test_coefficients_are_per_call(dgs, C):
    """two sets in turn on one binning, forward and backward, each against its own reference; then the
    first again, bit for bit (nothing of a call's coefficients stays on the device)"""
    from diff_gaussian_sampling import _C
    a, b = _lparity(C, "balanced"), _lparity(C, "heat")
    m, v, c, s = a.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    dl = [torch.from_numpy(a.dL[OP]).to(m.device)]

    def run(case):
        out = _C.volume_forward_linop([OP], case.coef, m, v, c, s, buf, False)[0]
        g = _C.volume_backward_linop([OP], case.coef, m, v, c, s, dl, buf, False)
        ds = _C.volume_samples_backward_linop([OP], case.coef, m, v, c, s, dl, buf, False)
        return [out] + list(g) + [ds]

    ra, rb, ra2 = run(a), run(b), run(a)
    torch.cuda.synchronize()
    for case, res, tag in ((a, ra, "balanced"), (b, rb, "heat")):
        close(res[0].cpu().numpy()[:, None, :], case.fwd(OP), RTOL, ATOL, f"linop per call {tag} C{C} forward")
        for k, name in enumerate(("dmeans", "dvalues", "dconics")):
            close(res[1 + k].cpu().numpy(), case.bwd(OP)[k], RTOL, ATOL, f"linop per call {tag} C{C} {name}")
        close(res[4].cpu().numpy(), case.sref(OP), RTOL, ATOL, f"linop per call {tag} C{C} dsamples")
    for x, y in zip(ra, ra2):
        assert torch.equal(x, y)
    assert not torch.equal(ra[0], rb[0])


# ---- 6. special fields and sizes
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", list(lr.SETS))
def test_operator_big_gaussians(dgs, name, C):
    """wide, ill-conditioned, indefinite (power > 0 skipped) and nearly singular conics; C = 1: the
    mask kernels (k_vol_backward_big_m), C = 3: the per-function ones"""
    _check(_lbig(C, name), (OP,), f"linop {name} big C{C}")


@pytest.mark.parametrize("C", [1, 3])
def test_operator_fused_big_gaussians(dgs, C):
    _check(_lbig(C), (0, 1, OP), f"linop fused big C{C}")


@pytest.mark.parametrize("codes", [(OP,), (0, 1, OP)])
def test_operator_seams_and_images(dgs, codes):
    """the construction of test_gpu_volume_trace.test_trace_seams_and_images at C = 2"""
    if "seams" not in _lcases:
        rng = np.random.default_rng(2)
        means, values, _, conics = _field(400, 2, 2)
        means[:100, 0] = np.float32(0.999)
        means[100:200, 1] = np.float32(-0.999)
        means[200:220] = rng.uniform(2.5, 3.5, (20, 3)).astype(np.float32)  # far outside: images
        samples = vo.samples3(1500, seed=3)
        samples[:300, 0] = np.float32(-0.998)
        samples[300:400] = rng.uniform(-3.2, -2.8, (100, 3)).astype(np.float32)
        _lcases["seams"] = LCase(means, values, conics, samples)
    _check(_lcases["seams"], codes, "linop seams C2")


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_operator_chunk_boundaries(dgs, C, last):
    """150 Gaussians and 200 samples in one cell (several 64-wide batches with a partial last one, in
    the lane = sample and the lane = Gaussian nests), the cluster's samples first and then last"""
    case = LCase.of(_chunk_case(C, cluster_last=last))
    _check(case, (OP,), f"linop chunks C{C}")
    _check(case, (0, 1, OP), f"linop chunks C{C}")


@pytest.mark.parametrize("C", [1, 3])
def test_operator_edge_sizes(dgs, C):
    means, values, _, conics = _field(50, C, 1)
    samples = vo.samples3(65, seed=1)
    for P, N in ((0, 40), (50, 0), (1, 1), (50, 65)):
        case = LCase(means[:P], values[:P], conics[:P], samples[:N])
        for codes in ((OP,), (0, 1, OP)):
            outs, grads, ds = _check(case, codes, f"linop edge P{P} N{N} C{C}")
            if P == 0:
                assert not ds.any() and not any(o.any() for o in outs)
            if N == 0:
                assert not any(g.any() for g in grads)


# ---- 7. the invariants of the trace
@pytest.mark.parametrize("codes", [(OP,), (0, 1, OP)])
def test_operator_padded_channels_are_never_read(dgs, codes):
    """C = 3 with the last sample by index among the staged candidates and NaN bit patterns behind
    hs in an oversized workspace: a padded channel that was read (and multiplied by 0 instead of
    selected to 0) would put NaN into the gradients of the Gaussians that meet that sample."""
    from diff_gaussian_sampling import _C
    import dgs_ctypes
    case = LCase.of(_chunk_case(3, cluster_last=True))
    N, C, mask = case.N, 3, sum(1 << f for f in codes)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
    need = dgs_ctypes.volume_workspace_size_linop(mask, 250, N, C, 1)
    assert need == N * (1 if mask == 32 else 5) * C * 4
    work = torch.full((need // 4 + 4096,), float("nan"), device=m.device).view(torch.uint8)
    torch.cuda.synchronize()
    grads = dgs_ctypes.volume_backward_linop(list(codes), case.coef, m, v, c, s, dls, buf, False, workspace=work)
    torch.cuda.synchronize()
    assert torch.isnan(work.view(torch.float32)[need // 4:]).all()  # nothing written behind hs either
    G = vo._pairs(case.means, case.conics, case.samples[N - 1:])[1]
    assert (np.asarray(G) > 0).sum() >= 100  # the last sample's pairs are live
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        g = grads[k].cpu().numpy()
        assert np.isfinite(g).all(), name
        close(g, sum(case.bwd(f)[k] for f in codes), RTOL, ATOL, f"linop padded channels C3 {tuple(codes)} {name}")


@pytest.mark.parametrize("codes", [(OP,), (0, 1, OP)])
def test_operator_nonfinite_dl_stays_local(dgs, codes):
    """dL = +inf in the operator's upstream gradient at one sample (C = 3): every other sample's
    dL_dsamples is bit for bit unchanged, and the Gaussians with a non-finite gradient row are among
    those whose pair set holds that sample (G > 0 by the oracle) and include every one of them whose
    G is far from the flush (G > 1e-30)."""
    case, j = _lparity(3), 1234
    inf = [None if x is None else x.copy() for x in case.dL]
    inf[OP][j] = np.inf
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


def test_operator_stale_buffer_is_loud(dgs):
    from diff_gaussian_sampling import _C
    dev = torch.device("cuda:0")
    means, values, _, conics = (torch.from_numpy(x).to(dev) for x in _field(100, 3, 1))
    s = torch.from_numpy(vo.samples3(200)).to(dev)

    def all_nan(m, buf, cs, vals=values):
        outs = _C.volume_forward_linop(cs, BAL, m, vals, conics, s, buf, False)
        dls = [torch.ones_like(o) for o in outs]
        res = list(outs) + list(_C.volume_backward_linop(cs, BAL, m, vals, conics, s, dls, buf, False))
        res.append(_C.volume_samples_backward_linop(cs, BAL, m, vals, conics, s, dls, buf, False))
        return [bool(torch.isnan(t).all()) and t.numel() > 0 for t in res], [bool(torch.isfinite(t).all()) for t in res]

    v1, v9 = values[:, :1].contiguous(), torch.cat([values] * 3, 1).contiguous()
    runs = (([0, 1, OP], values), ([OP], values), ([0, 1, OP], v1), ([OP], v1), ([OP], v9))
    other = _C.volume_preprocess(means, conics, s[:100].contiguous(), False)  # a binning of other sizes
    buf = _C.volume_preprocess(means, conics, s, False)
    for cs, vals in runs:
        assert all(all_nan(means, other, cs, vals)[0]), cs
        assert all(all_nan(means, buf, cs, vals)[1]), cs  # fresh: finite
    means[7, 0] += 1e-3  # changed in place after the binning
    for cs, vals in runs:
        assert all(all_nan(means, buf, cs, vals)[0]), cs


def test_operator_repeatable_and_debug(dgs):
    for case, codes in ((_lbig(3), (0, 1, OP)), (_lbig(3), (OP,)), (_lbig(1), (0, 1, OP)), (_lbig(1), (OP,))):
        a, ga, sa = _run(case, codes)
        b, gb, sb = _run(case, codes)
        d, gd, sd = _run(case, codes, debug=True)
        for x, y, z in zip(a + list(ga) + [sa], b + list(gb) + [sb], d + list(gd) + [sd]):
            assert np.isfinite(x).all()
            assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- 8. routing
def test_masks_below_32_are_the_ops_entry(dgs):
    """dgs_volume_*_linop with a mask below 32 (six-pointer arrays, coef NULL) against dgs_volume_*_ops"""
    from diff_gaussian_sampling import _C
    import dgs_ctypes
    case = _lparity(3)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    v1 = v[:, :1].contiguous()
    tdl = (np.random.default_rng(11).normal(size=(case.N, 3)) * 1e-4).astype(np.float32)
    for codes, vv, C in (([0, 1, 2], v, 3), ([T], v, 3), ([0, 1, T], v, 3), ([0, 1, 2, 3], v1, 1), ([1, T], v1, 1)):
        dls = [torch.from_numpy(np.ascontiguousarray((tdl if f == T else case.dL[f])[..., :C])).to(m.device)
               for f in codes]
        a = (dgs_ctypes.volume_forward_linop(codes, None, m, vv, c, s, buf, False)
             + list(dgs_ctypes.volume_backward_linop(codes, None, m, vv, c, s, dls, buf, False))
             + [dgs_ctypes.volume_samples_backward_linop(codes, None, m, vv, c, s, dls, buf, False)])
        b = (dgs_ctypes.volume_forward_fused(codes, m, vv, c, s, buf, False, entry="ops")
             + list(dgs_ctypes.volume_backward_fused(codes, m, vv, c, s, dls, buf, False, entry="ops"))
             + [dgs_ctypes.volume_samples_backward_fused(codes, m, vv, c, s, dls, buf, False, entry="ops")])
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.isfinite(x).all() and x.abs().max() > 0 and torch.equal(x, y), codes
        mask = sum(1 << f for f in codes)
        assert (dgs_ctypes.volume_workspace_size_linop(mask, 1000, 2000, C, 1)
                == dgs_ctypes.volume_workspace_size_ops(mask, 1000, 2000, C, 1))


def test_operator_python_routing(dgs):
    from diff_gaussian_sampling import _C
    from diff_gaussian_sampling.volume import LinearOperator, sample_volume, sample_volume_multi
    case = _lparity(3)
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    c0, b, W = lr.unpack(case.coef)
    op = LinearOperator(c0, b, W)
    assert op.coef == case.coef
    with pytest.raises(RuntimeError):
        _C.volume_forward_ops([OP], m, v, c, s, buf, False)  # the older bindings keep refusing it
    single = sample_volume(op, m, v, c, s, buf)
    assert single.shape == (case.N, 3)
    assert torch.equal(single, _C.volume_forward_linop([OP], case.coef, m, v, c, s, buf, False)[0])
    # beside the laplacian and beside the trace: the operator's own call next to the fused rest
    lap, o1, g = sample_volume_multi(("laplacian", op, "gaussian"), m, v, c, s, buf)
    trc, o2, d = sample_volume_multi(("laplacian_trace", op, "derivative"), m, v, c, s, buf)
    assert torch.equal(o1, single) and torch.equal(o2, single)
    assert torch.equal(lap, _C.volume_forward(2, m, v, c, s, buf, False))
    assert torch.equal(g, _C.volume_forward(0, m, v, c, s, buf, False))
    assert torch.equal(d, _C.volume_forward(1, m, v, c, s, buf, False))
    assert torch.equal(trc, _C.volume_forward_ops([T], m, v, c, s, buf, False)[0])
    codes = (2, OP, 0)
    dls = [torch.from_numpy(case.dL[f]).to(m.device) for f in codes]
    grads = _C.volume_backward_linop(list(codes), case.coef, m, v, c, s, dls, buf, False)
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        close(grads[k].cpu().numpy(), sum(case.bwd(f)[k] for f in codes), RTOL, ATOL, f"linop + laplacian C3 {name}")
    ds = _C.volume_samples_backward_linop(list(codes), case.coef, m, v, c, s, dls, buf, False)
    close(ds.cpu().numpy(), sum(case.sref(f) for f in codes), RTOL, ATOL, "linop + laplacian C3 dsamples")
    # two operators; a non-symmetric W; a coefficient that requires a gradient
    with pytest.raises(ValueError):
        sample_volume_multi((op, LinearOperator(1.0)), m, v, c, s, buf)
    skew = torch.tensor(W) + torch.tensor([[0.0, 1e-5, -2e-5], [-1e-5, 0.0, 3e-5], [2e-5, -3e-5, 0.0]])
    assert LinearOperator(c0, b, skew).coef == pytest.approx(case.coef, rel=1e-6, abs=1e-12)
    assert LinearOperator(W=[[0, 2, 0], [0, 0, 0], [0, 0, 0]]).coef[4:] == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert LinearOperator(W=[1, 2, 3, 4, 5, 6]).W == ((1.0, 2.0, 3.0), (2.0, 4.0, 5.0), (3.0, 5.0, 6.0))
    assert LinearOperator.laplacian((0, 1), -0.01).coef == LinearOperator.diagonal(-0.01, -0.01, 0.0).coef
    assert LinearOperator.laplacian().coef[4:] == [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    with pytest.raises(ValueError, match="sample_gaussians_multi"):
        LinearOperator(W=torch.eye(3, requires_grad=True))
    with pytest.raises(ValueError, match="sample_gaussians_multi"):
        LinearOperator(torch.tensor(1.0, requires_grad=True))


def test_operator_fallback_above_four_channels(dgs):
    """several functions with the operator at C = 5: every function on its own, gradients added"""
    if "c5" not in _lcases:
        means, values, _, conics = _field(200, 5, 9)
        _lcases["c5"] = LCase(means, values, conics, vo.samples3(300, seed=9))
    _check(_lcases["c5"], (0, 1, OP), "linop fallback C5")


# ---- 9. autograd through VolumeSampler
def test_operator_sampler_autograd(dgs):
    from diff_gaussian_sampling.volume import LinearOperator, VolumeSampler
    dev = torch.device("cuda:0")
    P, N, C = 500, 600, 3
    means, values, covs, conics = _field(P, C, 8)
    samples = vo.samples3(N, seed=8)
    case = LCase(means, values, conics, samples)
    op = LinearOperator(*lr.unpack(case.coef))
    w = {f: torch.from_numpy(case.dL[f]).to(dev).reshape(_shape(N, f, C)) for f in (0, 1, OP)}

    def leaves(smp):
        ts = [torch.from_numpy(x).to(dev) for x in (means, values, covs, conics, smp)]
        for t in (ts[0], ts[1], ts[3], ts[4]):
            t.requires_grad_(True)
        return ts

    # the single call
    m, v, cv, c, s = leaves(samples)
    vs = VolumeSampler(False, sample_grad=True)
    vs.preprocess(m, v, cv, c, s)
    out = vs.sample_gaussians_operator(op)
    assert out.shape == (N, C)
    (out * w[OP]).sum().backward()
    close(out.detach().cpu().numpy()[:, None, :], case.fwd(OP), RTOL, ATOL, "autograd linop C3 forward")
    for k, (name, t) in enumerate((("dmeans", m), ("dvalues", v), ("dconics", c))):
        close(t.grad.cpu().numpy(), case.bwd(OP)[k], RTOL, ATOL, f"autograd linop C3 {name}")
    close(s.grad.cpu().numpy(), case.sref(OP), RTOL, ATOL, "autograd linop C3 dsamples")

    # a Burgers-type residual's three functions, the derivative's output unused
    m, v, cv, c, s = leaves(samples)
    vs = VolumeSampler(False, sample_grad=True)
    vs.preprocess(m, v, cv, c, s)
    outs = dict(zip((0, 1, OP), vs.sample_gaussians_multi("gaussian", "derivative", op)))
    assert [tuple(outs[f].shape) for f in (0, 1, OP)] == [_shape(N, f, C) for f in (0, 1, OP)]
    sum((outs[f] * w[f]).sum() for f in (0, OP)).backward()
    for f in (0, 1, OP):
        close(outs[f].detach().cpu().numpy().reshape(N, _k(f), C), case.fwd(f), RTOL, ATOL, f"autograd C3 fn{f} forward")
    for k, (name, t) in enumerate((("dmeans", m), ("dvalues", v), ("dconics", c))):
        close(t.grad.cpu().numpy(), sum(case.bwd(f)[k] for f in (0, OP)), RTOL, ATOL, f"autograd C3 {name}")
    close(s.grad.cpu().numpy(), sum(case.sref(f) for f in (0, OP)), RTOL, ATOL, "autograd C3 dsamples")

    # an in-place step of the means: the sampler re-bins
    binned = vs.binning
    with torch.no_grad():
        m -= (0.005 / float(m.grad.abs().max())) * m.grad
        for t in (m, v, c, s):
            t.grad = None
    moved = m.detach().cpu().numpy()
    assert np.abs(moved - means).max() > 1e-3
    g, o = vs.sample_gaussians_multi("gaussian", op)
    assert vs.binning is not binned
    ((g * w[0]).sum() + (o * w[OP]).sum()).backward()
    after = LCase(moved, values, conics, samples)
    close(o.detach().cpu().numpy()[:, None, :], after.fwd(OP), RTOL, ATOL, "linop C3 after the step")
    close(m.grad.cpu().numpy(), sum(after.bwd(f)[0] for f in (0, OP)), RTOL, ATOL, "dmeans C3 after the step")
    close(s.grad.cpu().numpy(), sum(after.sref(f) for f in (0, OP)), RTOL, ATOL, "dsamples C3 after the step")

    # without sample_grad, samples that require a gradient raise
    m, v, cv, c, s = leaves(samples)
    vs = VolumeSampler(False)
    vs.preprocess(m, v, cv, c, s)
    with pytest.raises(NotImplementedError):
        vs.sample_gaussians_operator(op)
    with pytest.raises(NotImplementedError):
        vs.sample_gaussians_multi("gaussian", op)
