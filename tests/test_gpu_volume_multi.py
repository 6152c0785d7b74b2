"""GPU parity of the fused D = 3 functions (dgs_volume_{forward,backward}_multi, C = 1: one walk of
the candidates for several of the four functions) against the brute-force oracle
(oracle/volume.py) and against the single-function calls.

Tolerances as tests/test_gpu_volume.py: |d| <= 1e-5 |ref| + 1e-6 max|ref| for the
outputs and for the gradients of the summed loss.  Function f's upstream gradient is scaled by
0.01**f: unscaled, the third derivative's gradient is ~1e6 times the gaussian's and
atol * max|ref| would hide a missing low-order term.  With that scaling the oracle's per-function
maxima on the parity case are dmeans 54 / 65 / 195 / 85, dvalues 0.93 / 0.69 / 1.46 / 0.63 and
dconics 5.1e-4 / 3.0e-4 / 7.1e-4 / 4.4e-4 (asserted below to lie within a factor of 10); the
summed gradients' maxima are 108, 2.0 and 9.5e-4, so the bound on the sum is no looser than the
per-function bounds of tests/test_gpu_volume.py."""
import numpy as np
import pytest
import torch

from helpers import close

from oracle import volume as vo

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6  # SURVEY 8c, forward and backward
NAMES = ("gaussian", "derivative", "laplacian", "third")
MULTI_MASKS = [m for m in range(1, 16) if bin(m).count("1") >= 2]  # the 11 fused instantiations


def _codes(mask):
    return [f for f in range(4) if (mask >> f) & 1]


def _field(P, C, seed):
    return vo.gaussians3(P, C, seed=seed, scale=0.009 * max(P, 1) ** (1.0 / 3.0))


def _dLs(N, C=1):
    """per function: normal, seed 7 + f, scaled by 0.01**f"""
    return [(np.random.default_rng(7 + f).normal(size=(N, 3 ** f, C)) * 0.01 ** f).astype(np.float32)
            for f in range(4)]


def _with_big(conics):
    """the four replaced conics of test_gpu_volume.test_volume_big_gaussians"""
    conics[0] = [4.0, 0.0, 0.0, 4.0, 0.0, 4.0]  # sigma 0.5: wide
    conics[1] = [1e4, 0.0, 0.0, 1e-1, 0.0, 1e4]  # cond 1e5
    conics[2] = [30.0, 0.0, 0.0, -5.0, 0.0, 30.0]  # indefinite
    conics[3] = [2000.0, 1999.0, 0.0, 2000.0, 0.0, 50.0]  # nearly singular
    return conics


class Case:
    """Inputs plus the oracle's per-function outputs and gradients, computed once on first use."""

    def __init__(self, means, values, conics, samples):
        self.means, self.values, self.conics, self.samples = means, values, conics, samples
        self.N, self.C = samples.shape[0], values.shape[1]
        self.dL = _dLs(self.N, self.C)
        self._fwd, self._bwd = {}, {}

    def fwd(self, f):
        if f not in self._fwd:
            self._fwd[f] = vo.forward(f, self.means, self.values, self.conics, self.samples)
            self._fwd[f].setflags(write=False)
        return self._fwd[f]

    def bwd(self, f):
        if f not in self._bwd:
            self._bwd[f] = vo.backward(f, self.means, self.values, self.conics, self.samples, self.dL[f])
            for g in self._bwd[f]:
                g.setflags(write=False)
        return self._bwd[f]

    def dev(self):
        d = torch.device("cuda:0")
        return tuple(torch.from_numpy(x).to(d) for x in (self.means, self.values, self.conics, self.samples))


@pytest.fixture(scope="module")
def parity_case():
    means, values, _, conics = vo.gaussians3(1000, 1, seed=3, scale=0.009 * 1000 ** (1 / 3))
    return Case(means, values, conics, vo.samples3(2000, seed=12))


@pytest.fixture(scope="module")
def big_case():
    means, values, _, conics = _field(600, 1, 7)
    return Case(means, values, _with_big(conics), vo.samples3(1200, seed=8))


def _run(case, codes, debug=False, dL=None, backward=True):
    """fused forward (+ backward) through the extension; numpy outputs [N, 3^f, C] and gradients"""
    from diff_gaussian_sampling import _C
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, debug)
    outs = _C.volume_forward_multi(list(codes), m, v, c, s, buf, debug)
    grads = None
    if backward:
        dL = case.dL if dL is None else dL
        dls = [torch.from_numpy(dL[f]).to(m.device) for f in codes]
        grads = tuple(g.cpu().numpy() for g in _C.volume_backward_multi(list(codes), m, v, c, s, dls, buf, debug))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], grads


def _check(case, codes, debug=False):
    outs, grads = _run(case, codes, debug)
    for f, o in zip(codes, outs):
        assert o.shape == (case.N,) + (3,) * f + (case.C,)
        close(o.reshape(case.N, 3 ** f, case.C), case.fwd(f), RTOL, ATOL, f"{codes} fn{f} forward")
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        ref = sum(case.bwd(f)[k] for f in codes)
        close(grads[k], ref, RTOL, ATOL, f"{codes} {name}")


def _bitwise_vs_single(case, codes):
    from diff_gaussian_sampling import _C
    m, v, c, s = case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    outs = _C.volume_forward_multi(list(codes), m, v, c, s, buf, False)
    for f, o in zip(codes, outs):
        single = _C.volume_forward(f, m, v, c, s, buf, False)
        assert torch.equal(o, single), (codes, f, float((o - single).abs().max()))


# ---- 1. parity of every fused mask
def test_upstream_scaling_balances_the_functions(parity_case):
    """From the oracle alone: with dL_f scaled by 0.01**f no function's gradient is more than 10x
    another's, so the bound on the summed gradient sees every function."""
    for k, name in enumerate(("dmeans", "dvalues", "dconics")):
        mx = [float(np.abs(parity_case.bwd(f)[k]).max()) for f in range(4)]
        print(name, mx, float(np.abs(sum(parity_case.bwd(f)[k] for f in range(4))).max()))
        assert max(mx) <= 10.0 * min(mx), (name, mx)


@pytest.mark.parametrize("mask", MULTI_MASKS)
def test_fused_parity(dgs, parity_case, mask):
    _check(parity_case, _codes(mask))


# ---- 2. the forward is the single calls', bit for bit
@pytest.mark.parametrize("codes", [(0, 1, 2, 3), (1, 2)])
def test_fused_forward_is_bitwise_the_single_calls(dgs, parity_case, big_case, codes):
    _bitwise_vs_single(parity_case, codes)
    _bitwise_vs_single(big_case, codes)


# ---- 3. the every-sample class
@pytest.mark.parametrize("codes", [(0, 3), (0, 1, 2, 3)])
def test_fused_big_gaussians(dgs, big_case, codes):
    """wide, ill-conditioned, indefinite (power > 0 skipped) and nearly singular conics: the
    fused big-Gaussian backward writes their rows once, as the sum over the mask"""
    _check(big_case, codes)


# ---- 4. seams and images
def test_fused_seams_and_images(dgs):
    """the construction of test_gpu_volume.test_volume_seams_and_images"""
    rng = np.random.default_rng(2)
    means, values, _, conics = _field(400, 1, 2)
    means[:100, 0] = np.float32(0.999)
    means[100:200, 1] = np.float32(-0.999)
    means[200:220] = rng.uniform(2.5, 3.5, (20, 3)).astype(np.float32)  # far outside: images
    samples = vo.samples3(1500, seed=3)
    samples[:300, 0] = np.float32(-0.998)
    samples[300:400] = rng.uniform(-3.2, -2.8, (100, 3)).astype(np.float32)
    _check(Case(means, values, conics, samples), (0, 1, 2))


# ---- 5. chunk boundaries and edge sizes
def test_fused_chunk_boundaries(dgs):
    """150 Gaussians and 200 samples inside a box of side 0.004 (one grid cell: the cells here are
    about 0.2 wide) next to a sparse remainder: rows of several 64-wide chunks with a partial last
    one, in the lane = sample and the lane = Gaussian kernels."""
    rng = np.random.default_rng(21)
    means, values, _, conics = _field(250, 1, 5)
    samples = vo.samples3(330, seed=13)
    centre = np.array([0.31, -0.22, 0.47])
    means[:150] = (centre + rng.uniform(-0.002, 0.002, (150, 3))).astype(np.float32)
    samples[:200] = (centre + rng.uniform(-0.002, 0.002, (200, 3))).astype(np.float32)
    _check(Case(means, values, conics, samples), (0, 1, 2, 3))


def test_fused_edge_sizes(dgs):
    means, values, _, conics = _field(50, 1, 1)
    samples = vo.samples3(40, seed=1)
    for P, N in ((0, 40), (50, 0), (1, 1), (50, 1)):
        _check(Case(means[:P], values[:P], conics[:P], samples[:N]), (0, 1, 2, 3))


# ---- 6. order and the per-function fallback
def test_fused_order_and_fallback(dgs):
    """codes (3, 0) at C = 3: the C entry refuses several functions at C > 1, so the extension
    runs the per-function calls in turn; outputs in the order asked, gradients added"""
    means, values, _, conics = _field(300, 3, 4)
    case = Case(means, values, conics, vo.samples3(400, seed=5))
    outs, _ = _run(case, (3, 0), backward=False)
    assert outs[0].shape == (400, 3, 3, 3, 3) and outs[1].shape == (400, 3)
    _check(case, (3, 0))


def test_fused_codes_are_checked(dgs, parity_case):
    from diff_gaussian_sampling import _C
    m, v, c, s = parity_case.dev()
    buf = _C.volume_preprocess(m, c, s, False)
    for bad in ([0, 0], [4], [-1, 2], []):
        with pytest.raises(RuntimeError):
            _C.volume_forward_multi(bad, m, v, c, s, buf, False)


# ---- 7. autograd through VolumeSampler
def test_fused_sampler_autograd(dgs):
    from diff_gaussian_sampling.volume import VolumeSampler
    dev = torch.device("cuda:0")
    means, values, covs, conics = _field(500, 1, 8)
    samples = vo.samples3(600, seed=8)
    N = 600
    w = [torch.from_numpy(x).to(dev).reshape((N,) + (3,) * f + (1,)) for f, x in enumerate(_dLs(N))]

    def tensors():
        m, v, cv, c, s = (torch.from_numpy(x).to(dev) for x in (means, values, covs, conics, samples))
        for t in (m, v, c):
            t.requires_grad_(True)
        return m, v, cv, c, s

    m, v, cv, c, s = tensors()
    vs = VolumeSampler(False)
    vs.preprocess(m, v, cv, c, s)
    outs = vs.sample_gaussians_multi(*NAMES)
    assert [o.shape for o in outs] == [x.shape for x in w]
    sum((outs[f] * w[f]).sum() for f in (0, 2, 3)).backward()  # the derivative's output unused

    m2, v2, cv2, c2, s2 = tensors()
    vs2 = VolumeSampler(False)
    vs2.preprocess(m2, v2, cv2, c2, s2)
    sep = [vs2.sample_gaussians(), vs2.sample_gaussians_derivative(), vs2.sample_gaussians_laplacian(),
           vs2.sample_gaussians_third_derivative()]
    sum((sep[f] * w[f]).sum() for f in (0, 2, 3)).backward()
    for f in range(4):
        assert torch.equal(outs[f], sep[f]), f
    for name, a, b in (("dmeans", m, m2), ("dvalues", v, v2), ("dconics", c, c2)):
        close(a.grad.cpu().numpy(), b.grad.cpu().numpy(), RTOL, ATOL, "autograd " + name)
    # the unused output stayed out of the backward: the gradients are the oracle's sum over 0, 2, 3
    case = Case(means, values, conics, samples)
    for k, t in enumerate((m, v, c)):
        close(t.grad.cpu().numpy(), sum(case.bwd(f)[k] for f in (0, 2, 3)), RTOL, ATOL, f"autograd vs oracle {k}")

    with torch.no_grad():
        m.add_(torch.tensor([0.013, 0.0, 0.0], device=dev))  # moves every Gaussian: the next call re-bins
    again = vs.sample_gaussians_multi("derivative", "gaussian")
    moved = Case(m.detach().cpu().numpy(), values, conics, samples)
    close(again[0].detach().cpu().numpy().reshape(N, 3, 1), moved.fwd(1), RTOL, ATOL, "derivative after the step")
    close(again[1].detach().cpu().numpy().reshape(N, 1, 1), moved.fwd(0), RTOL, ATOL, "gaussian after the step")

    s.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        vs.sample_gaussians_multi("gaussian", "laplacian")


def test_fused_all_none_gradients(dgs):
    """every incoming gradient None: the backward returns None for every input"""
    from diff_gaussian_sampling.volume import _SampleVolumeMulti

    class Ctx:
        codes, debug, saved_tensors = (0, 1), False, (None,) * 5

    assert _SampleVolumeMulti.backward(Ctx(), None, None) == (None,) * 7


# ---- 8. loud on stale input
def test_fused_stale_buffer_is_loud(dgs):
    from diff_gaussian_sampling import _C
    dev = torch.device("cuda:0")
    means, values, _, conics = (torch.from_numpy(x).to(dev) for x in _field(100, 1, 1))
    s = torch.from_numpy(vo.samples3(200)).to(dev)
    buf = _C.volume_preprocess(means, conics, s[:100], False)  # a binning of other sizes
    codes = [0, 1, 2, 3]
    outs = _C.volume_forward_multi(codes, means, values, conics, s, buf, False)
    for o in outs:
        assert torch.isnan(o).all()
    dls = [torch.ones_like(o) for o in outs]
    for g in _C.volume_backward_multi(codes, means, values, conics, s, dls, buf, False):
        assert torch.isnan(g).all()
    # same sizes, changed means
    buf = _C.volume_preprocess(means, conics, s, False)
    m2 = means.clone()
    m2[7, 0] += 1e-3
    for o in _C.volume_forward_multi([1, 3], m2, values, conics, s, buf, False):
        assert torch.isnan(o).all()
    for g in _C.volume_backward_multi([1, 3], m2, values, conics, s, [dls[1], dls[3]], buf, False):
        assert torch.isnan(g).all()


# ---- 9. repeatable
def test_fused_repeatable_and_debug(dgs, big_case):
    codes = (0, 1, 2, 3)
    a, ga = _run(big_case, codes)
    b, gb = _run(big_case, codes)
    d, gd = _run(big_case, codes, debug=True)
    for x, y, z in zip(a + list(ga), b + list(gb), d + list(gd)):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)


# ---- 10. locality of a non-finite upstream gradient
def test_fused_nonfinite_dl_stays_local(dgs, parity_case):
    """One sample's laplacian dL = inf in mask 15: every Gaussian whose float32 power against that
    sample is below -110 (5 beyond -105, the exact-zero point the binning relies on) keeps the
    gradient rows of the run with that dL = 0."""
    case, j = parity_case, 1234
    X = vo._pairs(case.means, case.conics, case.samples[j:j + 1])[0][:, 0, :].astype(np.float32)
    c = case.conics.astype(np.float32)
    qd = c[:, 0] * X[:, 0] * X[:, 0] + c[:, 3] * X[:, 1] * X[:, 1] + c[:, 5] * X[:, 2] * X[:, 2]
    qo = c[:, 1] * X[:, 0] * X[:, 1] + c[:, 2] * X[:, 0] * X[:, 2] + c[:, 4] * X[:, 1] * X[:, 2]
    power = np.float32(-0.5) * qd - qo  # oracle/volume.py _pairs, float32 in that order
    far = power < np.float32(-110.0)
    assert 0 < far.sum() < far.size, far.sum()
    zero = [x.copy() for x in case.dL]
    zero[2][j] = 0.0
    inf = [x.copy() for x in case.dL]
    inf[2][j] = np.inf
    _, g0 = _run(case, (0, 1, 2, 3), dL=zero)
    _, g1 = _run(case, (0, 1, 2, 3), dL=inf)
    for a, b in zip(g0, g1):
        assert np.isfinite(a).all()
        assert np.array_equal(a[far], b[far])
    assert not np.isfinite(g1[0][~far]).all()  # (the sample's live pairs do carry it)
