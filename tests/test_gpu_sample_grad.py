"""GPU parity of the gradient with respect to the sample positions (dgs_sample_backward_samples,
DESIGN.md section 4.9) against the float64 reference of tests/sample_grad_ref.py, which
tests/test_sample_grad_ref.py pins to the oracle on the CPU for every case used here.

Bound: the project's 8c bound, |gpu - ref| <= 1e-5 |ref| + 1e-6 max|ref|.  The thin case states
8c + B, B the a-priori exponent-order bound of DESIGN.md section 6 evaluated for this output
by the helper (from the inputs alone).  Every case also records the distance of the helper's
own float32 serial-order gradient from the float64 one (helpers.record_margin).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_grad_ref as sgr
from diff_gaussian_sampling import synthetic as syn
from helpers import close, margin_of, record_margin

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def _bin(dgs, inputs):
    m, v, cv, c, s = (t.to(DEV) for t in inputs)
    R, gb, sb, rg, srg, _ = dgs._C.preprocess_gaussians(m, v, cv, c, s, False)
    return (m, v, c, s), (R, gb, sb, rg, srg)


def _gpu(dgs, name):
    functions, inputs, dLs, ob, ref = sgr.case(name)
    (m, v, c, s), (R, gb, sb, _, _) = _bin(dgs, inputs)
    assert R == ob.num_rendered
    got = dgs._C.sample_gaussians_samples_backward([sgr.FUNCS[f] for f in functions], m, v, c, s,
                                                   [d.to(DEV) for d in dLs], gb, sb, False)
    assert got.shape == (inputs[4].shape[0], inputs[0].shape[1])
    return got.cpu().numpy(), ref


def _check(name, got, ref, extra=None):
    record_margin(f"{name} dsamples [reference float32 serial order vs float64]",
                  margin_of(ref["serial32"], ref["dsamples"], RTOL, ATOL, extra), RTOL, ATOL, int(got.size))
    close(got, ref["dsamples"], RTOL, ATOL, f"{name} dL/dsamples", extra)


PLAIN = [n for n in sgr.CASE_NAMES if n not in ("thin", "aliasing", "duplicates", "d1_c3_multi")]


@pytest.mark.parametrize("name", PLAIN)
def test_sample_grad_matches_reference(dgs, oracle, name):
    """The four functions at D = 2, C = 1; the fused masks; C in {3, 5, 16}; D = 1; edge_case
    (seam wraps, a non-PD conic, a full-range Gaussian); far means; D = 1 zero variance."""
    got, ref = _gpu(dgs, name)
    _check(name, got, ref)


def test_aliasing_outside_samples_get_zero(dgs, oracle):
    got, ref = _gpu(dgs, "aliasing")
    _check("aliasing", got, ref)
    ob = sgr.case("aliasing")[3]
    keys = ob.sample_keys()
    outside = (keys < 0) | (keys >= ob.T)
    assert outside.any(), "the case must hold a sample outside every tile"
    assert not np.any(got[outside])


def test_duplicated_samples_get_identical_gradients(dgs, oracle):
    got, ref = _gpu(dgs, "duplicates")
    _check("duplicates", got, ref)
    assert np.array_equal(got[:500], got[500:])


def test_thin_gaussians(dgs, oracle):
    """cases.thin_case at 8c + the helper's a-priori exponent-order bound."""
    got, ref = _gpu(dgs, "thin")
    _check("thin", got, ref, extra=ref["bound"])


@pytest.mark.parametrize("name", ["multi_gl", "multi_all"])
def test_fused_mask_is_the_sum_and_deterministic(dgs, oracle, name):
    functions, inputs, dLs, ob, ref = sgr.case(name)
    (m, v, c, s), (R, gb, sb, _, _) = _bin(dgs, inputs)
    codes = [sgr.FUNCS[f] for f in functions]
    dl = [d.to(DEV) for d in dLs]
    call = dgs._C.sample_gaussians_samples_backward
    fused = call(codes, m, v, c, s, dl, gb, sb, False)
    again = call(codes, m, v, c, s, dl, gb, sb, False)
    assert torch.equal(fused, again)
    parts = [call([k], m, v, c, s, [d], gb, sb, False).double() for k, d in zip(codes, dl)]
    # each part is within its own 8c bound of its float64 value, the fused call within the sum's
    bound = sum(RTOL * p.abs() + ATOL * float(p.abs().max()) for p in parts)
    bound = bound + RTOL * fused.abs().double() + ATOL * float(fused.abs().max())
    assert bool(((fused.double() - sum(parts)).abs() <= bound).all())


def test_empty_inputs(dgs):
    C = dgs._C
    m, v, cv = torch.zeros(0, 2, device=DEV), torch.zeros(0, 1, device=DEV), torch.zeros(0, 3, device=DEV)
    s = torch.rand(10, 2, device=DEV)
    R, gb, sb, rg, srg, _ = C.preprocess_gaussians(m, v, cv, cv, s, False)
    g = C.sample_gaussians_samples_backward([1], m, v, cv, s, [torch.ones(10, 2, 1, device=DEV)], gb, sb, False)
    assert g.shape == (10, 2) and float(g.abs().sum()) == 0.0
    means, values, covs, conics = (t.to(DEV) for t in syn.gaussians(5, 2, 1))
    s0 = torch.zeros(0, 2, device=DEV)
    R, gb, sb, rg, srg, _ = C.preprocess_gaussians(means, values, covs, conics, s0, False)
    g = C.sample_gaussians_samples_backward([0], means, values, conics, s0, [torch.zeros(0, 1, device=DEV)], gb, sb,
                                            False)
    assert g.shape == (0, 2)


BWD_NAME = {"gaussian": "sample_gaussians_backward", "derivative": "sample_gaussians_derivative_backward",
            "laplacian": "sample_gaussians_laplacian_backward", "third": "sample_gaussians_third_derivative_backward"}
FWD_METHOD = {"gaussian": "sample_gaussians", "derivative": "sample_gaussians_derivative",
              "laplacian": "sample_gaussians_laplacian", "third": "sample_gaussians_third_derivative"}


def _same(x, y):
    if isinstance(x, torch.Tensor):
        return isinstance(y, torch.Tensor) and x.shape == y.shape and torch.equal(x, y)
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    return x == y


@pytest.mark.parametrize("name", ["d2_c1_laplacian", "d2_c3_derivative", "d1_c1_third", "multi_all"])
def test_autograd_through_the_package(dgs, oracle, name, monkeypatch):
    """GaussianSampler with samples.requires_grad_(True): samples.grad matches the reference.
    (Before this feature samples.grad stayed None: this is the test that shows it.)

    The means / values / conics gradients must be those of the run without it.  The backward that
    computes them adds with float atomics in no fixed order (tests/test_gpu_graph.py), so two runs
    of the unchanged code may already differ in the last bits; what is bitwise here is everything
    that decides them: the existing _C backward is called once, with bitwise the same arguments,
    and .grad is bitwise the tensor that call returned.  The two runs' values are compared at the
    8c bound on top."""
    functions, inputs, dLs, ob, ref = sgr.case(name)
    bwd = "sample_gaussians_multi_backward" if len(functions) > 1 else BWD_NAME[functions[0]]
    real = getattr(dgs._C, bwd)
    calls = []

    def spy(*a):
        r = real(*a)
        calls.append((a, r))
        return r

    monkeypatch.setattr(dgs._C, bwd, spy)
    grads = {}
    for want in (False, True):
        m, v, cv, c, s = (t.to(DEV) for t in inputs)
        for t in (m, v, c):
            t.requires_grad_(True)
        s.requires_grad_(want)
        sampler = dgs.GaussianSampler(False)
        sampler.preprocess(m, v, cv, c, s)
        if len(functions) > 1:
            outs = sampler.sample_gaussians_multi(*functions)
        else:
            outs = [getattr(sampler, FWD_METHOD[functions[0]])()]
        sum((o * d.to(DEV).reshape(o.shape)).sum() for o, d in zip(outs, dLs)).backward()
        grads[want] = (m.grad, v.grad, c.grad, s.grad)
    assert grads[False][3] is None
    assert grads[True][3] is not None, "samples.grad is None"
    _check(name + " autograd", grads[True][3].cpu().numpy(), ref)
    assert len(calls) == 2
    (args0, ret0), (args1, ret1) = calls
    # (binning buffers differ in address only; their bytes are compared like every tensor)
    assert _same([a for a in args0 if not isinstance(a, torch.Tensor) or a.dtype != torch.uint8],
                 [a for a in args1 if not isinstance(a, torch.Tensor) or a.dtype != torch.uint8])
    for k, w in enumerate(("means", "values", "conics")):
        assert torch.equal(grads[True][k], ret1[k]) and torch.equal(grads[False][k], ret0[k])
        close(grads[True][k].cpu().numpy(), grads[False][k].cpu().numpy(), RTOL, ATOL,
              f"{name} d{w} with / without samples.grad")


def test_backward_calls_unchanged_without_sample_grad(dgs, monkeypatch):
    """With samples that do not require grad the new _C function is not called at all; with it,
    the existing backward binding still gets exactly its former arguments."""
    calls = []
    real = dgs._C.sample_gaussians_samples_backward
    monkeypatch.setattr(dgs._C, "sample_gaussians_samples_backward", lambda *a: (calls.append(a), real(*a))[1])
    m, v, cv, c = (t.to(DEV) for t in syn.gaussians(200, 2, 1, seed=3))
    s = syn.samples(500, 2, seed=4).to(DEV)
    m.requires_grad_(True)
    sampler = dgs.GaussianSampler(False)
    sampler.preprocess(m, v, cv, c, s)
    sampler.sample_gaussians().sum().backward()
    assert not calls and s.grad is None
    s.requires_grad_(True)
    sampler.sample_gaussians_derivative().sum().backward()
    assert len(calls) == 1 and s.grad is not None and s.grad.shape == s.shape


def test_translation_invariance_against_the_backward(dgs, oracle):
    """sum_n dL/ds_n = -sum_g dL/dm_g: the new kernel against the existing k_backward."""
    functions, inputs, dLs, ob, ref = sgr.case("d2_c1_third")
    (m, v, c, s), (R, gb, sb, rg, srg) = _bin(dgs, inputs)
    dl = dLs[0].to(DEV).reshape(-1, 2, 2, 2, 1)
    ds = dgs._C.sample_gaussians_samples_backward([3], m, v, c, s, [dl], gb, sb, False).double()
    dm = dgs._C.sample_gaussians_third_derivative_backward(m, v, c, s, R, dl, gb, sb, rg, srg, False)[0].double()
    bound = ((RTOL * ds.abs() + ATOL * float(ds.abs().max())).sum(0)
             + (RTOL * dm.abs() + ATOL * float(dm.abs().max())).sum(0))
    assert bool(((ds.sum(0) + dm.sum(0)).abs() <= bound).all()), (ds.sum(0), dm.sum(0), bound)


def test_non_finite_dl_stays_in_its_sample(dgs, oracle):
    functions, inputs, dLs, ob, ref = sgr.case("multi_all")
    (m, v, c, s), (R, gb, sb, _, _) = _bin(dgs, inputs)
    codes = [sgr.FUNCS[f] for f in functions]
    j = 1234
    runs = []
    for bad in (0.0, float("inf")):
        dl = [d.clone().to(DEV) for d in dLs]
        dl[1][j] = bad
        runs.append(dgs._C.sample_gaussians_samples_backward(codes, m, v, c, s, dl, gb, sb, False))
    keep = torch.ones(len(runs[0]), dtype=torch.bool, device=DEV)
    keep[j] = False
    assert bool(torch.isfinite(runs[1][keep]).all())
    assert torch.equal(runs[0][keep], runs[1][keep])


@pytest.mark.parametrize("name", ["d2_c1_derivative", "d2_c3_derivative", "d1_c1_third", "multi_gl"])
def test_stale_binning_takes_the_call_time_path(dgs, oracle, name):
    """means changed in place after the binning: the oracle's pair set with the new means."""
    functions, inputs, dLs, ob, _ = sgr.case(name)
    (m, v, c, s), (R, gb, sb, _, _) = _bin(dgs, inputs)
    P, D = inputs[0].shape
    step = (torch.randn(P, D, generator=torch.Generator().manual_seed(7)) * (0.5 * 2.0 / P ** (1.0 / D))).float()
    m.add_(step.to(DEV))
    assert not dgs._C.inputs_match(m, c, s, gb, sb)
    got = dgs._C.sample_gaussians_samples_backward([sgr.FUNCS[f] for f in functions], m, v, c, s,
                                                   [d.to(DEV) for d in dLs], gb, sb, False)
    ref = sgr.sample_grad_ref(ob, functions, m.cpu().numpy(), inputs[1].numpy(), inputs[3].numpy(),
                              inputs[4].numpy(), [d.numpy() for d in dLs])
    _check(name + " (stale means)", got.cpu().numpy(), ref)


def test_graph_capture_replay_is_bitwise(dgs):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "sample_grad_graph_child.py")],
                       capture_output=True, text=True, timeout=240)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"rc {r.returncode}: {tail}"


def test_c_abi_matches_extension(dgs):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import dgs_ctypes
    functions, inputs, dLs, ob, _ = sgr.case("multi_gl")
    (m, v, c, s), (R, gb, sb, _, _) = _bin(dgs, inputs)
    dl = [d.to(DEV) for d in dLs]
    a = dgs._C.sample_gaussians_samples_backward([0, 2], m, v, c, s, dl, gb, sb, False)
    b = dgs_ctypes.sample_gaussians_samples_backward([0, 2], m, v, c, s, dl, gb, sb, False)
    assert torch.equal(a, b)
    lib = ctypes.CDLL(os.path.join(os.path.dirname(dgs.__file__), "libdgs.so"))
    assert lib.dgs_version() == 12


def test_fused_mask_outside_d2_c1(dgs, oracle):
    """Several functions at D = 1: the extension runs the per-function calls in turn and adds them;
    the C entry point itself refuses a multi-bit mask there (DGS_ERR_ARG)."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import dgs_ctypes
    functions, inputs, dLs, ob, ref = sgr.case("d1_c3_multi")
    (m, v, c, s), (R, gb, sb, _, _) = _bin(dgs, inputs)
    got = dgs._C.sample_gaussians_samples_backward([0, 3], m, v, c, s, [d.to(DEV) for d in dLs], gb, sb, False)
    _check("d1_c3 gaussian + third", got.cpu().numpy(), ref)
    with pytest.raises(RuntimeError, match="D = 2, C = 1"):
        dgs_ctypes.sample_gaussians_samples_backward([0, 3], m, v, c, s, [d.to(DEV) for d in dLs], gb, sb, False)


def test_out_of_scope_samplers_raise(dgs):
    """VolumeSampler (D = 3) returns no sample gradient: a clear error instead of a silent None."""
    from diff_gaussian_sampling.volume import VolumeSampler
    from oracle import volume as vo
    m3, v3, cv3, c3 = (torch.from_numpy(x).to(DEV) for x in vo.gaussians3(50, 1, seed=1, scale=0.05))
    s3 = torch.from_numpy(vo.samples3(80, seed=2)).to(DEV)
    vs = VolumeSampler(False)
    vs.preprocess(m3, v3, cv3, c3, s3)
    assert vs.sample_gaussians().shape[0] == 80  # unchanged without a gradient request
    s3.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="samples"):
        vs.sample_gaussians()
