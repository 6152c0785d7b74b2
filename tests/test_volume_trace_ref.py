"""The trace reference (tests/volume_trace_ref.py) against torch float64 autograd of
`volume_sample_grad_ref.torch_forward(2, ...)` contracted over the diagonal: the gradients of
means, values, conics and samples.  Tolerance: tests/test_volume_oracle.py's for the same kind of
check (rtol 1e-5, atol 1e-5 max|want| for the gradients; rtol 1e-5, atol 1e-6 max for the forward)."""
import numpy as np
import pytest
import torch

import volume_sample_grad_ref as vr
import volume_trace_ref as tr
from oracle import volume as vo


@pytest.mark.parametrize("C", [1, 2])
def test_trace_reference_gradients_match_autograd(C):
    P, N = 40, 60
    means, values, _, conics = vo.gaussians3(P, C, seed=4 + C, scale=3.0)
    samples = vo.samples3(N, seed=20 + C)
    samples[0] = means[0]  # an exact hit
    samples[1] = means[1] + np.float32(1.95)  # across the seam (wrapped)
    samples[1] = np.where(samples[1] > 1, samples[1] - np.float32(4.0), samples[1])
    dL = np.random.default_rng(3).normal(size=(N, C))
    m, v, c, s = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (means, values, conics, samples))
    out = vr.torch_forward(2, m, v, c, s)[:, tr.DIAG, :].sum(1)
    ref = tr.forward(means, values, conics, samples)
    assert ref.shape == (N, C) and np.abs(ref).max() > 0
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    (out * torch.tensor(dL)).sum().backward()
    dm, dv, dc = tr.backward(means, values, conics, samples, dL)
    ds = tr.dsamples(means, values, conics, samples, dL)
    for name, got, want in (("means", dm, m.grad), ("values", dv, v.grad), ("conics", dc, c.grad),
                            ("samples", ds, s.grad)):
        want = want.numpy()
        assert np.abs(want).max() > 0, name
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max(), err_msg=name)


def test_trace_reference_float32_order_is_close():
    """the float32 serial order of the forward and of the sample gradient: the same sums"""
    means, values, _, conics = vo.gaussians3(40, 2, seed=1, scale=3.0)
    samples = vo.samples3(60, seed=2)
    dL = np.random.default_rng(5).normal(size=(60, 2)).astype(np.float32)
    for f64, f32 in ((tr.forward(means, values, conics, samples), tr.forward(means, values, conics, samples, np.float32)),
                     (tr.dsamples(means, values, conics, samples, dL),
                      tr.dsamples(means, values, conics, samples, dL, np.float32))):
        assert f32.dtype == np.float32 and f32.shape == f64.shape
        np.testing.assert_allclose(f32, f64, rtol=1e-4, atol=1e-5 * np.abs(f64).max())


def test_lift_places_the_gradient_on_the_diagonal():
    dL = np.arange(6, dtype=np.float32).reshape(3, 2) + 1
    up = tr.lift(dL)
    assert up.shape == (3, 9, 2)
    for f in range(9):
        assert np.array_equal(up[:, f, :], dL if f in (0, 4, 8) else np.zeros_like(dL))
