"""CPU checks of the D = 3 sample-gradient reference (tests/volume_sample_grad_ref.py), on the field
of tests/test_volume_oracle.py: its closed form against torch float64 autograd with respect to the
samples of a torch restatement of the forward, and the translation identity
sum_n dL/ds_n = -sum_p dL/dm_p against oracle.volume.backward."""
import numpy as np
import pytest
import torch

import volume_sample_grad_ref as vr
from oracle import volume as vo


def _field(function, C):
    means, values, _, conics = vo.gaussians3(6, C, seed=function, scale=6.0)
    samples = vo.samples3(9, seed=10 + function)
    samples[0] = means[0]  # an exact hit
    samples[1] = means[1] + np.float32(1.95)  # across the seam (wrapped)
    samples[1] = np.where(samples[1] > 1, samples[1] - np.float32(4.0), samples[1])
    dL = np.random.default_rng(3).normal(size=(samples.shape[0], 3 ** function, C))
    return means, values, conics, samples, dL


@pytest.mark.parametrize("function", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [1, 2])
def test_closed_form_matches_autograd(function, C):
    """rtol 1e-5, atol 1e-5 max|ref| (test_volume_oracle.py's bound for the other gradients): what
    is left is the float32 power inside oracle.volume._pairs."""
    means, values, conics, samples, dL = _field(function, C)
    m, v, c = (torch.tensor(x.astype(np.float64)) for x in (means, values, conics))
    s = torch.tensor(samples.astype(np.float64), requires_grad=True)
    out = vr.torch_forward(function, m, v, c, s)
    ref = vo.forward(function, means, values, conics, samples)
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    (out * torch.tensor(dL)).sum().backward()
    want = s.grad.numpy()
    got = vr.dsamples(function, means, values, conics, samples, dL)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


@pytest.mark.parametrize("function", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [1, 2])
def test_translation_identity(function, C):
    """Moving every sample by d is moving every mean by -d: the sums agree to 1e-10 max|dm|."""
    means, values, conics, samples, dL = _field(function, C)
    ds = vr.dsamples(function, means, values, conics, samples, dL)
    dm, _, _ = vo.backward(function, means, values, conics, samples, dL)
    assert np.abs(ds.sum(0) + dm.sum(0)).max() <= 1e-10 * np.abs(dm).max()


@pytest.mark.parametrize("function", [0, 3])
def test_float32_serial_variant_is_close(function):
    """The float32 serial-order variant is the same sum: within the 8c bound of the float64 form on
    this small field (it is the measure of float32's own cost on the GPU tests' fields)."""
    means, values, conics, samples, dL = _field(function, 2)
    ref = vr.dsamples(function, means, values, conics, samples, dL)
    got = vr.dsamples(function, means, values, conics, samples, dL, dtype=np.float32)
    assert got.dtype == np.float32
    assert (np.abs(got - ref) <= vr.bound8c(ref)).all()


def test_multi_is_the_sum_and_edge_sizes():
    means, values, conics, samples, _ = _field(2, 1)
    dLs = [np.random.default_rng(f).normal(size=(9, 3 ** f, 1)) for f in (0, 2)]
    both = vr.dsamples_multi((0, 2), means, values, conics, samples, dLs)
    assert np.array_equal(both, vr.dsamples(0, means, values, conics, samples, dLs[0])
                          + vr.dsamples(2, means, values, conics, samples, dLs[1]))
    assert vr.dsamples(1, means[:0], values[:0], conics[:0], samples, np.zeros((9, 3, 1))).tolist() == [[0.0] * 3] * 9
    assert vr.dsamples(1, means, values, conics, samples[:0], np.zeros((0, 3, 1))).shape == (0, 3)
