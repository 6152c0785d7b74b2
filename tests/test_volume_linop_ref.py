"""The linear operator's reference (tests/volume_linop_ref.py), on the CPU.

1. The lift is the adjoint of the combination: <lift(dL), outs> = <dL, L outs> in float64, for
   random outputs; the packed order and the doubled off-diagonals go through both sides.
2. The reference gradients against torch float64 autograd of the combined
   `volume_sample_grad_ref.torch_forward` (tolerances of tests/test_volume_trace_ref.py).
3. The margin check: for every coefficient set and field the GPU tests compare on
   (tests/test_gpu_volume_linop.py: the parity field and the big-Gaussian field at C = 1 and 3), the
   reference's own float32 serial order of the forward lies within 0.9 of the SURVEY 8c bound,
   |d| <= 1e-5 |ref| + 1e-6 max|ref|.  That is what lets the GPU comparison mean something: a field
   on which float32 itself takes the whole bound would test the field, not the kernels.  The same
   share of the sample gradient (the one gradient with a float32 order in the references) is
   computed and asserted here too: it is at most 0.46, so the GPU test leaves no comparison out.
   Measured: forward 0.03 .. 0.07 on the parity field, 0.14 .. 0.51 on the big-Gaussian field;
   sample gradient 0.06 .. 0.11 and 0.04 .. 0.46.  With DGS_MARGINS set the shares are recorded
   (profiles/volume_linop_margins.json).
"""
import numpy as np
import pytest
import torch

import volume_linop_ref as lr
import volume_sample_grad_ref as vr
from helpers import margin_of, record_margin
from oracle import volume as vo
from test_gpu_volume_multi import _field, _with_big
from test_gpu_volume_multi_c import _parity

RTOL, ATOL = 1e-5, 1e-6


@pytest.mark.parametrize("name", list(lr.SETS) + ["random"])
def test_lift_is_the_adjoint_of_the_combination(name):
    rng = np.random.default_rng(1)
    coef = lr.SETS[name] if name != "random" else rng.normal(size=10)
    N, C = 7, 3
    outs = {f: rng.normal(size=(N, 3 ** f, C)) for f in range(3)}
    for f in (1, 2):  # (nothing here relies on the outputs' symmetry)
        assert outs[f].shape[1] == 3 ** f
    dL = rng.normal(size=(N, C))
    up = lr.lift(coef, dL)
    lhs = sum(float((up[f] * outs[f]).sum()) for f in lr.parts(coef))
    rhs = float((dL * lr.combine(coef, outs)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)


def test_packed_order_and_off_diagonals():
    """one-hot coefficients: c0 the gaussian, b_i component i, a diagonal w the full component (i, i),
    an off-diagonal w the sum of the two full components (i, j) and (j, i)"""
    rng = np.random.default_rng(2)
    outs = {f: rng.normal(size=(5, 3 ** f, 2)) for f in range(3)}
    want = [outs[0][:, 0], outs[1][:, 0], outs[1][:, 1], outs[1][:, 2], outs[2][:, 0], outs[2][:, 1] + outs[2][:, 3],
            outs[2][:, 2] + outs[2][:, 6], outs[2][:, 4], outs[2][:, 5] + outs[2][:, 7], outs[2][:, 8]]
    for q in range(10):
        coef = np.zeros(10)
        coef[q] = 1.0
        np.testing.assert_allclose(lr.combine(coef, outs), want[q], rtol=0, atol=1e-15)


@pytest.mark.parametrize("C", [1, 2])
def test_reference_gradients_match_autograd(C):
    P, N = 40, 60
    coef = lr.SETS["balanced"]
    means, values, _, conics = vo.gaussians3(P, C, seed=4 + C, scale=3.0)
    samples = vo.samples3(N, seed=20 + C)
    samples[0] = means[0]  # an exact hit
    dL = np.random.default_rng(3).normal(size=(N, C))
    m, v, c, s = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (means, values, conics, samples))
    c0, b, W = lr.unpack(coef)
    out = (c0 * vr.torch_forward(0, m, v, c, s)[:, 0]
           + torch.einsum("i,nic->nc", torch.tensor(b), vr.torch_forward(1, m, v, c, s))
           + torch.einsum("f,nfc->nc", torch.tensor(W.reshape(9)), vr.torch_forward(2, m, v, c, s)))
    ref = lr.forward(coef, means, values, conics, samples)
    assert ref.shape == (N, C) and np.abs(ref).max() > 0
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    (out * torch.tensor(dL)).sum().backward()
    dm, dv, dc = lr.backward(coef, means, values, conics, samples, dL)
    ds = lr.dsamples(coef, means, values, conics, samples, dL)
    for name, got, want in (("means", dm, m.grad), ("values", dv, v.grad), ("conics", dc, c.grad),
                            ("samples", ds, s.grad)):
        want = want.numpy()
        assert np.abs(want).max() > 0, name
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max(), err_msg=name)


def fields(C):
    """the two fields of the GPU comparisons: (name, means, values, conics, samples)"""
    p = _parity(C)
    means, values, _, conics = _field(600, C, 7)
    return (("parity", p.means, p.values, p.conics, p.samples),
            ("big", means, values, _with_big(conics), vo.samples3(1200, seed=8)))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", list(lr.SETS))
def test_float32_order_leaves_room_under_the_bound(name, C):
    coef = lr.SETS[name]
    for field, means, values, conics, samples in fields(C):
        ref = lr.forward(coef, means, values, conics, samples)
        share = margin_of(lr.forward(coef, means, values, conics, samples, np.float32), ref, RTOL, ATOL)
        record_margin(f"linop {name} {field} C{C} forward [float32 serial order vs float64]", share, RTOL, ATOL,
                      int(ref.size))
        print(name, field, C, "forward", share)
        assert share <= 0.9, (name, field, C, share)
        dL = lr.op_dL(samples.shape[0], C)
        sref = lr.dsamples(coef, means, values, conics, samples, dL)
        sshare = margin_of(lr.dsamples(coef, means, values, conics, samples, dL, np.float32), sref, RTOL, ATOL)
        record_margin(f"linop {name} {field} C{C} dsamples [float32 serial order vs float64]", sshare, RTOL, ATOL,
                      int(sref.size))
        print(name, field, C, "dsamples", sshare)
        assert sshare <= 0.9, (name, field, C, sshare)
