"""Reference of the constant-coefficient linear operator of a D = 3 field (function 5; not a test).

    L u = c0 u + sum_i b_i d_i u + sum_ij W_ij d_ij u,
    coef = [c0, b0, b1, b2, w00, w01, w02, w11, w12, w22]  (w the packed entries of the symmetric W)

The operator is by definition that combination of the gaussian, the derivative and the laplacian,
so the brute-force oracle (oracle/volume.py) and the sample gradient reference
(tests/volume_sample_grad_ref.py) need no operator of their own:

    forward    combine(coef, fwd(0), fwd(1), fwd(2)) = c0 fwd(0) + b . fwd(1) + W : fwd(2)
    gradients  the sum of oracle.volume.backward(f, ..., lift(coef, dL)[f]) over f = 0, 1, 2 with the
               operator's upstream gradient lifted: dL c0, dL (x) b, dL (x) W
    dsamples   the sum of volume_sample_grad_ref.dsamples(f, ..., lift(coef, dL)[f])

A function whose coefficients are all zero is left out (it adds exactly nothing).

dtype=np.float32: one float32 order of the same sums: the per-pair factor t in float32 in the order
include/dgs_volume.h states, float32 terms added serially over the Gaussians in index order.  It is
the measure of what float32 itself costs against the bound, as `volume_trace_ref` offers it.
"""
import numpy as np

import volume_sample_grad_ref as vr
from oracle import volume as vo

# the coefficient sets the GPU tests compare on (the issue's table): name -> coef[10]
SETS = {
    "balanced": [0.7, 0.011, -0.006, 0.009, 1.1e-4, -0.4e-4, 0.3e-4, 0.8e-4, 0.5e-4, -0.9e-4],
    "lap_xy": [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0],
    "heat": [0.0, 0.0, 0.0, 1.0, -0.01, 0.0, 0.0, -0.01, 0.0, 0.0],
    "wave": [0.0, 0.0, 0.0, 0.0, -0.5, 0.0, 0.0, -0.5, 0.0, 1.0],
}


def op_dL(N, C):
    """the operator's upstream gradient in the tests: normal, seed 12, unscaled (the sets carry their
    own scale: `balanced` weighs u, grad u and the Hessian as 0.01**f weighs their upstream gradients)"""
    return np.random.default_rng(12).normal(size=(N, C)).astype(np.float32)


def unpack(coef):
    """(c0, b [3], W [3, 3]) in float64 from the ten coefficients rounded to float32"""
    k = np.asarray(coef, np.float32).astype(np.float64)
    assert k.shape == (10,)
    W = np.zeros((3, 3))
    for u, (i, j) in enumerate(vo.PAIRS):
        W[i, j] = W[j, i] = k[4 + u]
    return k[0], k[1:4].copy(), W


def parts(coef):
    """the functions (0, 1, 2) with a non-zero coefficient"""
    c0, b, W = unpack(coef)
    return [f for f, on in ((0, c0 != 0), (1, b.any()), (2, W.any())) if on]


def combine(coef, outs):
    """L of the outputs {f: [N, 3^f, C]} of functions 0, 1, 2 (those of parts(coef) suffice): [N, C]"""
    c0, b, W = unpack(coef)
    w = {0: np.array([c0]), 1: b, 2: W.reshape(9)}
    return sum(np.einsum("f,nfc->nc", w[f], np.asarray(outs[f], np.float64)) for f in parts(coef))


def lift(coef, dL):
    """the operator's upstream gradient [N, C] as those of functions 0, 1, 2: {f: [N, 3^f, C]}"""
    c0, b, W = unpack(coef)
    dL = np.asarray(dL, np.float64)
    return {0: dL[:, None, :] * c0, 1: dL[:, None, :] * b[None, :, None], 2: dL[:, None, :] * W.reshape(9)[None, :, None]}


def _t32(k, a, A):
    """the per-pair factor in float32, the order of include/dgs_volume.h; a [P, n, 3], A [P, 3, 3]"""
    f = np.float32
    k = np.asarray(k, f)
    m = [f(1), f(2), f(2), f(1), f(2), f(1)]
    lin = k[1] * a[..., 0] + k[2] * a[..., 1] + k[3] * a[..., 2]
    q = None
    for u, (i, j) in enumerate(vo.PAIRS):
        term = (m[u] * k[4 + u]) * (a[..., i] * a[..., j] - A[:, i, j][:, None])
        q = term if q is None else q + term
    t = (k[0] + lin) + q
    assert t.dtype == f
    return t


def forward(coef, means, values, conics, samples, dtype=np.float64, chunk=512):
    """out [N, C]; float64: the oracle's outputs combined.  float32: v G t, serially over the Gaussians."""
    P, N, C = means.shape[0], samples.shape[0], values.shape[1]
    if dtype == np.float64:
        if P == 0 or N == 0 or not parts(coef):
            return np.zeros((N, C))
        return combine(coef, {f: vo.forward(f, means, values, conics, samples) for f in parts(coef)})
    out = np.zeros((N, C), np.float32)
    if P == 0 or N == 0:
        return out
    A = vo._amat(conics.astype(np.float64)).astype(np.float32)
    v = values.astype(np.float32)
    for s0 in range(0, N, chunk):
        X, G, _ = vo._pairs(means, conics, samples[s0:s0 + chunk])
        X, G = X.astype(np.float32), G.astype(np.float32)
        a = np.einsum("pij,pnj->pni", A, X)
        term = (G * _t32(coef, a, A))[:, :, None] * v[:, None, :]  # [P, n, C]
        out[s0:s0 + chunk] = np.cumsum(term.astype(np.float32), axis=0, dtype=np.float32)[-1]
    return out


def backward(coef, means, values, conics, samples, dL):
    """(dmeans [P, 3], dvalues [P, C], dconics [P, 6]) of sum(dL * L u), float64"""
    P, C = means.shape[0], values.shape[1]
    up = lift(coef, dL)
    res = [np.zeros((P, 3)), np.zeros((P, C)), np.zeros((P, 6))]
    for f in parts(coef):
        res = [r + g for r, g in zip(res, vo.backward(f, means, values, conics, samples, up[f]))]
    return tuple(res)


def dsamples(coef, means, values, conics, samples, dL, dtype=np.float64, chunk=512):
    """dL/d samples [N, 3] of sum(dL * L u).  float32: phi = hv t and g = hv (b + 2 W a) in float32,
    the pairs' G (phi a - A g) added serially over the Gaussians."""
    P, N = means.shape[0], samples.shape[0]
    if dtype == np.float64:
        up = lift(coef, dL)
        out = np.zeros((N, 3))
        for f in parts(coef):
            out = out + vr.dsamples(f, means, values, conics, samples, up[f])
        return out
    out = np.zeros((N, 3), np.float32)
    if P == 0 or N == 0:
        return out
    f32 = np.float32
    c0, b, W = unpack(coef)
    b, W2 = b.astype(f32), (2.0 * W).astype(f32)
    A = vo._amat(conics.astype(np.float64)).astype(f32)
    v, h = values.astype(f32), np.asarray(dL, f32)
    for s0 in range(0, N, chunk):
        X, G, _ = vo._pairs(means, conics, samples[s0:s0 + chunk])
        X, G = X.astype(f32), G.astype(f32)
        a = np.einsum("pij,pnj->pni", A, X)
        hv = np.einsum("pc,nc->pn", v, h[s0:s0 + chunk])
        phi = hv * _t32(coef, a, A)
        g = hv[..., None] * (b + np.einsum("ij,pnj->pni", W2, a))
        Ag = np.einsum("pij,pnj->pni", A, g)
        term = G[..., None] * (phi[..., None] * a - Ag)
        out[s0:s0 + chunk] = np.cumsum(term.astype(f32), axis=0, dtype=f32)[-1]
    return out
