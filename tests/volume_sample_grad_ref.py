"""Reference for the gradient with respect to the sample positions of a D = 3 field (not a test).

Brute force over every pair of every Gaussian, built on oracle/volume.py: X = wrap(mean - sample)
and the power in float32 exactly as `_pairs` forms them (the GPU does the same), G = exp(power)
unless power > 0, a = A X, and per pair the closed form of DESIGN.md section 4.9 at any D,

    dL/ds (pair) = G (phi a - A g) = -dL/dm (pair),
    phi = sum_u hv_u t_u,  g = d phi / d a,  hv_u = sum_ch v_ch h_u,ch,

with h the upstream gradient summed over the full components that share unique component u, t of
`oracle.volume._terms`, and g restated from `oracle.volume.backward`.  The wrap and the float32
rounding of the displacement count with slope 1 and the pair set is held fixed.  Everything after
X and the power is float64: `dsamples` is the authority of tests/test_gpu_volume_sample_grad.py.
`dsamples(..., dtype=np.float32)` is the same closed form with float32 terms, added serially over
the Gaussians in index order: one float32 order of the same sum, the measure of what float32
itself costs against the bound.  tests/test_volume_sample_grad_ref.py pins the float64 form
against torch float64 autograd of `torch_forward` below.
"""
import numpy as np

from oracle import volume as vo


def _hsum(function, dL, N, C):
    K, KU = 3 ** function, vo.NUNIQUE[function]
    dL = np.asarray(dL).reshape(N, K, C).astype(np.float64)
    hs = np.zeros((N, KU, C))
    for f, u in enumerate(vo.umap(function)):
        hs[:, u, :] += dL[:, f, :]
    return hs


def _g(function, hv, a, A):
    """g = d phi / d a [P, n, 3] for phi = sum_u hv_u t_u (oracle.volume.backward's g)"""
    g = np.zeros(a.shape, a.dtype)
    if function == 1:
        g = hv.copy()
    elif function == 2:
        for u, (i, j) in enumerate(vo.PAIRS):
            g[..., i] += hv[..., u] * a[..., j]
            g[..., j] += hv[..., u] * a[..., i]
    elif function == 3:
        for u, (i, j, k) in enumerate(vo.TRIPLES):
            hu = hv[..., u]
            g[..., k] += hu * A[:, i, j][:, None]
            g[..., j] += hu * A[:, i, k][:, None]
            g[..., i] += hu * A[:, j, k][:, None]
            g[..., i] -= hu * a[..., j] * a[..., k]
            g[..., j] -= hu * a[..., i] * a[..., k]
            g[..., k] -= hu * a[..., i] * a[..., j]
    return g


def dsamples(function, means, values, conics, samples, dL, dtype=np.float64, chunk=512):
    """dL/d samples [N, 3] of sum(dL * out) for one function (0..3); dL [N, 3^function, C].
    dtype float64: the authority (float32 X and power, float64 everything else, exact-order-free
    float64 sums).  dtype float32: float32 terms, summed serially over the Gaussians."""
    P, N, C = means.shape[0], samples.shape[0], values.shape[1]
    out = np.zeros((N, 3), dtype)
    if P == 0 or N == 0:
        return out
    A = vo._amat(conics.astype(np.float64)).astype(dtype)
    v = values.astype(dtype)
    hs = _hsum(function, dL, N, C).astype(dtype)
    for s0 in range(0, N, chunk):
        s = samples[s0:s0 + chunk]
        X, G, _ = vo._pairs(means, conics, s)
        X, G = X.astype(dtype), G.astype(dtype)
        a = np.einsum("pij,pnj->pni", A, X)
        t = vo._terms(function, a, A).astype(dtype)
        hv = np.einsum("pc,nuc->pnu", v, hs[s0:s0 + chunk])
        phi = np.einsum("pnu,pnu->pn", hv, t)
        g = _g(function, hv, a, A)
        Ag = np.einsum("pij,pnj->pni", A, g)
        term = G[..., None] * (phi[..., None] * a - Ag)  # [P, n, 3]
        if dtype == np.float64:
            out[s0:s0 + chunk] = term.sum(0)
        else:  # (cumsum adds in order: the serial float sum over the Gaussians)
            out[s0:s0 + chunk] = np.cumsum(term.astype(np.float32), axis=0, dtype=np.float32)[-1]
    return out


def dsamples_multi(functions, means, values, conics, samples, dLs, dtype=np.float64):
    """the sum of the per-function gradients (the loss is the sum over the functions)"""
    out = np.zeros((samples.shape[0], 3), dtype)
    for f, d in zip(functions, dLs):
        out = out + dsamples(f, means, values, conics, samples, d, dtype)
    return out


def torch_forward(function, means, values, conics, samples):
    """oracle.volume.forward restated in torch float64 for autograd with respect to any of its
    arguments: the same wrap (a per-pair constant shift, slope 1), the displacement rounded to
    float32 as `_pairs` forms it (slope 1 as well), the power skip and the terms."""
    import torch
    X = means[:, None, :] - samples[None, :, :]
    with torch.no_grad():
        Xd = X.detach().numpy()
        X32 = (means.detach().numpy().astype(np.float32)[:, None, :]
               - samples.detach().numpy().astype(np.float32)[None, :, :])
        shift = torch.from_numpy(vo._wrap(X32).astype(np.float64) - Xd)
    X = X + shift
    A = torch.zeros(means.shape[0], 3, 3, dtype=torch.float64)
    for q, (i, j) in enumerate(vo.PAIRS):
        A[:, i, j] = conics[:, q]
        A[:, j, i] = conics[:, q]
    power = -0.5 * torch.einsum("pni,pij,pnj->pn", X, A, X)
    G = torch.exp(power) * (power <= 0)
    a = torch.einsum("pij,pnj->pni", A, X)
    if function == 0:
        t = torch.ones(a.shape[:-1] + (1,), dtype=torch.float64)
    elif function == 1:
        t = a
    elif function == 2:
        t = torch.stack([a[..., i] * a[..., j] - A[:, i, j][:, None] for i, j in vo.PAIRS], -1)
    else:
        t = torch.stack([A[:, i, j][:, None] * a[..., k] + A[:, i, k][:, None] * a[..., j]
                         + A[:, j, k][:, None] * a[..., i] - a[..., i] * a[..., j] * a[..., k]
                         for i, j, k in vo.TRIPLES], -1)
    uo = torch.einsum("pn,pnu,pc->nuc", G, t, values)
    return uo[:, vo.umap(function), :]


def bound8c(ref, rtol=1e-5, atol_frac=1e-6):
    """the SURVEY 8c bound per element, rtol |ref| + atol_frac max|ref|"""
    ref = np.asarray(ref, np.float64)
    return rtol * np.abs(ref) + atol_frac * (float(np.abs(ref).max()) if ref.size else 0.0)
