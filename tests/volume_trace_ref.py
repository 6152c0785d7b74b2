"""Reference of the trace of the laplacian of a D = 3 field (function 4; not a test).

The trace is linear in the laplacian, so the brute-force oracle (oracle/volume.py) and the sample
gradient reference (tests/volume_sample_grad_ref.py) need no trace of their own:

    forward    oracle.volume.forward(2, ...)[:, [0, 4, 8], :].sum(1)
    gradients  oracle.volume.backward(2, ..., dL9), dL9 = the trace's upstream gradient on the
               full components 0, 4 and 8 ((0,0), (1,1), (2,2)) and zeros elsewhere
    dsamples   volume_sample_grad_ref.dsamples(2, ..., dL9)

dtype=np.float32: one float32 order of the same sums (float32 terms, added serially over the
Gaussians in index order), the measure of what float32 itself costs against the bound, as
`volume_sample_grad_ref.dsamples` offers it.
"""
import numpy as np

import volume_sample_grad_ref as vr
from oracle import volume as vo

DIAG = [0, 4, 8]  # the full components (0,0), (1,1), (2,2) of the laplacian's [N, 9, C]


def lift(dL):
    """the trace's upstream gradient [N, C] as the laplacian's [N, 9, C]"""
    dL = np.asarray(dL)
    N, C = dL.shape
    out = np.zeros((N, 9, C), dL.dtype)
    out[:, DIAG, :] = dL[:, None, :]
    return out


def forward(means, values, conics, samples, dtype=np.float64, chunk=512):
    """out [N, C]; float64: the oracle's laplacian contracted.  float32: v G t with float32 terms
    of the unique diagonal components, added serially over the Gaussians, then contracted."""
    if dtype == np.float64:
        return vo.forward(2, means, values, conics, samples)[:, DIAG, :].sum(1)
    P, N, C = means.shape[0], samples.shape[0], values.shape[1]
    out = np.zeros((N, C), np.float32)
    if P == 0 or N == 0:
        return out
    A = vo._amat(conics.astype(np.float64)).astype(np.float32)
    v = values.astype(np.float32)
    ud = [vo.pidx(i, i) for i in range(3)]
    for s0 in range(0, N, chunk):
        X, G, _ = vo._pairs(means, conics, samples[s0:s0 + chunk])
        X, G = X.astype(np.float32), G.astype(np.float32)
        a = np.einsum("pij,pnj->pni", A, X)
        t = vo._terms(2, a, A).astype(np.float32)[..., ud].sum(-1, dtype=np.float32)  # [P, n]
        term = (G * t)[:, :, None] * v[:, None, :]  # [P, n, C]
        out[s0:s0 + chunk] = np.cumsum(term.astype(np.float32), axis=0, dtype=np.float32)[-1]
    return out


def backward(means, values, conics, samples, dL):
    """(dmeans [P, 3], dvalues [P, C], dconics [P, 6]) of sum(dL * trace), float64"""
    return vo.backward(2, means, values, conics, samples, lift(dL))


def dsamples(means, values, conics, samples, dL, dtype=np.float64):
    """dL/d samples [N, 3] of sum(dL * trace)"""
    return vr.dsamples(2, means, values, conics, samples, lift(dL), dtype)
