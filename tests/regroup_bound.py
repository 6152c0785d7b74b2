"""The a-priori bound between two float32 evaluations that add the same terms in another order
(not a test): per-element sum |term| over the oracle's pair set, and the bound built from it.
Used by tests/test_gpu_flush_cut.py; tests/test_regroup_bound.py pins the terms on the CPU."""
import numpy as np
import torch

import sample_grad_ref as sgr
from oracle.torch_eager import _wrap

U = 2.0 ** -24


def _pair_terms(k, a, A):
    """t of function k (sample_grad_ref._terms) with a per-pair conic matrix: a [S, G, D],
    A [S, G, D, D]; returns [S, G, D^k]."""
    if k == 0:
        t = torch.ones_like(a[..., :1])
    elif k == 1:
        t = a
    else:
        aa = a[..., :, None] * a[..., None, :]
        if k == 2:
            t = aa - A
        else:
            Aa = A[..., :, :, None] * a[..., None, None, :]
            t = Aa + Aa.permute(0, 1, 2, 4, 3) + Aa.permute(0, 1, 4, 2, 3) - aa[..., None] * a[..., None, None, :]
    return t.reshape(a.shape[0], a.shape[1], -1)


def abs_term_sums(ob, f, means, values, conics, samples, dL, q_live, device="cpu", pairs_per_chunk=1 << 18):
    """Per output element of function f, over the ORACLE's pair set (OracleBins `ob`) in float64:
    {name: (sum |term|, signed sum of the terms, n)} for name in forward [N, K, C], dmeans [P, D],
    dvalues [P, C], dconics [P, S], dsamples [N, D]; n (broadcastable) is the number of the
    element's pairs with q = X^T A X <= q_live, the ones that can carry a non-zero term.

    The pairs are sample_grad_ref's (the sample's tile, that tile's Gaussians, X = wrap(fp32(m - s))).
    Every pair gets its OWN copy of X, conic and value as autograd leaves, so the gradient of
    sum(out * dL) with respect to those copies is the pair's term of dmeans (= -dsamples), dconics
    and dvalues: no closed form is restated here.  The signed sums are returned so that
    tests/test_regroup_bound.py can hold them against the oracle's forward and exact backward."""
    D, C = means.shape[1], values.shape[1]
    N, P, k = samples.shape[0], means.shape[0], sgr.FUNCS[f]
    S3 = D * (D + 1) // 2
    f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).double().to(device)  # noqa: E731
    m, v, c, s = f64(means), f64(values), f64(conics).reshape(P, S3), f64(samples)
    dl = f64(dL).reshape(N, D ** k, C)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=device)  # noqa: E731
    shapes = {"forward": (N, D ** k, C), "dmeans": (P, D), "dvalues": (P, C), "dconics": (P, S3), "dsamples": (N, D)}
    acc = {n: (z(*sh), z(*sh)) for n, sh in shapes.items()}  # (sum |term|, signed sum)
    nf, ng = z(N), z(P)
    keys = ob.sample_keys()
    for t in np.unique(keys):
        if t < 0 or t >= ob.T:  # never rendered
            continue
        gid = torch.from_numpy(ob.tile_gaussians(int(t)).astype(np.int64)).to(device)
        if gid.numel() == 0:
            continue
        rows = np.nonzero(keys == t)[0]
        chunk = max(1, pairs_per_chunk // gid.numel())
        for b in range(0, len(rows), chunk):
            sid = torch.from_numpy(rows[b:b + chunk].astype(np.int64)).to(device)
            X = _wrap((m[gid][None] - s[sid][:, None]).float().double()).requires_grad_(True)  # [S, G, D]
            cp = c[gid][None].expand(sid.numel(), -1, -1).clone().requires_grad_(True)
            vp = v[gid][None].expand(sid.numel(), -1, -1).clone().requires_grad_(True)
            if D == 1:
                q = cp[..., 0] * X[..., 0] ** 2
                A = cp[..., None]
            else:
                q = cp[..., 0] * X[..., 0] ** 2 + 2 * cp[..., 1] * X[..., 0] * X[..., 1] + cp[..., 2] * X[..., 1] ** 2
                A = torch.stack([cp[..., :2], cp[..., 1:]], -2)
            G = torch.where(q < 0, torch.zeros_like(q), torch.exp(-0.5 * q))  # (power > 0: G = 0)
            a = (A * X[..., None, :]).sum(-1)
            T = G[..., None] * _pair_terms(k, a, A)                              # [S, G, K]
            torch.einsum("sgk,sgc,skc->", T, vp, dl[sid]).backward()
            Td, vd = T.detach(), vp.detach()
            acc["forward"][0][sid] = torch.einsum("sgk,sgc->skc", Td.abs(), vd.abs())
            acc["forward"][1][sid] = torch.einsum("sgk,sgc->skc", Td, vd)
            acc["dsamples"][0][sid] = X.grad.abs().sum(1)
            acc["dsamples"][1][sid] = -X.grad.sum(1)
            gc = cp.grad
            if D == 1 and k == 3:
                # the reference's D = 1 third-derivative dconics is not the true derivative
                # (oracle_bwd_body.h, backward.cu:322-325); every implementation reproduces it
                x, x1 = X.detach()[..., 0], (cp.detach() * X.detach())[..., 0]
                H = torch.einsum("sgc,sc->sg", vd, dl[sid][:, 0, :])
                gc = ((2 * x * x - 2 * x1 * x1 * x - 0.5 * (2 * x * x1 - x) * x * x
                       + 0.5 * (x1 * x1 - cp.detach()[..., 0]) * x1 * x * x) * H * G.detach())[..., None]
            for name, g in (("dmeans", X.grad), ("dvalues", vp.grad), ("dconics", gc)):
                acc[name][0].index_add_(0, gid, g.abs().sum(0))
                acc[name][1].index_add_(0, gid, g.sum(0))
            live = (q.detach() <= q_live).double()
            nf[sid] = live.sum(1)
            ng.index_add_(0, gid, live.sum(0))
    nf, ng = nf.cpu().numpy(), ng.cpu().numpy()
    counts = {"forward": nf[:, None, None], "dsamples": nf[:, None], "dmeans": ng[:, None], "dvalues": ng[:, None],
              "dconics": ng[:, None]}
    return {n: (a.cpu().numpy(), sg.cpu().numpy(), counts[n]) for n, (a, sg) in acc.items()}


def regroup_bound(B, abs_sum, n, calls=1):
    """The a-priori bound on the distance between two float32 evaluations of one output element
    whose pair sets differ only by exact zeros and whose non-zero terms are added in another order:

        B + 2 n calls u (sum |term| + B),   u = 2^-24.

    B (helpers.order_bounds) bounds sum |term_any order - term|, the exponent's evaluation order:
    two binnings may send a pair through different fast paths.  A float sum of n terms in ANY
    order (serial, tree, atomics) is within (n - 1) u sum |term| (1 + O(n u)) of the exact sum of
    those terms (standard summation analysis), so two orders differ by at most twice that, and the
    float32 terms' magnitudes add up to at most sum |term| + B.  n counts the element's pairs that
    can carry a non-zero term -- every other term is an exact zero and adds no rounding -- and n
    instead of n - 1 absorbs the O(n u) factor (n < 1e5).  `calls`: launches added into the element
    (the sample-position gradient outside D = 2, C = 1 adds one call per function).  Nothing
    measured enters.  What it still detects: an element fed only by far pairs has a sum |term| of
    the size of those terms, so a dropped non-zero term t stands out once |t| > 2 n u sum |term|
    (n up to a few thousand) -- at any G, with no absolute floor."""
    B = np.asarray(B, np.float64)
    return B + 2.0 * np.asarray(n, np.float64) * calls * U * (np.asarray(abs_sum, np.float64).reshape(B.shape) + B)
