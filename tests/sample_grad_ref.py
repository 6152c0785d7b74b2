"""Reference for the gradient with respect to the sample positions (not a test).

A torch restatement of the four sampling functions' forward over the ORACLE's pair set: each
sample's tile from OracleBins.sample_keys(), that tile's Gaussians from tile_gaussians(t),
X = wrap(mean - sample) with the period-2 wrap of oracle/torch_eager.py:_wrap, G = exp(power)
unless power > 0, out = sum_g v G t(a, A) with a = A X and the terms of dgs_render.h fwd_terms
(written once for any D as symmetric tensors:
  t = 1 | a_i | a_i a_j - A_ij | A_ij a_k + A_ik a_j + A_jk a_i - a_i a_j a_k).
In float64 with samples.requires_grad, dL/dsamples is autograd of sum(out * dL): the authority.
The displacement mean - sample is rounded to float32 first, as every float32 evaluation of the
reference's expression forms it (at sigma ~ 0.005 and |mean - sample| ~ 0.01 that rounding alone
moves a third derivative by 3e-5 of its value); like the wrap, the rounding has slope 1.

From the same pairs the helper also evaluates the per-pair closed form
  dL/ds (pair) = G (phi a - A g),  phi = sum_k H_k t_k,  g = d phi / d a,  H = sum_ch v_ch dL_k,ch
- in float64 (its sum must equal autograd's: tests/test_sample_grad_ref.py),
- in float32, summed serially in list order ("the reference's own float order"),
- and the a-priori exponent-order bound of DESIGN.md section 6 for this output,
  B = sum_pairs |term| (exp(gamma_6 M) - 1), M = 0.5|c0 X0^2| + |c1 X0 X1| + 0.5|c2 X1^2|.
"""
import numpy as np
import torch

from oracle.torch_eager import _wrap

FUNCS = {"gaussian": 0, "derivative": 1, "laplacian": 2, "third": 3}
_U = 2.0 ** -24
GAMMA6 = 6 * _U / (1 - 6 * _U)


def _terms(f, a, A):
    """t of function f, shape [S, G] + [D] * f; a [S, G, D], A [G, D, D]."""
    if f == 0:
        return torch.ones(a.shape[:2], dtype=a.dtype)
    if f == 1:
        return a
    aa = a[..., :, None] * a[..., None, :]
    if f == 2:
        return aa - A[None]
    Aa = A[None, :, :, :, None] * a[:, :, None, None, :]           # A_ij a_k
    return Aa + Aa.permute(0, 1, 2, 4, 3) + Aa.permute(0, 1, 4, 2, 3) - aa[..., None] * a[:, :, None, None, :]


def _phi_g(f, a, A, H):
    """phi = <H, t> and g = d phi / d a for function f; H [S, G] + [D] * f."""
    t = _terms(f, a, A)
    if f == 0:
        return H * t, torch.zeros_like(a)
    if f == 1:
        return (H * t).sum(-1), H
    if f == 2:
        return (H * t).sum((-1, -2)), (H * a[..., None, :]).sum(-1) + (H * a[..., :, None]).sum(-2)
    phi = (H * t).sum((-1, -2, -3))
    aa = a[..., :, None] * a[..., None, :]
    Ab = A[None]
    g = ((H * Ab[..., :, :, None]).sum((-2, -3)) + (H * Ab[..., :, None, :]).sum((-1, -3))
         + (H * Ab[..., None, :, :]).sum((-1, -2))
         - (H * aa[..., None, :, :]).sum((-1, -2)) - (H * aa[..., :, None, :]).sum((-1, -3))
         - (H * aa[..., :, :, None]).sum((-2, -3)))
    return phi, g


def _conic_matrix(c, D):
    if D == 1:
        return c.reshape(-1, 1, 1)
    return torch.stack([torch.stack([c[:, 0], c[:, 1]], -1), torch.stack([c[:, 1], c[:, 2]], -1)], -2)


def _power(X, c, D):
    if D == 1:
        return -0.5 * c[None, :, 0] * X[..., 0] * X[..., 0]
    return (-0.5 * (c[None, :, 0] * X[..., 0] * X[..., 0] + c[None, :, 2] * X[..., 1] * X[..., 1])
            - c[None, :, 1] * X[..., 0] * X[..., 1])


def sample_grad_ref(ob, functions, means, values, conics, samples, dLs, chunk=512):
    """functions: names; dLs: one dL/dout per function ([N, D^f, C] after reshape).  Returns a
    dict: outs {f: [N, D^f, C]}, dsamples / dmeans (float64 autograd of the summed loss),
    closed (the closed form summed in float64), serial32 (float32 terms, serial list order),
    bound (the a-priori exponent-order bound B), all [N, D]."""
    D = int(np.asarray(means).shape[1])
    N, C = int(np.asarray(samples).shape[0]), int(np.asarray(values).shape[1])
    f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).double()  # noqa: E731
    m = f64(means).requires_grad_(True)
    s = f64(samples).requires_grad_(True)
    v, c = f64(values), f64(conics).reshape(len(m), -1)
    codes = [FUNCS[f] for f in functions]
    dl = [f64(np.asarray(d)).reshape([N] + [D] * k + [C]) for d, k in zip(dLs, codes)]
    outs = {f: torch.zeros([N] + [D] * k + [C], dtype=torch.float64) for f, k in zip(functions, codes)}
    closed = torch.zeros(N, D, dtype=torch.float64)
    bound = torch.zeros(N, D, dtype=torch.float64)
    serial = np.zeros((N, D), np.float32)
    keys = ob.sample_keys()
    A = _conic_matrix(c, D)
    for t in np.unique(keys):
        if t < 0 or t >= ob.T:  # never rendered: output and gradient stay 0
            continue
        gid = torch.from_numpy(ob.tile_gaussians(int(t)).astype(np.int64))
        if gid.numel() == 0:
            continue
        rows = np.nonzero(keys == t)[0]
        for b in range(0, len(rows), chunk):
            sid = torch.from_numpy(rows[b:b + chunk].astype(np.int64))
            X = m[gid][None, :, :] - s[sid][:, None, :]                        # [S, G, D], exact in float64
            X = _wrap(X + (X.detach().float().double() - X.detach()))          # rounded as float32 forms it
            power = _power(X, c[gid], D)
            G = torch.where(power > 0, torch.zeros_like(power), torch.exp(power))
            Ag = A[gid]
            a = (Ag[None] * X[..., None, :]).sum(-1)
            loss = 0.0
            for f, k, d in zip(functions, codes, dl):
                tt = _terms(k, a, Ag)                                          # [S, G] + [D] * k
                o = torch.einsum("sg...,gc->s...c", G.reshape(G.shape + (1,) * k) * tt, v[gid])
                outs[f][sid] = o.detach()
                loss = loss + (o * d[sid]).sum()
            loss.backward()
            # the closed form per pair, float64 and float32
            for dt in (torch.float64, torch.float32):
                Xd, cd, Ad = X.detach().to(dt), c[gid].to(dt), Ag.to(dt)
                if dt == torch.float32:  # the displacement as float32 arithmetic forms it
                    Xd = _wrap(m.detach()[gid].float()[None] - s.detach()[sid].float()[:, None])
                pw = _power(Xd, cd, D)
                Gd = torch.where(pw > 0, torch.zeros_like(pw), torch.exp(pw))
                ad = (Ad[None] * Xd[..., None, :]).sum(-1)
                phi = torch.zeros_like(Gd)
                g = torch.zeros_like(ad)
                for k, d in zip(codes, dl):
                    H = torch.einsum("s...c,gc->sg...", d[sid].to(dt), v[gid].to(dt))
                    p_, g_ = _phi_g(k, ad, Ad, H)
                    phi, g = phi + p_, g + g_
                term = Gd[..., None] * (phi[..., None] * ad - (Ad[None] * g[..., None, :]).sum(-1))  # [S, G, D]
                if dt == torch.float64:
                    closed[sid] = term.sum(1)
                    M = 0.5 * (cd[None, :, 0] * Xd[..., 0] ** 2).abs()
                    if D == 2:
                        M = M + (cd[None, :, 1] * Xd[..., 0] * Xd[..., 1]).abs() + 0.5 * (cd[None, :, 2] * Xd[..., 1] ** 2).abs()
                    bound[sid] = (term.abs() * torch.expm1(GAMMA6 * M)[..., None]).sum(1)
                else:  # (cumsum adds in order: the serial float sum over the list)
                    serial[sid.numpy()] = np.cumsum(term.numpy(), axis=1, dtype=np.float32)[:, -1]
    zero = torch.zeros(N, D, dtype=torch.float64)
    return {"outs": {f: o.reshape(N, -1, C).numpy() for f, o in outs.items()},
            "dsamples": (s.grad if s.grad is not None else zero).numpy(),
            "dmeans": (m.grad if m.grad is not None else torch.zeros_like(m)).numpy(),
            "closed": closed.numpy(), "serial32": serial, "bound": bound.numpy()}


# ------------------------------------------------------------------------------ the cases
# Shared by tests/test_sample_grad_ref.py (CPU: pins this helper on every case) and
# tests/test_gpu_sample_grad.py.  name -> (functions, means, values, covs, conics, samples);
# the dL of function i is synthetic.grad_out(N, D^f, C, seed=DL_SEED + i).
DL_SEED = 405


def _golden(name):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return tuple(torch.from_numpy(z[k]) for k in ("means", "values", "covariances", "conics", "samples"))


def _case_inputs(name):
    import cases
    from diff_gaussian_sampling import synthetic as syn
    if name.startswith("d2_c1_"):           # the four functions on the d2_c1_1k_4k inputs
        return (name[6:],), _golden("d2_c1_1k_4k")
    if name.startswith("multi_"):           # fused masks (D = 2, C = 1), same inputs
        fs = {"gl": ("gaussian", "laplacian"), "all": ("gaussian", "derivative", "laplacian", "third")}[name[6:]]
        return fs, _golden("d2_c1_1k_4k")
    if name.startswith("d2_c"):             # d2_c{3,5,16}_{function}: the general path
        C, f = name[4:].split("_")
        return (f,), syn.gaussians(300, 2, int(C), seed=411) + (syn.samples(1100, 2, seed=412),)
    if name == "d1_c3_multi":               # two functions outside D = 2, C = 1: per-function calls, added
        return ("gaussian", "third"), syn.gaussians(200, 1, 3, seed=421) + (syn.samples(1500, 1, seed=422),)
    if name.startswith("d1_c"):             # d1_c{1,3}_{function}
        C, f = name[4:].split("_")
        return (f,), syn.gaussians(200, 1, int(C), seed=421) + (syn.samples(1500, 1, seed=422),)
    if name == "edge":
        return ("derivative",), cases.edge_case(n_random=1500)
    if name == "far_means":
        return ("laplacian",), cases.far_means_case(n=1500)
    if name == "aliasing":                  # plus the corner sample: x-tile == grid in the last row,
        m, v, cv, c, s = cases.aliasing_case(n=2000, P=300)  # a key past the last tile (never rendered)
        return ("gaussian",), (m, v, cv, c, torch.cat([s, torch.tensor([[float(s[:, 0].max()), 1.0]])]))
    if name == "d1_zero_variance":
        return ("third",), cases.d1_zero_variance_case()
    if name == "duplicates":                # identical rows must get identical gradients
        m, v, cv, c = syn.gaussians(300, 2, 1, seed=431)
        s = syn.samples(1000, 2, seed=432)
        s[500:] = s[:500]
        return ("third",), (m, v, cv, c, s)
    if name == "thin":
        return ("laplacian",), cases.thin_case(P=1500, n=6000)
    raise KeyError(name)


CASE_NAMES = (["d2_c1_" + f for f in FUNCS] + ["multi_gl", "multi_all"]
              + [f"d2_c{C}_{f}" for C, f in ((3, "derivative"), (5, "laplacian"), (16, "third"))]
              + [f"d1_c{C}_{f}" for C in (1, 3) for f in ("gaussian", "third")]
              + ["d1_c3_multi", "edge", "far_means", "aliasing", "d1_zero_variance", "duplicates", "thin"])

_cache = {}


def case(name):
    """(functions, inputs (means, values, covs, conics, samples) as float32 tensors, dLs, the
    oracle's bins, sample_grad_ref's result) of a case -- computed once per process."""
    if name not in _cache:
        from diff_gaussian_sampling import synthetic as syn
        from oracle import oracle as orc
        functions, inputs = _case_inputs(name)
        means, values, covs, conics, samples = (t.float().contiguous() for t in inputs)
        N, D, C = samples.shape[0], means.shape[1], values.shape[1]
        dLs = [syn.grad_out(N, D ** FUNCS[f], C, seed=DL_SEED + i) for i, f in enumerate(functions)]
        if name == "duplicates":  # identical rows: the same position and the same dL
            for d in dLs:
                d[N // 2:] = d[:N // 2]
        ob = orc.OracleBins(means.numpy(), covs.numpy(), samples.numpy())
        ref = sample_grad_ref(ob, functions, means.numpy(), values.numpy(), conics.numpy(), samples.numpy(),
                              [d.numpy() for d in dLs])
        _cache[name] = (functions, (means, values, covs, conics, samples), dLs, ob, ref)
    return _cache[name]
