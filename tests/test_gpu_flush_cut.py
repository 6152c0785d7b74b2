"""The fast cut kQCutFast (dgs_internal.h): entries that only the fast paths
evaluate are binned with X^T A X <= 176 instead of the reference's 210, because the fast paths'
bare v_exp_f32 returns exactly +0 for every log2 exponent below -126.

- Probe: the hardware fact, over every float of [-160, -120].
- Ring: pairs just outside the fast cut are exact zeros in the forward's and the backward's
  evaluation order; pairs just inside q = 174 are not.
- Equivalence: binning with the fast cut and with the reference cut for every entry
  (DGS_BIN_QCUT_REFERENCE) gives the same R / ranges / radii bit for bit, never more entries, and
  outputs and gradients within helpers.order_bounds' B plus the per-element summation-order
  allowance 2 n u (sum |term| + B) of regroup_bound.py -- no relative or absolute floor (the lists
  are regrouped, so the float sums are not bit-equal); the live pairs the lists hold at the flush
  threshold (count_pairs) are the same number under both cuts.
- Empty lists: cells and sub-cells whose only entry the fast cut removes give exact zeros.
"""
import math

import numpy as np
import pytest
import torch

import cases
import sample_grad_ref as sgr
from diff_gaussian_sampling import synthetic as syn
from helpers import FUNCS, FWD_NAME, order_bounds
from regroup_bound import abs_term_sums, regroup_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2E = 1.4426950408889634


def _constants(dgs):
    """(kQCut, kQCutFast, kRho2Max, kExp2FlushBelow) of dgs_internal.h, from the library itself."""
    return dgs._C.cut_constants()


# ------------------------------------------------------------------------------ probe
def _probe_threshold(dgs):
    """(T, x, out): every float of [-160, -120] through fast_exp2; T = the lowest input whose
    result is not +0."""
    bits = np.arange(0xC2F00000, 0xC3200000 + 1, dtype=np.int64).astype(np.uint32)  # -120 ... -160
    x = bits.view(np.float32)
    assert x[0] == -120.0 and x[-1] == -160.0 and x.size == 0x300001
    out = dgs._C.exp2_probe(torch.from_numpy(x).to(DEV)).cpu().numpy()
    nz = out.view(np.uint32) != 0
    assert nz.any()
    return float(x[nz].min()), x, out


def test_exp2_probe_flushes_below_threshold(dgs):
    """v_exp_f32 delivers no subnormal: exactly +0 (the bit pattern) below the threshold T, a normal
    number from T up; T is -126 (2^-126 is the smallest normal), and kQCutFast puts the COMPUTED
    exponent of every culled pair below T (the derivation at dgs_internal.h kQCutFast)."""
    T, x, out = _probe_threshold(dgs)
    below, above = x < T, x >= T
    print(f"exp2 probe: lowest input with a non-zero result T = {T!r}; {int(below.sum())} inputs below, "
          f"{int(above.sum())} from T up")
    assert np.all(out[below].view(np.uint32) == 0), "a non-zero (or -0) result below the threshold"
    assert np.all(out[above] >= 2.0 ** -126), "a zero or subnormal result at or above the threshold"
    q_ref, qf, rho2_max, flush_below = _constants(dgs)
    assert qf == dgs._C.qcut_fast() and q_ref == 210.0
    # the threshold the header's derivation (and its static_assert) starts from is the measured one
    assert T == flush_below == -126.0
    assert -2.0 * T / LOG2E < qf < q_ref  # (174.7: the exact-arithmetic cut; the margin above it is the header's)


# ------------------------------------------------------------------------------ ring
def _ring_gaussians2():
    """64 conics at D = 2 as (covariance factor L with Sigma = L L^T in float64 of the float32
    conic, float32 mean, float32 conic): isotropic, axis ratio 3, thin up to rho^2 just under
    kRho2Max; the major sigma from the headline's smallest width (h / 2 = 0.001 at P = 1M) up to a
    reference extent sqrt(210 Sigma_dd) just under 0.5."""
    rng = np.random.default_rng(7)
    specs = []
    for s in np.geomspace(0.001, 0.0344, 16):                      # isotropic: e_ref = 14.49 s < 0.4985
        specs.append((s, s, 0.0))
    for s in np.geomspace(0.003, 0.034, 16):                       # axis ratio 3, any rotation
        specs.append((s, s / 3.0, rng.uniform(0, math.pi)))
    # thin: at 45 degrees rho = (r^2 - 1) / (r^2 + 1); rho^2 in [0.82, 0.9994]
    for rho2, s in zip(np.linspace(0.82, 0.9994, 32), np.tile(np.geomspace(0.003, 0.047, 8), 4)):
        rho = math.sqrt(rho2)
        r = math.sqrt((1 + rho) / (1 - rho))
        specs.append((s, s / r, math.pi / 4 if len(specs) % 2 else -math.pi / 4))
    means = rng.uniform(-0.9, 0.9, (len(specs), 2)).astype(np.float32)
    conics = np.zeros((len(specs), 3), np.float32)
    for i, (s0, s1, th) in enumerate(specs):
        c, s = math.cos(th), math.sin(th)
        xx, xy, yy = c * c * s0 ** 2 + s * s * s1 ** 2, c * s * (s0 ** 2 - s1 ** 2), s * s * s0 ** 2 + c * c * s1 ** 2
        det = xx * yy - xy * xy
        conics[i] = [yy / det, -xy / det, xx / det]
    return means, conics


def _ring_pairs(means, conics, q_targets, seed):
    """Per Gaussian, len(q_targets) samples s = m - X (rounded to float32) with X on the ellipse
    X^T A X = q_target of the float32 conic; returns flat float32 (means, conics, samples) and the
    float64 q of the rounded inputs."""
    rng = np.random.default_rng(seed)
    n, D = means.shape
    k = len(q_targets)
    c = conics.astype(np.float64)
    if D == 1:
        X = (np.sqrt(q_targets)[None, :] / np.sqrt(c[:, :1])) * rng.choice([-1.0, 1.0], (n, k))
        X = X[..., None]
    else:
        A = np.stack([np.stack([c[:, 0], c[:, 1]], -1), np.stack([c[:, 1], c[:, 2]], -1)], -2)
        L = np.linalg.cholesky(np.linalg.inv(A))                   # Sigma = L L^T
        phi = rng.uniform(0, 2 * math.pi, (n, k))
        u = np.stack([np.cos(phi), np.sin(phi)], -1) * np.sqrt(q_targets)[None, :, None]
        X = np.einsum("nij,nkj->nki", L, u)
    s32 = (means.astype(np.float64)[:, None, :] - X).astype(np.float32)
    m = np.repeat(means[:, None, :], k, 1).reshape(-1, D)
    cc = np.repeat(conics[:, None, :], k, 1).reshape(n * k, -1)
    s = s32.reshape(-1, D)
    Xr = m.astype(np.float64) - s.astype(np.float64)
    c = cc.astype(np.float64)
    q = c[:, 0] * Xr[:, 0] ** 2 if D == 1 else c[:, 0] * Xr[:, 0] ** 2 + 2 * c[:, 1] * Xr[:, 0] * Xr[:, 1] + c[:, 2] * Xr[:, 1] ** 2
    return m, cc, s, q


def _amplification(cc):
    if cc.shape[1] == 1:
        return np.ones(len(cc))
    c = cc.astype(np.float64)
    rho = np.abs(c[:, 1]) / np.sqrt(c[:, 0] * c[:, 2])
    return (1 + rho) / (1 - rho)


@pytest.mark.parametrize("D", [2, 1])
def test_ring_pairs_are_hardware_zeros(dgs, D):
    """Pairs with fp64 q > kQCutFast give exactly +0 in the forward's fma form and in the gaussian
    backward's monomial form (D = 2); pairs with q just below 174 do not.

    The pair hook returns G and the fp32 exponent p of that evaluation order.  The inner pairs' G
    is within 1e-5 relative of 2^p evaluated in fp64 (the accuracy of the exponential itself), and p
    is within the a-priori exponent-order bound 3e-7 A q log2(e) of the fp64 exponent
    -(log2(e) / 2) q (dgs_internal.h): with A up to 8000 the exponent itself is not 1e-5 accurate,
    which is why G is compared with 2^p of the computed p."""
    Q_REF, qf, RHO2_MAX, _ = _constants(dgs)
    if D == 2:
        means, conics = _ring_gaussians2()
        c = conics.astype(np.float64)
        rho2 = c[:, 1] ** 2 / (c[:, 0] * c[:, 2])
        det = c[:, 0] * c[:, 2] - c[:, 1] ** 2
        e_ref = np.sqrt(Q_REF * np.maximum(c[:, 0], c[:, 2]) / det)
        assert len(means) == 64 and rho2.max() < RHO2_MAX and rho2.max() > 0.999 and e_ref.max() < 0.5
        assert e_ref.max() > 0.49 and (rho2 == 0).sum() == 16
    else:
        rng = np.random.default_rng(9)
        sig = np.geomspace(0.001, 0.0344, 16)
        means = rng.uniform(-0.9, 0.9, (16, 1)).astype(np.float32)
        conics = (1.0 / sig ** 2).astype(np.float32)[:, None]
        assert math.sqrt(Q_REF) * sig.max() < 0.5
    rng = np.random.default_rng(11)
    outer_t = np.concatenate([rng.uniform(qf + 0.02, qf + 1.0, 192), rng.uniform(qf + 1.0, Q_REF + 5.0, 64)])
    inner_t = rng.uniform(173.0, 173.9, 32)
    mo, co, so, qo = _ring_pairs(means, conics, outer_t, 12)
    mi, ci, si, qi = _ring_pairs(means, conics, inner_t, 13)
    # the chosen inputs put the pairs where intended (float64 of the rounded float32 inputs)
    assert np.all(qo > qf) and qo.min() < qf + 0.05 and np.all(qi < 174.0) and np.all(qi > 172.9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    for form in ((0, 1) if D == 2 else (0,)):
        G, p = (r.cpu().numpy() for r in dgs._C.pair_probe(t(mo), t(co), t(so), form))
        print(f"D={D} form {form}: outer pairs max computed exponent {p.max():.4f} (threshold -126), "
              f"non-zero G: {int((G.view(np.uint32) != 0).sum())} of {G.size}")
        assert np.all(G.view(np.uint32) == 0), "a pair beyond kQCutFast is not an exact +0"
        assert p.max() < -126.0
        G, p = (r.cpu().numpy() for r in dgs._C.pair_probe(t(mi), t(ci), t(si), form))
        exact = -0.5 * LOG2E * qi
        # the exponent's terms are rounded in fp32 (3e-7 A q, dgs_internal.h); X = m - s itself is
        # rounded once: |dq| <= 2 sqrt(q lambda_max) u (|m| + |s|), lambda_max <= c0 + c2
        lam = ci.astype(np.float64)[:, 0] + (ci.astype(np.float64)[:, 2] if D == 2 else 0.0)
        dq = 2 * np.sqrt(qi * lam) * 2.0 ** -24 * (np.abs(mi).sum(1) + np.abs(si).sum(1))
        bound = LOG2E * (3e-7 * _amplification(ci) * qi + 0.5 * dq)
        rel = np.abs(G.astype(np.float64) / np.exp2(p.astype(np.float64)) - 1.0)
        print(f"D={D} form {form}: inner pairs min G {G.min():.3e}, max |G / 2^p - 1| {rel.max():.2e}, "
              f"max |p - exact| / bound {np.max(np.abs(p - exact) / bound):.3f}")
        assert np.all(G > 0.0), "a pair just below q = 174 evaluates to zero"
        assert np.all(rel <= 1e-5)
        assert np.all(np.abs(p - exact) <= bound)


# ------------------------------------------------------------------------------ equivalence
def _field(P, D, C, seed, h):
    """syn.gaussians with per-axis sigma ~ h U[0.5, 1.5]."""
    return syn.gaussians(P, D, C, seed=seed, scale=h / (2.0 / P ** (1.0 / D)))


def _with_values(inputs, C, seed):
    m, v, cv, c, s = inputs
    g = torch.Generator().manual_seed(seed)
    return m, torch.randn(m.shape[0], C, generator=g), cv, c, s


# name -> (inputs, strict).  The fine cells hold ~150 samples each, so at D = 2 the N <= 4001 shapes
# have ONE cell per tile: the tiles come from the reference's 3 sigma rect, far inside either cut,
# and no list can differ (the entry counts are equal there; the sub lists still use the fast cut).
# The D = 2 lists first differ at 4 x 4 cells per tile, N >= 29400 on the 4 x 4 tile grid: the
# *_n30011 cases.  strict = the case certainly has cells that only the ring 176 < q <= 210 of some
# Gaussian reaches (hundreds of Gaussians whose extent is a fraction of a cell, so that a cell
# edge falls into the ring of one in five), and the fine entry count must fall.
EQ_CASES = {
    "d2_p3000_n4001_c1": (lambda: syn.gaussians(3000, 2, 1, seed=501) + (syn.samples(4001, 2, seed=502),), False),
    "d2_p257_n4001_c3": (lambda: _field(257, 2, 3, 503, 0.015) + (syn.samples(4001, 2, seed=504),), False),
    "d2_p3000_n3_c16": (lambda: syn.gaussians(3000, 2, 16, seed=505) + (syn.samples(3, 2, seed=506),), False),
    "d2_p1_n4001_c1": (lambda: _field(1, 2, 1, 507, 0.02) + (syn.samples(4001, 2, seed=508),), False),
    "d2_p257_n1_c3": (lambda: _field(257, 2, 3, 509, 0.015) + (syn.samples(1, 2, seed=510),), False),
    "d2_p1_n1_c1": (lambda: _field(1, 2, 1, 511, 0.02) + (syn.samples(1, 2, seed=512),), False),
    "d1_p3000_n4001_c3": (lambda: syn.gaussians(3000, 1, 3, seed=513) + (syn.samples(4001, 1, seed=514),), True),
    "d1_p257_n3_c1": (lambda: syn.gaussians(257, 1, 1, seed=515) + (syn.samples(3, 1, seed=516),), False),
    "d1_p1_n4001_c16": (lambda: _field(1, 1, 16, 517, 0.02) + (syn.samples(4001, 1, seed=518),), False),
    "seam_d2_c1": (lambda: cases.seam_case(D=2, P=400, n=4000, C=1), False),
    "seam_d1_c3": (lambda: cases.seam_case(D=1, P=400, n=4000, C=3), True),
    "thin_p3000_n4001_c1": (lambda: cases.thin_case(P=3000, n=4001, C=1), False),
    "thin_p257_n4001_c16": (lambda: cases.thin_case(P=257, n=4001, C=16), False),
    "edge_c1": (lambda: cases.edge_case(n_random=3000), False),
    "edge_c3": (lambda: _with_values(cases.edge_case(n_random=3000), 3, 519), False),
    "d2_p3000_n30011_c1": (lambda: _field(3000, 2, 1, 521, 0.006) + (syn.samples(30011, 2, seed=522),), True),
    "d2_p257_n30011_c3": (lambda: _field(257, 2, 3, 523, 0.006) + (syn.samples(30011, 2, seed=524),), True),
    "seam_d2_n30011_c1": (lambda: cases.seam_case(D=2, P=400, n=30011, C=1), True),
    "thin_p3000_n30011_c1": (lambda: cases.thin_case(P=3000, n=30011, C=1), True),
}
# the sample-position gradient (all four functions in one call) on these
SGRAD_CASES = ("d2_p257_n4001_c3", "d1_p257_n3_c1", "seam_d1_c3", "edge_c1", "d2_p1_n1_c1", "d2_p257_n30011_c3")


def _both_binnings(dgs, inputs):
    m, v, cv, c, s = (t.float().contiguous().to(DEV) for t in inputs)
    fast = dgs._C.preprocess_gaussians(m, v, cv, c, s, False)
    ref = dgs._C.preprocess_gaussians_refcut(m, v, cv, c, s, False)
    return (m, v, c, s), fast, ref


def _agree(got, ref, bound, what):
    """|got - ref| <= bound elementwise, no relative or absolute floor."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.asarray(bound, np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    worst = float(np.max(err / (bound + 1e-300))) if err.size else 0.0
    print(f"{what}: max |diff| / bound = {worst:.4f}, max |diff| = {float(err.max()) if err.size else 0.0:.3e}")
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err / (bound + 1e-300)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.size} elements beyond the regrouping bound; worst at {i}: "
                             f"fast cut {got[i]!r} reference cut {ref[i]!r} bound {bound[i]!r}")


@pytest.mark.parametrize("name", list(EQ_CASES))
def test_fast_cut_matches_reference_cut(dgs, oracle, name):
    build, strict = EQ_CASES[name]
    inputs = tuple(t.float().contiguous() for t in build())
    means, values, covs, conics, samples = inputs
    N, D, C = samples.shape[0], means.shape[1], values.shape[1]
    (m, v, c, s), fast, ref = _both_binnings(dgs, inputs)
    # R, ranges, sample ranges and radii: bit-identical
    assert fast[0] == ref[0]
    for i in (3, 4, 5):
        assert torch.equal(fast[i], ref[i])
    Ef, Er = dgs._C.binning_info(fast[1], fast[2])[1], dgs._C.binning_info(ref[1], ref[2])[1]
    print(f"{name}: fine entries {Ef} (fast cut) / {Er} (reference cut)")
    assert Ef <= Er
    if strict:
        assert Ef < Er
    # the lists the forward walks: no more candidates, and the SAME number of live pairs at the
    # fast paths' flush threshold (power >= -126 / log2 e): the fast cut dropped none of them
    q_ref, _, _, flush_below = _constants(dgs)
    (cand_f, live_f), (cand_r, live_r) = (dgs._C.count_pairs(m, c, s, b[1], b[2], flush_below / LOG2E) for b in (fast, ref))
    print(f"{name}: W_cand {cand_f} / {cand_r}, W_live at the flush threshold {live_f} / {live_r}")
    assert cand_f <= cand_r and live_f == live_r
    ob = oracle.OracleBins(means.numpy(), covs.numpy(), samples.numpy())
    dLs = [syn.grad_out(N, syn.out_components(f, D), C, seed=520 + i) for i, f in enumerate(FUNCS)]
    ds_abs = 0.0
    for f, dL in zip(FUNCS, dLs):
        bounds = order_bounds(ob, [f], values, conics, [dL])
        sums = abs_term_sums(ob, f, means.numpy(), values.numpy(), conics.numpy(), samples.numpy(), dL.numpy(),
                             q_ref + 1.0, device=DEV)
        bounds = {gname: regroup_bound(bounds[f"{f} forward" if gname == "forward" else gname], *sums[gname][::2])
                  for gname in ("forward", "dmeans", "dvalues", "dconics")}
        ds_abs = ds_abs + sums["dsamples"][0]
        res = []
        for R, gb, sb, rg, srg, _ in (fast, ref):
            out = getattr(dgs._C, FWD_NAME[f])(m, v, c, s, R, gb, sb, rg, srg, False)
            grads = getattr(dgs._C, FWD_NAME[f] + "_backward")(m, v, c, s, R, dL.to(DEV).reshape(out.shape), gb, sb,
                                                              rg, srg, False)
            res.append((out.cpu().numpy().reshape(N, -1, C), [g.cpu().numpy() for g in grads]))
        _agree(res[0][0], res[1][0], bounds["forward"], f"{name} {f} forward")
        for k, gname in enumerate(("dmeans", "dvalues", "dconics")):
            _agree(res[0][1][k], res[1][1][k], bounds[gname], f"{name} {f} {gname}")
    if name in SGRAD_CASES:
        codes = [sgr.FUNCS[f] for f in FUNCS]
        dl = [d.to(DEV) for d in dLs]
        got = [dgs._C.sample_gaussians_samples_backward(codes, m, v, c, s, dl, b[1], b[2], False).cpu().numpy()
               for b in (fast, ref)]
        bound = sgr.sample_grad_ref(ob, FUNCS, means.numpy(), values.numpy(), conics.numpy(), samples.numpy(),
                                    [d.numpy() for d in dLs])["bound"]
        # (D = 2, C = 1 is one fused launch; otherwise one call per function, added)
        bound = regroup_bound(bound, ds_abs, sums["dsamples"][2], calls=1 if (D == 2 and C == 1) else len(FUNCS))
        _agree(got[0], got[1], bound, f"{name} dsamples")


# ------------------------------------------------------------------------------ empty lists
def test_emptied_lists_give_exact_zeros(dgs):
    """One Gaussian (every cell list and sub list holds at most that entry) whose reference
    extent is just under 0.5: each cell the fast cut drops it from is left with an EMPTY list, and
    so are those cells' sub lists.  The samples beyond the fast cut get exactly 0 from every
    function, forward and sample-position gradient, and the backward that walks the emptied cell
    lists (k_backward / k_bwd_esum) returns exact zeros for a dL that lives only on those samples, and
    finite, non-zero gradients for a full one."""
    Q_REF, qf, _, _ = _constants(dgs)
    sig = 0.0343
    means = torch.tensor([[0.02, 0.02]])  # (a tile corner: the ring crosses four tiles)
    covs = torch.tensor([[sig ** 2, 0.0, sig ** 2]])
    conics = torch.tensor([[1 / sig ** 2, 0.0, 1 / sig ** 2]])
    values = torch.tensor([[1.5]])
    # (30011 samples: 4 x 4 fine cells per tile; up to 4001 a tile is one cell and no list differs)
    samples = syn.samples(30011, 2, seed=531)
    (m, v, c, s), fast, ref = _both_binnings(dgs, (means, values, covs, conics, samples))
    Ef, Er = dgs._C.binning_info(fast[1], fast[2])[1], dgs._C.binning_info(ref[1], ref[2])[1]
    print(f"one Gaussian: {Er} cells list it under the reference cut, {Ef} under the fast cut")
    assert 0 < Ef < Er, "the fast cut must empty some cell lists"
    X = means.double().numpy() - samples.double().numpy()
    cc = conics.double().numpy()[0]
    q = cc[0] * X[:, 0] ** 2 + 2 * cc[1] * X[:, 0] * X[:, 1] + cc[2] * X[:, 1] ** 2
    outside = q > qf + 0.5
    ring = outside & (q <= Q_REF)
    assert ring.sum() >= 20 and (~outside).sum() >= 20
    codes = [sgr.FUNCS[f] for f in FUNCS]
    for R, gb, sb, rg, srg, _ in (fast, ref):
        dls = []
        for f in FUNCS:
            out = getattr(dgs._C, FWD_NAME[f])(m, v, c, s, R, gb, sb, rg, srg, False)
            o = out.cpu().numpy().reshape(samples.shape[0], -1)
            assert not np.any(o[outside]), f
            assert np.any(o[~outside])
            dls.append(torch.ones_like(out))
            # a dL that is non-zero ONLY on the samples beyond the fast cut: every term carries G = 0
            dl0 = torch.zeros_like(out)
            dl0[torch.from_numpy(outside).to(DEV)] = 1.0
            bw = getattr(dgs._C, FWD_NAME[f] + "_backward")
            for g in bw(m, v, c, s, R, dl0, gb, sb, rg, srg, False):
                assert not np.any(g.cpu().numpy()), f
            full = [g.cpu().numpy() for g in bw(m, v, c, s, R, dls[-1], gb, sb, rg, srg, False)]
            assert all(np.all(np.isfinite(g)) for g in full) and np.any(full[1]), f
        ds = dgs._C.sample_gaussians_samples_backward(codes, m, v, c, s, dls, gb, sb, False).cpu().numpy()
        assert not np.any(ds[outside]) and np.any(ds[~outside])
