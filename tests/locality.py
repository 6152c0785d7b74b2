"""Locality of non-finite data (not a test; no GPU, no torch.cuda): DESIGN.md section 6.

The reference forms a pair (Gaussian g, sample n) only if g is in the tile list of n's tile, and
within a tile it multiplies G * dL even where G underflows.  A non-finite dL[n] may therefore
reach every Gaussian of that tile's list and no other; a non-finite value of g every sample of
g's tiles and no other.  The GPU's pair set is a subset of the reference's, so the contract is
one-sided: what the oracle leaves untouched, the GPU must leave untouched.

The helpers colour the tiles by the reference's linear tile index (t & 1: black), so that
consecutive tiles of the sort order always differ in colour, poison the black tiles' samples (or
the values of the Gaussians that only black tiles list) and name the Gaussians / samples the
oracle provably leaves alone.  tests/test_locality_ref.py pins the oracle side of every case on
the CPU; tests/test_gpu_locality.py holds the HIP path to it.
"""
import numpy as np
import torch

import cases
from diff_gaussian_sampling import synthetic as syn

INF, NAN, HUGE = float("inf"), float("nan"), 3e38
BADS = {"inf": INF, "nan": NAN, "3e38": HUGE}


# ------------------------------------------------------------------------------ the colouring
def stripes(ob):
    """(black [T], poisoned [N], clean [P], only_black [P]) boolean masks of OracleBins `ob`:
    tile t is black if t & 1; poisoned samples are those whose key is a black tile (never
    rendered ones, key >= T, are left alone); clean Gaussians are in no black tile's list;
    only-black ones are in some black list and in no white one."""
    T = ob.T
    black = (np.arange(T) & 1).astype(bool)
    keys = ob.sample_keys()
    rendered = (keys >= 0) & (keys < T)
    poisoned = np.zeros(ob.N, bool)
    poisoned[rendered] = black[keys[rendered]]
    in_black, in_white = np.zeros(ob.P, bool), np.zeros(ob.P, bool)
    for t in range(T):
        (in_black if black[t] else in_white)[ob.tile_gaussians(t)] = True
    return black, poisoned, ~in_black, in_black & ~in_white


def transitions(ob):
    """For every white -> black pair of consecutive non-empty tiles of the sorted sample order:
    (the white tile's sample count mod 16, the parity of the black tile's first sorted index, the
    number of clean Gaussians in the white tile's list)."""
    black, _, clean, _ = stripes(ob)
    sr = ob.ranges()[1].astype(np.int64)
    tiles = [t for t in range(ob.T) if sr[t, 1] > sr[t, 0]]
    out = []
    for a, b in zip(tiles[:-1], tiles[1:]):
        if not black[a] and black[b]:
            out.append((int(sr[a, 1] - sr[a, 0]) % 16, int(sr[b, 0]) & 1, int(clean[ob.tile_gaussians(a)].sum())))
    return out


def poison_dl(dL, mask, bad, channel=None, component=None):
    """A copy of dL [N, K, C] with `bad` at the samples of `mask` (one channel / component, or all)."""
    out = dL.clone()
    rows = torch.from_numpy(np.nonzero(np.asarray(mask))[0])
    k = slice(None) if component is None else component
    c = slice(None) if channel is None else channel
    sub = out[rows]
    sub[:, k, c] = bad
    out[rows] = sub
    return out


def poison_values(values, mask, bad):
    """A copy of values [P, C] with `bad` in the rows of `mask`."""
    out = values.clone()
    out[torch.from_numpy(np.asarray(mask))] = bad
    return out


# ------------------------------------------------------------------------------ the cases
def _white_columns(samples):
    """x-intervals of the white tile columns (an even grid width: tile y * W + x is white iff x
    is even), from the reference's grid of these samples."""
    from oracle import oracle as orc
    grid, off = orc.tile_grid(samples.numpy())
    assert grid[0] % 2 == 0, "the seam-y Gaussians need an even grid width"
    return [(float(off[0]) + 0.51 * x, float(off[0]) + 0.51 * (x + 1)) for x in range(0, int(grid[0]), 2)]


def _seam_y(samples, C, P=200, seed=221):
    """Gaussians built like cases.seam_case's, hugging only the y edges (|y| within 0.02 of 1:
    constant-shift wraps onto the opposite edge's cells), x at least 0.08 (> their radius, at
    most 0.06) inside a white tile column: their tiles are the white columns' first and last rows."""
    g = torch.Generator().manual_seed(seed)
    cols = _white_columns(samples)
    pick = torch.randint(len(cols), (P,), generator=g)
    lo = torch.tensor([cols[i][0] for i in pick.tolist()]) + 0.08
    hi = torch.tensor([min(cols[i][1], float(samples[:, 0].max())) for i in pick.tolist()]) - 0.08
    x = lo + (hi - lo) * torch.rand(P, generator=g)
    side = torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0)
    y = side * (1.0 - 0.02 * torch.rand(P, generator=g))
    means = torch.stack([x, y], 1).float()
    sig = 0.004 + 0.01 * torch.rand(P, 1, generator=g)
    covs = torch.cat([sig ** 2, 0.3 * sig ** 2, 1.2 * sig ** 2], 1).float()
    det = covs[:, 0] * covs[:, 2] - covs[:, 1] ** 2
    conics = torch.stack([covs[:, 2] / det, -covs[:, 1] / det, covs[:, 0] / det], 1).float()
    return means, torch.randn(P, C, generator=g).float(), covs, conics


def _nonpd(C, P=40, seed=231):
    """Non-PD conics (c1 = 1.2 sqrt(c0 c2), c0, c2 in [4000, 8000]; covariances diag(1/c0, 1/c2),
    the reference reads them for the radius only): kUnsafe units, the literal power."""
    g = torch.Generator().manual_seed(seed)
    means = (torch.rand(P, 2, generator=g) * 2 - 1).float()
    c0 = 4000.0 + 4000.0 * torch.rand(P, generator=g)
    c2 = 4000.0 + 4000.0 * torch.rand(P, generator=g)
    conics = torch.stack([c0, 1.2 * torch.sqrt(c0 * c2), c2], 1).float()
    covs = torch.stack([1.0 / c0, torch.zeros(P), 1.0 / c2], 1).float()
    return means, torch.randn(P, C, generator=g).float(), covs, conics


def locality_case(D, C, extras=()):
    """The base field: 2000 Gaussians of scale 0.3 over 4000 samples at D = 2 (16 tiles), 400 of
    scale 0.1 over 3000 at D = 1 (4 tiles).  extras (D = 2): "seam_y", "nonpd" append the
    Gaussians of _seam_y / _nonpd.  Returns (means, values, covs, conics, samples, kinds): kinds
    [P] names each Gaussian's builder ("base", "seam_y", "nonpd")."""
    if D == 2:
        parts = [syn.gaussians(2000, 2, C, seed=211, scale=0.3)]
        samples = syn.samples(4000, 2, seed=212)
    else:
        assert not extras
        parts = [syn.gaussians(400, 1, C, seed=211, scale=0.1)]
        samples = syn.samples(3000, 1, seed=212)
    kinds = ["base"] * parts[0][0].shape[0]
    for e in extras:
        parts.append(_seam_y(samples, C) if e == "seam_y" else _nonpd(C))
        kinds += [e] * parts[-1][0].shape[0]
    means, values, covs, conics = (torch.cat([p[i] for p in parts]).contiguous() for i in range(4))
    return means, values, covs, conics, samples, np.array(kinds)


def _inputs(name, C):
    if name == "base":
        return locality_case(2, C)
    if name in ("seam_y", "nonpd"):
        return locality_case(2, C, extras=(name,))
    if name == "d1":
        return locality_case(1, C)
    if name == "thin":
        inp = cases.thin_case(P=1500, n=8000, C=C)
    elif name == "mixed":
        # scales from 1e-3 (cases.mixed_scales_case's own 1e-4 leaves a quarter of the Gaussians
        # without any sample in reach: zero gradients, nothing to compare); still under the radius floor
        inp = cases.mixed_scales_case(n=20000, C=C, decades=(-3.0, 1.7))
    elif name == "clustered":
        # x and y swapped: the blob (70 % of the samples) then lies in tile 9, a black one -- as
        # built it lies in tile 6 and only 15 % of the samples would be poisoned
        m, v, cv, c, s = cases.clustered_case(C=C)
        inp = (m[:, [1, 0]], v, cv[:, [2, 1, 0]], c[:, [2, 1, 0]], s[:, [1, 0]])
    else:
        raise KeyError(name)
    return inp + (np.array(["base"] * inp[0].shape[0]),)


class Case:
    """One case's inputs, oracle bins, masks and (cached, read-only) oracle references."""

    def __init__(self, name, C):
        from oracle import oracle as orc
        self.name, self.C = name, C
        *inp, self.kinds = _inputs(name, C)
        self.inputs = tuple(t.float().contiguous() for t in inp)
        self.means, self.values, self.covs, self.conics, self.samples = self.inputs
        self.P, self.D = self.means.shape
        self.N = self.samples.shape[0]
        self.ob = orc.OracleBins(self.means.numpy(), self.covs.numpy(), self.samples.numpy())
        self.black, self.poisoned, self.clean, self.only_black = stripes(self.ob)
        self.white = ~self.poisoned
        self._refs = {}

    def dL(self, function, seed=213):
        return syn.grad_out(self.N, syn.out_components(function, self.D), self.C, seed=seed)

    def backward(self, function, dL, values=None, means=None, exact=True):
        """The oracle's gradients (cached per argument bytes; do not modify the result)."""
        v = self.values if values is None else values
        key = ("b", function, dL.numpy().tobytes(), v.numpy().tobytes(),
               None if means is None else means.numpy().tobytes(), exact)
        if key not in self._refs:
            self._refs[key] = self.ob.backward(function, v.numpy(), self.conics.numpy(), dL.numpy(),
                                               means=None if means is None else means.numpy(), exact=exact)
        return self._refs[key]

    def forward(self, function, values=None):
        v = self.values if values is None else values
        key = ("f", function, v.numpy().tobytes())
        if key not in self._refs:
            self._refs[key] = self.ob.forward(function, v.numpy(), self.conics.numpy())
        return self._refs[key]

    def order_bound(self, function, dL):
        key = ("o", function, dL.numpy().tobytes())
        if key not in self._refs:
            self._refs[key] = self.ob.order_bound(function, self.values.numpy(), self.conics.numpy(), dL.numpy())
        return self._refs[key]


_cases = {}


def case(name, C):
    if (name, C) not in _cases:
        _cases[(name, C)] = Case(name, C)
    return _cases[(name, C)]


# The poisoned-dL matrix (tests/test_gpu_locality.py; every row pinned by test_locality_ref.py):
# (case, C, function, bad, poisoned channel or None).
DL_MATRIX = (
    [("base", 1, "gaussian", b, None) for b in ("inf", "nan", "3e38")]
    + [("base", 1, f, "inf", None) for f in ("derivative", "laplacian", "third")]
    + [("base", 3, "gaussian", "inf", None), ("base", 5, "derivative", "inf", None)]
    + [("base", 16, "gaussian", b, None) for b in ("inf", "nan", "3e38")]
    + [("base", 12, "gaussian", "inf", None), ("base", 20, "gaussian", "inf", None),
       ("base", 16, "laplacian", "inf", None),
       ("seam_y", 16, "gaussian", "inf", None), ("nonpd", 16, "gaussian", "inf", None),
       ("base", 16, "gaussian", "inf", 3), ("base", 20, "gaussian", "inf", 17),
       ("d1", 1, "gaussian", "inf", None), ("d1", 1, "third", "inf", None), ("d1", 5, "third", "inf", None),
       ("thin", 1, "gaussian", "inf", None), ("thin", 16, "gaussian", "inf", None),
       ("mixed", 1, "gaussian", "inf", None), ("clustered", 1, "gaussian", "inf", None)])
FUSED = (("gaussian", "derivative", "laplacian", "third"), ("gaussian", "laplacian"))
CALLTIME = (("derivative", 1), ("gaussian", 16))
# The poisoned-values matrix: (case, C, function, bad).
VALUES_MATRIX = (
    [("base", 1, f, "inf") for f in ("gaussian", "derivative", "laplacian", "third")]
    + [("base", 1, "gaussian", "nan"), ("base", 5, "derivative", "inf"), ("base", 16, "gaussian", "inf"),
       ("base", 16, "laplacian", "inf"), ("d1", 1, "gaussian", "inf")])
SAMPLE_GRAD = (("base", 1, ("gaussian", "derivative", "laplacian", "third")), ("d1", 3, ("third",)))
ALL_CASES = sorted({(n, C) for n, C, *_ in DL_MATRIX} | {(n, C) for n, C, *_ in VALUES_MATRIX}
                   | {("base", C) for _, C in CALLTIME} | {(n, C) for n, C, _ in SAMPLE_GRAD})


def dl_id(row):
    name, C, f, bad, ch = row
    return f"{name}-c{C}-{f}-{bad}" + (f"-ch{ch}" if ch is not None else "")


def calltime_means(c):
    """The binned means after a small in-place step (test_stale_binning_takes_the_call_time_path)."""
    step = torch.randn(c.P, c.D, generator=torch.Generator().manual_seed(7)) * (0.5 * 2.0 / c.P ** (1.0 / c.D))
    return (c.means + step.float()).contiguous()


# ------------------------------------------------------------------------------ the aggregation
AGG_SHAPES = ((2, 16, 16), (2, 6, 5), (2, 40, 20), (1, 8, 4))
_agg = {}


def agg_case(D, L, K):
    """The aggregation problem, the poisoned rows (5::50 of the upstream gradient), the clean
    Gaussians (neither a poisoned row nor a neighbour of one) and the oracle's lists / forward."""
    if (D, L, K) not in _agg:
        from oracle import oracle as orc
        P = 1200
        means, conics, radii, fe = cases.agg_problem(P=P, D=D, L=L, K=K, F=4, seed=110 + L, spread=1.0,
                                                     radius=(0.1, 0.3) if D == 2 else (0.02, 0.08))
        if D == 1:  # (agg_problem's non-PD conic is D = 2 only: power > 0 slots, index -1)
            conics[5] = -3.0
        pre = orc.agg_preprocess(means, conics, radii)
        idx, rg = pre[0], pre[1]
        rows = np.zeros(P, bool)
        rows[5::50] = True
        row_of = np.repeat(np.arange(P), np.diff(np.concatenate([[0], rg])))
        touched = rows.copy()
        nb = idx[rows[row_of] & (idx >= 0)]
        touched[nb] = True
        args = [fe[k] for k in cases.AGG_FEATURES]
        w, e, f, _ = orc.agg_forward(*args, *pre)
        g = np.random.default_rng(7).normal(size=(P, L)).astype(np.float32)
        _agg[(D, L, K)] = dict(means=means, conics=conics, radii=radii, fe=fe, args=args, pre=pre, fwd=(w, e, f),
                               rows=rows, clean=~touched, g=g, refs={})
    return _agg[(D, L, K)]


def agg_ref(a, g):
    """oracle.agg_backward(exact=True) of upstream gradient g (cached; read-only)."""
    from oracle import oracle as orc
    key = g.tobytes()
    if key not in a["refs"]:
        idx, rg, X, dn, inv = a["pre"]
        a["refs"][key] = orc.agg_backward(*a["args"], idx, rg, X, dn, *a["fwd"], inv, g, exact=True)
    return a["refs"][key]


def agg_poison(a, bad):
    g = a["g"].copy()
    g[a["rows"]] = bad
    return g
