"""Non-finite upstream gradients and values stay inside the reference's pair set (DESIGN.md
section 6, tests/locality.py): what the oracle leaves untouched, the HIP path leaves untouched.

The black tiles' samples get a non-finite (or overflowing) dL, or the Gaussians that only black
tiles list get non-finite values.  On the rows the oracle provably leaves alone (pinned bit for bit
on the CPU by tests/test_locality_ref.py) the GPU result must be finite and within the project's
existing bound of the oracle's result for the ZEROED poison:
    |gpu - ref| <= 1e-5 |ref| + 1e-6 max|ref|   (max over the checked rows only: never looser than
                                                 test_gpu_parity.py's max over the whole array),
the thin case plus the a-priori exponent-order bound of those rows, the clustered case at
ATOL_BWD_CLUSTERED, the aggregation at test_gpu_aggregate.py's RTOL 1e-5 / ATOL 1e-5.
A kernel that handles a pair outside the pair set by multiplying with G = 0 passes every other
parity test (finite dL: the product is exactly 0) and fails here (0 * inf = NaN).
Means, conics, covariances and sample positions are never poisoned.
"""
import numpy as np
import pytest
import torch

import locality as loc
import sample_grad_ref as sgr
from cases import AGG_FEATURES
from helpers import FWD_NAME, close, close_grad
from locality import BADS

pytestmark = pytest.mark.gpu

RTOL, ATOL_FWD, ATOL_BWD = 1e-5, 1e-6, 1e-6  # SURVEY 8c (test_gpu_parity.py)
ATOL_BWD_CLUSTERED = 4e-6  # test_gpu_parity.py, DESIGN.md 6
DEV = "cuda:0"
GRADS = ("dmeans", "dvalues", "dconics")


def _bin(dgs, c, values=None):
    m, v, cv, cn, s = (t.to(DEV) for t in (c.means, c.values if values is None else values, c.covs, c.conics,
                                           c.samples))
    R, gb, sb, rg, srg, _ = dgs._C.preprocess_gaussians(m, v, cv, cn, s, False)
    assert R == c.ob.num_rendered
    return (m, v, cn, s), (R, gb, sb, rg, srg)


def _shape(c, function):
    return [c.N] + [c.D] * sgr.FUNCS[function] + [c.C]


def _backward(dgs, c, function, dL, values=None, step_means=None):
    (m, v, cn, s), (R, gb, sb, rg, srg) = _bin(dgs, c, values)
    if step_means is not None:  # in place, after the binning: the call-time path
        m.copy_(step_means.to(DEV))
        assert not dgs._C.inputs_match(m, cn, s, gb, sb)
    grads = getattr(dgs._C, FWD_NAME[function] + "_backward")(
        m, v, cn, s, R, dL.to(DEV).reshape(_shape(c, function)), gb, sb, rg, srg, False)
    return [g.cpu().numpy() for g in grads]


def _check_rows(got, exact, literal, rows, what, atol=ATOL_BWD, extra=None):
    """Every gradient finite and within the bound on `rows`; all failures reported together, the
    non-finite row counts first."""
    errors = []
    for k, name in enumerate(GRADS):
        g = got[k][rows]
        bad = ~np.isfinite(g).all(axis=1)
        print(f"{what} {name}: {int(bad.sum())} / {len(g)} checked rows non-finite")
        if bad.any():
            errors.append(f"{what} {name}: {int(bad.sum())} / {len(g)} checked rows are non-finite")
            continue
        try:
            close_grad(g, exact[k][rows], literal[k][rows], RTOL, atol, f"{what} {name}",
                       None if extra is None else extra[k][rows])
        except AssertionError as e:
            errors.append(" ".join(str(e).split())[:300])
    assert not errors, "\n".join(errors)


# ------------------------------------------------------------------------------ poisoned dL
@pytest.mark.parametrize("row", loc.DL_MATRIX, ids=loc.dl_id)
def test_poisoned_dl_leaves_clean_gaussians(dgs, oracle, row):
    """D = 2, C = 1: the packed-pair k_backward, the q-form and the moment form; C = 3, 5: the
    literal terms with scalar rows; gaussian at C = 16, 12, 20: k_backward_mx (padding channels,
    two channel blocks; constant-shift entries with seam_y, kUnsafe units with nonpd); laplacian
    at C = 16: the VALU backward at channel block 16; D = 1; thin: the slot sums of k_bwd_esum
    under the a-priori bound; mixed scales (duplicated samples, floor radii); clustered."""
    name, C, function, bad, ch = row
    c = loc.case(name, C)
    dL = c.dL(function)
    zeroed = loc.poison_dl(dL, c.poisoned, 0.0, channel=ch)
    got = _backward(dgs, c, function, loc.poison_dl(dL, c.poisoned, BADS[bad], channel=ch))
    _check_rows(got, c.backward(function, zeroed), c.backward(function, zeroed, exact=False), c.clean, loc.dl_id(row),
                atol=ATOL_BWD_CLUSTERED if name == "clustered" else ATOL_BWD,
                extra=c.order_bound(function, zeroed) if name == "thin" else None)
    if ch is not None:  # the other channels' dvalues of every Gaussian, at the full-array bound
        other = np.arange(C) != ch
        dv = got[1][:, other]
        assert np.isfinite(dv).all(), f"{int((~np.isfinite(dv)).any(axis=1).sum())} rows of dvalues[:, != {ch}] non-finite"
        close_grad(dv, c.backward(function, dL)[1][:, other], c.backward(function, dL, exact=False)[1][:, other],
                   RTOL, ATOL_BWD, f"{loc.dl_id(row)} dvalues of the other channels")


@pytest.mark.parametrize("functions", loc.FUSED, ids=lambda f: "+".join(x[:3] for x in f))
def test_poisoned_dl_fused_call(dgs, oracle, functions):
    """_C.sample_gaussians_multi_backward with every function's dL poisoned at the same samples;
    the reference is the sum of the per-function oracle gradients (test_gpu_multi.py)."""
    c = loc.case("base", 1)
    (m, v, cn, s), (R, gb, sb, _, _) = _bin(dgs, c)
    dLs = [c.dL(f, seed=213 + i) for i, f in enumerate(functions)]
    bad = [loc.poison_dl(d, c.poisoned, np.inf).to(DEV) for d in dLs]
    got = dgs._C.sample_gaussians_multi_backward([dgs.FUNCTIONS[f] for f in functions], m, v, cn, s, bad, gb, sb, False)
    zeroed = [loc.poison_dl(d, c.poisoned, 0.0) for d in dLs]
    exact = [sum(c.backward(f, z)[k] for f, z in zip(functions, zeroed)) for k in range(3)]
    lit = [sum(c.backward(f, z, exact=False)[k].astype(np.float64) for f, z in zip(functions, zeroed)) for k in range(3)]
    _check_rows([g.cpu().numpy() for g in got], exact, lit, c.clean, "fused " + "+".join(functions))


@pytest.mark.parametrize("function,C", loc.CALLTIME)
def test_poisoned_dl_call_time_path(dgs, oracle, function, C):
    """means.add_ after the binning (test_stale_binning_takes_the_call_time_path): the clean set
    is the BINNED oracle's, the reference its backward with the new means and the zeroed dL."""
    c = loc.case("base", C)
    m = loc.calltime_means(c)
    dL = c.dL(function)
    zeroed = loc.poison_dl(dL, c.poisoned, 0.0)
    got = _backward(dgs, c, function, loc.poison_dl(dL, c.poisoned, np.inf), step_means=m)
    _check_rows(got, c.backward(function, zeroed, means=m), c.backward(function, zeroed, means=m, exact=False),
                c.clean, f"call-time {function} C={C}")


def test_poisoned_loss_weights_through_autograd(dgs, oracle):
    """GaussianSampler, loss (out * w).sum() with w = inf on the poisoned samples (gaussian, C = 16)."""
    c = loc.case("base", 16)
    m, v, cv, cn, s = (t.to(DEV) for t in c.inputs)
    for t in (m, v, cn):
        t.requires_grad_(True)
    sampler = dgs.GaussianSampler(False)
    sampler.preprocess(m, v, cv, cn, s)
    out = sampler.sample_gaussians()
    dL = c.dL("gaussian")
    w = loc.poison_dl(dL, c.poisoned, np.inf).to(DEV).reshape(out.shape)
    (out * w).sum().backward()
    zeroed = loc.poison_dl(dL, c.poisoned, 0.0)
    _check_rows([t.grad.cpu().numpy() for t in (m, v, cn)], c.backward("gaussian", zeroed),
                c.backward("gaussian", zeroed, exact=False), c.clean, "autograd gaussian C=16")


# ------------------------------------------------------------------------------ poisoned values
def _check_white(out, ref, white, what):
    got = np.asarray(out).reshape(ref.shape)[white]
    n_bad = int((~np.isfinite(got)).reshape(len(got), -1).any(axis=1).sum())
    print(f"{what}: {n_bad} / {len(got)} white samples non-finite")
    assert n_bad == 0, f"{what}: {n_bad} / {len(got)} white samples are non-finite"
    close(got, ref[white], RTOL, ATOL_FWD, what)


@pytest.mark.parametrize("row", loc.VALUES_MATRIX, ids=lambda r: "-".join(str(x) for x in r))
def test_poisoned_values_leave_white_samples(dgs, oracle, row):
    """The only-black Gaussians' values non-finite: the forward at the white samples (C = 1:
    k_forward_s / _t; derivative C = 5: the lane-per-sample forward; C = 16: k_forward_mx) and
    the gradients of every Gaussian that is not only-black, against the unpoisoned oracle."""
    name, C, function, bad = row
    c = loc.case(name, C)
    pv = loc.poison_values(c.values, c.only_black, BADS[bad])
    (m, v, cn, s), (R, gb, sb, rg, srg) = _bin(dgs, c, pv)
    out = getattr(dgs._C, FWD_NAME[function])(m, v, cn, s, R, gb, sb, rg, srg, False)
    _check_white(out.cpu().numpy(), c.forward(function, loc.poison_values(c.values, c.only_black, 0.0)), c.white,
                 f"{function} forward, values {bad}")
    dL = c.dL(function)
    got = _backward(dgs, c, function, dL, values=pv)
    _check_rows(got, c.backward(function, dL), c.backward(function, dL, exact=False), ~c.only_black,
                f"{function} C={C} values {bad}")


def test_poisoned_values_fused_forward(dgs, oracle):
    c = loc.case("base", 1)
    functions = loc.FUSED[0]
    (m, v, cn, s), (R, gb, sb, _, _) = _bin(dgs, c, loc.poison_values(c.values, c.only_black, np.inf))
    outs = dgs._C.sample_gaussians_multi([dgs.FUNCTIONS[f] for f in functions], m, v, cn, s, gb, sb, False)
    zv = loc.poison_values(c.values, c.only_black, 0.0)
    for f, o in zip(functions, outs):
        _check_white(o.cpu().numpy(), c.forward(f, zv), c.white, f"fused {f} forward, values inf")


@pytest.mark.parametrize("name,C,functions", loc.SAMPLE_GRAD, ids=lambda v: str(v) if not isinstance(v, tuple) else "+".join(x[:3] for x in v))
def test_poisoned_values_sample_gradient(dgs, oracle, name, C, functions):
    """_C.sample_gaussians_samples_backward: dsamples at the white samples against sample_grad_ref
    with the poisoned values zeroed, at test_gpu_sample_grad.py's bound."""
    c = loc.case(name, C)
    dLs = [c.dL(f, seed=213 + i) for i, f in enumerate(functions)]
    (m, v, cn, s), (R, gb, sb, _, _) = _bin(dgs, c, loc.poison_values(c.values, c.only_black, np.inf))
    got = dgs._C.sample_gaussians_samples_backward([sgr.FUNCS[f] for f in functions], m, v, cn, s,
                                                   [d.to(DEV) for d in dLs], gb, sb, False).cpu().numpy()
    ref = sgr.sample_grad_ref(c.ob, functions, c.means.numpy(), loc.poison_values(c.values, c.only_black, 0.0).numpy(),
                              c.conics.numpy(), c.samples.numpy(), [d.numpy() for d in dLs])["dsamples"]
    _check_white(got, ref, c.white, f"{name} C={C} dsamples, values inf")


# ------------------------------------------------------------------------------ aggregation
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("transpose", ["1", "0"])
@pytest.mark.parametrize("D,L,K,bad", [s + ("inf",) for s in loc.AGG_SHAPES] + [loc.AGG_SHAPES[0] + ("nan",)])
def test_aggregation_poisoned_rows(dgs, oracle, monkeypatch, D, L, K, bad, transpose):
    """Rows 5::50 of the upstream gradient non-finite: d/dfeatures and d/dkeys of the Gaussians
    that are neither such a row nor a neighbour of one, and d/dqueries of every other row."""
    a = loc.agg_case(D, L, K)
    pre = dgs._C.preprocess_aggregate(_cuda(a["means"]), _cuda(a["conics"]), _cuda(a["radii"]), False)
    assert np.array_equal(pre[0].cpu().numpy(), a["pre"][0]), "indices"
    t = [_cuda(x) for x in a["args"]]
    fwd = dgs._C.aggregate_neighbors(*t, *pre, False)
    monkeypatch.setenv("DGS_AGG_TRANSPOSE", transpose)
    got = dgs._C.aggregate_neighbors_backward(*t, *pre[:4], *fwd[:3], pre[4], _cuda(loc.agg_poison(a, BADS[bad])), False)
    ref = loc.agg_ref(a, loc.agg_poison(a, 0.0))
    errors = []
    for k, rows in ((0, a["clean"]), (3, a["clean"]), (2, ~a["rows"])):
        g = got[k].cpu().numpy().reshape(ref[k].shape)[rows]
        n_bad = int((~np.isfinite(g)).any(axis=1).sum())
        print(f"d/d{AGG_FEATURES[k]}: {n_bad} / {len(g)} checked rows non-finite")
        if n_bad:
            errors.append(f"d/d{AGG_FEATURES[k]}: {n_bad} / {len(g)} checked rows are non-finite")
            continue
        try:
            close(g, ref[k][rows], 1e-5, 1e-5, f"d/d{AGG_FEATURES[k]}")
        except AssertionError as e:
            errors.append(" ".join(str(e).split())[:300])
    assert not errors, "\n".join(errors)
