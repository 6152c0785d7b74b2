"""The oracle side of the locality contract (tests/locality.py), on the CPU,
for every case tests/test_gpu_locality.py uses -- so that the GPU test can never pass by vacuity.

These are conditions on the cases, not measurements: a case that misses one is changed (scale,
seed, P), never the condition.  The bit-equality pins state what the GPU test relies on: with the
black tiles' dL (or the only-black Gaussians' values) non-finite, the oracle's results on the
clean rows (the white samples) are bit for bit those of the run with them zeroed.
"""
import numpy as np
import pytest

import locality as loc
from locality import BADS


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("name,C", loc.ALL_CASES, ids=lambda v: str(v))
def test_case_conditions(name, C):
    c = loc.case(name, C)
    n_clean = int(c.clean.sum())
    assert n_clean >= 0.10 * c.P, (n_clean, c.P)
    if c.D == 2:
        assert n_clean >= 100
    assert int(c.poisoned.sum()) >= 0.25 * c.N
    assert int(c.only_black.sum()) > 0 and int(c.white.sum()) > 0
    tr = loc.transitions(c.ob)
    assert any(cnt % 16 != 0 and n > 0 for cnt, _, n in tr), tr
    assert any(par == 1 for _, par, _ in tr), tr
    if name in ("seam_y", "nonpd"):
        assert int((c.clean & (c.kinds == name)).sum()) >= 1


def test_base_layout():
    """The layout the cases were chosen for (D = 2: 16 tiles, every white -> black transition
    after a partial 16-row step, three black tiles starting odd; D = 1: 4 tiles)."""
    c = loc.case("base", 1)
    assert (c.ob.T, int(c.poisoned.sum()), int(c.clean.sum()), int(c.only_black.sum())) == (16, 1961, 612, 615)
    tr = loc.transitions(c.ob)
    assert [t[0] for t in tr] == [9, 2, 2, 9, 3, 7, 1, 6] and sum(t[1] for t in tr) == 3
    assert all(90 <= t[2] <= 126 for t in tr)
    d = loc.case("d1", 1)
    assert (d.ob.T, int(d.clean.sum()), int(d.only_black.sum())) == (4, 205, 195)
    assert [t[:2] for t in loc.transitions(d.ob)] == [(15, 1), (7, 1)]


def _clean_rows_equal(a, b, rows, what):
    for name, x, y in zip(("dmeans", "dvalues", "dconics"), a, b):
        assert np.array_equal(x[rows], y[rows]), f"{what}: oracle {name} differs on the untouched rows"


@pytest.mark.parametrize("row", loc.DL_MATRIX, ids=loc.dl_id)
def test_oracle_poisoned_dl_leaves_clean_rows(row):
    name, C, function, bad, ch = row
    c = loc.case(name, C)
    dL = c.dL(function)
    zeroed = c.backward(function, loc.poison_dl(dL, c.poisoned, 0.0, channel=ch))
    got = c.backward(function, loc.poison_dl(dL, c.poisoned, BADS[bad], channel=ch))
    _clean_rows_equal(got, zeroed, c.clean, loc.dl_id(row))
    assert all(np.isfinite(z).all() for z in zeroed)
    nz = np.any(zeroed[0][c.clean] != 0, axis=1)
    assert nz.mean() >= 0.90, f"{nz.mean():.3f} of the clean rows have a non-zero dmeans"
    # (a clean Gaussian has no pair with a black sample at all: the unpoisoned run's gradient too)
    _clean_rows_equal(zeroed, c.backward(function, dL), c.clean, "zeroed vs unpoisoned")
    if ch is not None:  # one poisoned channel: the other channels' dvalues of EVERY Gaussian
        other = np.arange(C) != ch
        assert np.array_equal(got[1][:, other], c.backward(function, dL)[1][:, other])


@pytest.mark.parametrize("functions", loc.FUSED, ids=lambda f: "+".join(x[:3] for x in f))
def test_oracle_fused_reference(functions):
    """The fused call's reference is the sum of the per-function gradients: each term is pinned."""
    c = loc.case("base", 1)
    for i, f in enumerate(functions):
        dL = c.dL(f, seed=213 + i)
        _clean_rows_equal(c.backward(f, loc.poison_dl(dL, c.poisoned, np.inf)),
                          c.backward(f, loc.poison_dl(dL, c.poisoned, 0.0)), c.clean, f)


@pytest.mark.parametrize("function,C", loc.CALLTIME)
def test_oracle_calltime_means(function, C):
    c = loc.case("base", C)
    m = loc.calltime_means(c)
    dL = c.dL(function)
    _clean_rows_equal(c.backward(function, loc.poison_dl(dL, c.poisoned, np.inf), means=m),
                      c.backward(function, loc.poison_dl(dL, c.poisoned, 0.0), means=m), c.clean, "call-time means")


@pytest.mark.parametrize("row", loc.VALUES_MATRIX, ids=lambda r: "-".join(str(x) for x in r))
def test_oracle_poisoned_values_leave_white_samples(row):
    name, C, function, bad = row
    c = loc.case(name, C)
    zeroed = c.forward(function, loc.poison_values(c.values, c.only_black, 0.0))
    got = c.forward(function, loc.poison_values(c.values, c.only_black, BADS[bad]))
    assert np.array_equal(got[c.white], zeroed[c.white])
    assert np.isfinite(zeroed).all() and np.any(zeroed[c.white] != 0)
    dL = c.dL(function)
    keep = ~c.only_black
    _clean_rows_equal(c.backward(function, dL, values=loc.poison_values(c.values, c.only_black, BADS[bad])),
                      c.backward(function, dL), keep, "poisoned values")


@pytest.mark.parametrize("D,L,K", loc.AGG_SHAPES)
@pytest.mark.parametrize("bad", ["inf", "nan"])
def test_oracle_aggregation(D, L, K, bad):
    a = loc.agg_case(D, L, K)
    P = len(a["rows"])
    assert int(a["clean"].sum()) >= P / 4 and int(a["rows"].sum()) >= 8 and np.any(a["pre"][0] == -1)
    got = loc.agg_ref(a, loc.agg_poison(a, BADS[bad]))
    ref = loc.agg_ref(a, loc.agg_poison(a, 0.0))
    assert np.array_equal(got[0][a["clean"]], ref[0][a["clean"]]), "d/dfeatures"
    assert np.array_equal(got[3][a["clean"]], ref[3][a["clean"]]), "d/dkeys"
    assert np.array_equal(got[2][~a["rows"]], ref[2][~a["rows"]]), "d/dqueries"
    assert np.any(ref[0][a["clean"]] != 0) and np.any(ref[3][a["clean"]] != 0)
