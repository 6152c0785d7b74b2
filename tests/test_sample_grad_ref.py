"""Pins tests/sample_grad_ref.py (the float64 reference of dL/dsamples) on the CPU, on every
case the GPU tests use: its forward against the oracle's, its autograd dmeans against the
oracle's exact backward, translation invariance, and its closed form against its autograd."""
import numpy as np
import pytest

import sample_grad_ref as sgr
from helpers import close

RTOL, ATOL = 1e-5, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _built(oracle):
    return oracle


@pytest.mark.parametrize("name", sgr.CASE_NAMES)
def test_helper_matches_the_oracle(name):
    functions, (means, values, covs, conics, samples), dLs, ob, ref = sgr.case(name)
    dm, bm = None, None
    thin = name == "thin"  # thin Gaussians: the project's stated bound is 8c + the oracle's a-priori
    # exponent-order bound (tests/helpers.py) -- the oracle's own float32 exponent is
    # one of the orders that bound covers, and no thin case is within plain 8c of float64
    for f, dL in zip(functions, dLs):
        fb = ob.order_bound(f, values.numpy(), conics.numpy()) if thin else None
        close(ref["outs"][f], ob.forward(f, values.numpy(), conics.numpy()), RTOL, ATOL, f"{name}: {f} forward", fb)
        g = ob.backward(f, values.numpy(), conics.numpy(), dL.numpy(), exact=True)[0]
        dm = g if dm is None else dm + g
        if thin:
            b = ob.order_bound(f, values.numpy(), conics.numpy(), dL.numpy())[0]
            bm = b if bm is None else bm + b
    close(ref["dmeans"], dm, RTOL, ATOL, f"{name}: dmeans", bm)


@pytest.mark.parametrize("name", sgr.CASE_NAMES)
def test_translation_invariance(name):
    ref = sgr.case(name)[4]
    a, b = ref["dsamples"].sum(0), -ref["dmeans"].sum(0)
    scale = np.abs(ref["dsamples"]).sum(0) + np.abs(ref["dmeans"]).sum(0)
    assert np.all(np.abs(a - b) <= 1e-10 * scale), (a, b)


@pytest.mark.parametrize("name", sgr.CASE_NAMES)
def test_closed_form_equals_autograd(name):
    """G (phi a - A g), the form the kernels evaluate, against float64 autograd."""
    ref = sgr.case(name)[4]
    close(ref["closed"], ref["dsamples"], 1e-9, 1e-12, f"{name}: closed form")


def test_outside_samples_and_duplicates():
    ref = sgr.case("aliasing")
    keys = ref[3].sample_keys()
    outside = (keys < 0) | (keys >= ref[3].T)
    assert outside.any() and not np.any(ref[4]["dsamples"][outside])
    d = sgr.case("duplicates")[4]["dsamples"]
    assert np.array_equal(d[:500], d[500:])
