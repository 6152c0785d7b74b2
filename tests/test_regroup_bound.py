"""Pins tests/regroup_bound.py on the CPU: the per-pair terms whose magnitudes it sums are the
oracle's -- their SIGNED sums equal the oracle's forward, its exact backward and
sample_grad_ref's sample-position gradient -- so sum |term| is the quantity the bound's
derivation speaks of."""
import numpy as np
import pytest

import sample_grad_ref as sgr
from diff_gaussian_sampling import synthetic as syn
from helpers import FUNCS
from regroup_bound import abs_term_sums, regroup_bound

CASES = {"d2_c3": (120, 2, 3, 400), "d1_c2": (60, 1, 2, 300)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, oracle):
    P, D, C, N = CASES[request.param]
    means, values, covs, conics = (t.float().contiguous() for t in syn.gaussians(P, D, C, seed=601))
    samples = syn.samples(N, D, seed=602).float().contiguous()
    ob = oracle.OracleBins(means.numpy(), covs.numpy(), samples.numpy())
    return ob, means, values, conics, samples


@pytest.mark.parametrize("f", FUNCS)
def test_signed_sums_are_the_oracles(case, f):
    ob, means, values, conics, samples = case
    N, D, C = samples.shape[0], means.shape[1], values.shape[1]
    dL = syn.grad_out(N, syn.out_components(f, D), C, seed=603)
    sums = abs_term_sums(ob, f, means.numpy(), values.numpy(), conics.numpy(), samples.numpy(), dL.numpy(), 211.0)
    ref = {"forward": ob.forward(f, values.numpy(), conics.numpy())}
    ref.update(zip(("dmeans", "dvalues", "dconics"),
                   ob.backward(f, values.numpy(), conics.numpy(), dL.numpy(), exact=True)))
    ref["dsamples"] = sgr.sample_grad_ref(ob, [f], means.numpy(), values.numpy(), conics.numpy(), samples.numpy(),
                                          [dL.numpy()])["dsamples"]
    for name, (abs_sum, signed, n) in sums.items():
        r = np.asarray(ref[name], np.float64).reshape(signed.shape)
        assert np.any(r != 0) and np.all(n >= 0) and n.max() >= 1
        # the oracle's terms are float32: a few ulp of each term (the exponent's rounding grows with q / 2 <= 105)
        assert np.all(np.abs(signed - r) <= 1e-4 * abs_sum + 1e-30), name
        assert np.all(np.abs(signed) <= abs_sum * (1 + 1e-12) + 1e-300), name


def test_regroup_bound_formula():
    B, s, n = np.array([0.0, 1e-9]), np.array([2.0, 3.0]), np.array([[10.0], [0.0]])[:, 0]
    got = regroup_bound(B, s, n, calls=4)
    assert np.allclose(got, [2 * 10 * 4 * 2.0 ** -24 * 2.0, 1e-9], rtol=1e-12, atol=0)
