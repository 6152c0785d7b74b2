"""Reference of open (non-periodic) axes of a D = 3 field (dgs_volume_preprocess_axes; not a test).

    with open_axes(periodic):   # a mask in 0..7, bit d set = axis d periodic
        ...                     # any reference call

replaces `oracle.volume._wrap` for its duration and restores it in `finally`: the replacement is the
original on the periodic axes and the identity on the open ones, X_d = fl(m_d - s_d).  Everything
that forms a pair reaches `_wrap` through the module at call time (`oracle.volume._pairs`, and
`volume_sample_grad_ref.torch_forward`), so `oracle.volume.forward` / `backward`,
`volume_sample_grad_ref.dsamples` and `torch_forward`, `volume_trace_ref` and `volume_linop_ref` are
the references of any mask as they stand; nothing else of a pair depends on the axes (the power, the
skips, a = A X and the terms follow X).

`OpenCase(case, periodic)` holds the references of one field (a `test_gpu_volume_multi.Case`) under
one mask, for the function codes 0..5 (4: the trace, 5: the operator with `coef`), each computed
once on first use and left unchanged; it shares the field's arrays and its upstream gradients.
"""
import contextlib

import numpy as np

import volume_linop_ref as lr
import volume_sample_grad_ref as vr
import volume_trace_ref as tr
from oracle import volume as vo

TRACE, OP = 4, 5


def mask_of(periodic):
    """the mask of a bool or three bools (as `preprocess_volume` takes them), or of a mask"""
    if isinstance(periodic, bool):
        return 7 if periodic else 0
    if isinstance(periodic, (tuple, list)):
        return sum(1 << d for d in range(3) if periodic[d])
    return int(periodic)


@contextlib.contextmanager
def open_axes(periodic):
    periodic = mask_of(periodic)
    assert 0 <= periodic <= 7
    orig = vo._wrap

    def wrap(x):
        y = orig(x)
        for d in range(3):
            if not (periodic >> d) & 1:
                y[..., d] = x[..., d]
        return y

    vo._wrap = wrap
    try:
        yield
    finally:
        vo._wrap = orig


class OpenCase:
    """The references of `case`'s field with the axes `periodic`."""

    def __init__(self, case, periodic, coef=lr.SETS["balanced"]):
        self.means, self.values, self.conics, self.samples = case.means, case.values, case.conics, case.samples
        self.N, self.C, self.periodic = case.N, case.C, mask_of(periodic)
        self.coef = [float(x) for x in np.asarray(coef, np.float32)]
        # the trace's and the operator's upstream gradients of tests/test_gpu_volume_trace.py / _linop.py
        rng = np.random.default_rng(7 + TRACE)
        self.dL = list(case.dL[:4]) + [(rng.normal(size=(self.N, self.C)) * 0.01 ** 2).astype(np.float32),
                                       lr.op_dL(self.N, self.C)]
        self.dev = case.dev
        self._cache = {}

    def _args(self):
        return self.means, self.values, self.conics, self.samples

    def _get(self, kind, f, make):
        if (kind, f) not in self._cache:
            with open_axes(self.periodic):
                r = make()
            for a in (r if isinstance(r, tuple) else (r,)):
                a.setflags(write=False)
            self._cache[(kind, f)] = r
        return self._cache[(kind, f)]

    def fwd(self, f):
        """[N, K, C]; K = 1 for the trace and the operator"""
        if f == TRACE:
            return self._get("fwd", f, lambda: tr.forward(*self._args())[:, None, :])
        if f == OP:
            return self._get("fwd", f, lambda: lr.forward(self.coef, *self._args())[:, None, :])
        return self._get("fwd", f, lambda: vo.forward(f, *self._args()))

    def bwd(self, f):
        if f == TRACE:
            return self._get("bwd", f, lambda: tuple(tr.backward(*self._args(), self.dL[f])))
        if f == OP:
            return self._get("bwd", f, lambda: tuple(lr.backward(self.coef, *self._args(), self.dL[f])))
        return self._get("bwd", f, lambda: tuple(vo.backward(f, *self._args(), self.dL[f])))

    def sref(self, f):
        if f == TRACE:
            return self._get("sg", f, lambda: tr.dsamples(*self._args(), self.dL[f]))
        if f == OP:
            return self._get("sg", f, lambda: lr.dsamples(self.coef, *self._args(), self.dL[f]))
        return self._get("sg", f, lambda: vr.dsamples(f, *self._args(), self.dL[f]))

    def live_pairs(self, samples_of_last=False):
        """(sure, last): the pairs whose exact G = exp(power) is at least the smallest float32 subnormal
        2^-149, and those with 2^-150 < G < 2^-149, where a float32 G > 0 is the exponential's last
        rounding: numpy rounds them up to 2^-149, an exponential that truncates returns 0.  Their sum is
        the oracle's count of pairs with G > 0 (asserted); power in float32 as `oracle.volume._pairs`
        forms it.  samples_of_last: also the indices of the samples that have a pair among `last`."""
        f = np.float32
        sure = last = ref = 0
        which = []
        lo, hi = -150 * np.log(2.0), -149 * np.log(2.0)
        with open_axes(self.periodic):
            for s0 in range(0, self.N, 512):
                s = self.samples[s0:s0 + 512]
                X = vo._wrap(self.means[:, None, :].astype(f) - s[None, :, :].astype(f))
                c = [self.conics[:, q].astype(f)[:, None] for q in range(6)]
                X0, X1, X2 = X[..., 0], X[..., 1], X[..., 2]
                qd = c[0] * X0 * X0 + c[3] * X1 * X1 + c[5] * X2 * X2
                qo = c[1] * X0 * X1 + c[2] * X0 * X2 + c[4] * X1 * X2
                power = (f(-0.5) * qd - qo).astype(np.float64)
                band = (power < hi) & (power > lo)
                sure += int(((power <= 0) & (power >= hi)).sum())
                last += int(band.sum())
                which += [s0 + int(j) for j in np.nonzero(band.any(0))[0]]
                ref += int((vo._pairs(self.means, self.conics, s)[1] > 0).sum())
        assert sure + last == ref, (sure, last, ref)
        return (sure, last, which) if samples_of_last else (sure, last)
