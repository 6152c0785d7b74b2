"""D = 3 Gaussian fields -- beyond the reference.

The reference stops at D = 2: its device functions have no D = 3 branch
(cuda_sampler/forward.cu:164-275, backward.cu:108-416), its radius is 0 there
(forward.cu:52-61) and its sample keys are uninitialised (sampler_impl.cu:177-182), so
`GaussianSampler` renders nothing at D = 3 and this package's reference API rejects it.
`VolumeSampler` carries the reference's per-pair arithmetic to three dimensions
(include/dgs_volume.h): the per-axis torus wrap of forward.cu:149-157, the
power with conics packed [c00 c01 c02 c11 c12 c22], and the four functions in index form
(gaussian v G, derivative v G a, laplacian v G (a a^T - A), third
v G (A_ij a_k + A_ik a_j + A_jk a_i - a_i a_j a_k)), summed over every Gaussian (no tile
truncation; only pairs whose contribution is exactly 0 in fp32 are skipped).

Outputs are [N, 3, ..., 3, C] (3^k components for the k-th derivative), gradients flow to
means [P, 3], values [P, C] and conics [P, 6] through autograd, as in the reference's
Functions (diff_gaussian_sampling/__init__.py:80-160 of the reference).

The gradient with respect to the sample positions [N, 3] (moving or learned collocation points,
advected tracers, a learned warp in front of the sampler) is opt-in:
`VolumeSampler(debug, sample_grad=True)`, or `sample_grad=True` on `sample_volume` /
`sample_volume_multi`.  It costs a third walk of the candidates, about a forward's time, on top
of the forward and the backward, and nobody should pay that because a tensor happens to carry
requires_grad: without the flag, samples that require a gradient raise NotImplementedError as
before.  With it, `samples.grad` is filled (the pair set held fixed, the wrap with slope 1, as
for the other gradients), and the gradients of means, values and conics are bit for bit what they
are without it.

The wrap is a choice per axis (`periodic=` of `preprocess_volume` and `VolumeSampler`; DESIGN.md
§4.8, "Open axes"): by default every axis is periodic with period 2; on an open axis X_d is the
plain difference mean_d - sample_d and only the direct image exists, which is what a time axis or an
axis with walls needs.  The choice is fixed at binning time and stored in the binning, so
`sample_volume` and `sample_volume_multi` follow it with no argument of their own.
"""
import torch

from . import _C, call_debug

FUNCTION_CODES = {"gaussian": 0, "derivative": 1, "laplacian": 2, "third": 3, "laplacian_trace": 4}
TRACE = FUNCTION_CODES["laplacian_trace"]
OPERATOR = 5  # a LinearOperator instance in place of a name (DGS_VOLUME_FN_OPERATOR)


class LinearOperator:
    """A constant-coefficient linear operator of a D = 3 field,

        L u = c0 u + sum_i b_i d_i u + sum_ij W_ij d_ij u,

    sampled as ONE output [N, C] ("Linear operator"): a heat residual
    LinearOperator(b=(0, 0, 1), W=LinearOperator.laplacian((0, 1), -kappa).W) of a field over
    (x, y, t), a wave operator, anisotropic diffusion div(K grad u), Helmholtz.  An instance goes
    wherever a function name does (`sample_volume`, `sample_volume_multi`,
    `VolumeSampler.sample_gaussians_multi`, `VolumeSampler.sample_gaussians_operator`).  By
    definition the output is c0 * gaussian + (b * derivative).sum + (W * laplacian).sum of this
    package's outputs, with their sign conventions, at about the gaussian's cost.

    `b` is three numbers; `W` a 3 x 3 nested sequence or tensor, symmetrised as (W + W^T) / 2, or six
    packed numbers [w00, w01, w02, w11, w12, w22] (entries of the symmetric W).  The coefficients are
    constants: they are kept as ten Python floats rounded to float32 (`coef`: c0, b, packed W) and
    get no gradient; learnable coefficients combine the outputs of `sample_gaussians_multi`."""

    def __init__(self, c0=0.0, b=None, W=None):
        for x in (c0, b, W):
            if isinstance(x, torch.Tensor) and x.requires_grad:
                raise ValueError("LinearOperator takes constants: a coefficient tensor that requires a gradient is "
                                 "not supported; combine the outputs of sample_gaussians_multi(\"gaussian\", "
                                 "\"derivative\", \"laplacian\") instead")
        c0 = torch.as_tensor(c0, dtype=torch.float64).reshape(())
        b = torch.zeros(3, dtype=torch.float64) if b is None else torch.as_tensor(b, dtype=torch.float64).cpu()
        W = torch.zeros(6, dtype=torch.float64) if W is None else torch.as_tensor(W, dtype=torch.float64).cpu()
        if b.shape != (3,):
            raise ValueError("LinearOperator: b is three numbers")
        if W.shape == (3, 3):
            W = (W + W.T) / 2
            W = torch.stack([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]])
        elif W.shape != (6,):
            raise ValueError("LinearOperator: W is 3 x 3 or six packed numbers [w00, w01, w02, w11, w12, w22]")
        coef = torch.cat([c0.cpu().reshape(1), b, W]).to(torch.float32)
        if not bool(torch.isfinite(coef).all()):
            raise ValueError("LinearOperator: the coefficients must be finite")
        self.coef = [float(x) for x in coef.tolist()]

    @property
    def c0(self):
        return self.coef[0]

    @property
    def b(self):
        return tuple(self.coef[1:4])

    @property
    def W(self):
        w = self.coef[4:]
        return ((w[0], w[1], w[2]), (w[1], w[3], w[4]), (w[2], w[4], w[5]))

    @classmethod
    def laplacian(cls, axes=(0, 1, 2), scale=1.0):
        """scale * sum of d_ii u over `axes` (axes=(0, 1): the space Laplacian of an (x, y, t) field)."""
        return cls.diagonal(*[scale if i in axes else 0.0 for i in range(3)])

    @classmethod
    def diagonal(cls, w0, w1, w2):
        """w0 d_00 u + w1 d_11 u + w2 d_22 u"""
        return cls(W=[w0, 0.0, 0.0, w1, 0.0, w2])

    def __repr__(self):
        return f"LinearOperator(c0={self.c0}, b={self.b}, W={self.W})"


class _Codes(tuple):
    """The function codes of a call; `coef` holds the operator's coefficients when code 5 is among them."""
    coef = None


def _coef(codes):
    return getattr(codes, "coef", None)  # (a plain tuple of codes holds no operator)


def _parse(functions):
    codes, coef = [], None
    for f in functions:
        if isinstance(f, LinearOperator):
            if coef is not None:
                raise ValueError("one LinearOperator per call (their coefficients are the call's); "
                                 "sample the second one in a call of its own")
            codes.append(OPERATOR)
            coef = f.coef
        else:
            codes.append(FUNCTION_CODES[f] if isinstance(f, str) else int(f))
            if codes[-1] == OPERATOR:
                raise ValueError("function 5 is given as a LinearOperator instance")
    codes = _Codes(codes)
    codes.coef = coef
    return codes


def _multi_calls(codes, coef=None):
    """The forward, backward and sample-gradient bindings of a list of codes: the _linop ones
    (dgs_volume_*_linop, with the coefficients) only when the operator is among them, the _ops ones
    (dgs_volume_*_ops, five functions) only when the trace is, else the ones every call without
    either has always taken."""
    if OPERATOR in codes:
        return tuple((lambda cs, *a, _f=f: _f(cs, coef, *a)) for f in
                     (_C.volume_forward_linop, _C.volume_backward_linop, _C.volume_samples_backward_linop))
    if TRACE in codes:
        return _C.volume_forward_ops, _C.volume_backward_ops, _C.volume_samples_backward_ops
    return _C.volume_forward_multi, _C.volume_backward_multi, _C.volume_samples_backward


def _axes(periodic):
    """`periodic` as a tuple of three bools (axis 0, 1, 2): a bool for all three, or three bools."""
    if isinstance(periodic, bool):
        return (periodic,) * 3
    if isinstance(periodic, (tuple, list)) and len(periodic) == 3 and all(isinstance(p, bool) for p in periodic):
        return tuple(periodic)
    raise ValueError(f"periodic is a bool or three bools for (axis 0, axis 1, axis 2), not {periodic!r}")


def preprocess_volume(means, conics, samples, debug=False, periodic=True):
    """Cell binning of a D = 3 field; returns the opaque uint8 buffer.  `periodic`: a bool, or three
    bools for (axis 0, 1, 2); False makes an axis open (no wrap, only the direct image: a time axis,
    an axis with walls).  The binning carries the axes: every call on it follows them."""
    axes = _axes(periodic)
    if all(axes):  # the default: the call it has always been
        return call_debug(_C.volume_preprocess, debug, "vol_preprocess", means, conics, samples, debug)
    mask = sum(1 << d for d in range(3) if axes[d])
    return call_debug(_C.volume_preprocess_axes, debug, "vol_preprocess", means, conics, samples, mask, debug)


class _SampleVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, function, means, values, conics, samples, binning, debug):
        if ctx.needs_input_grad[4]:  # (the sample-position gradient is D = 1 / 2 only: DESIGN.md 4.9)
            raise NotImplementedError("VolumeSampler returns no gradient for samples; detach them "
                                      "(or ask for it: sample_grad=True)")
        out = call_debug(_C.volume_forward, debug, "vol_fw", function, means, values, conics, samples,
                         binning, debug)
        ctx.function, ctx.debug = function, debug
        ctx.save_for_backward(means, values, conics, samples, binning)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        means, values, conics, samples, binning = ctx.saved_tensors
        gm, gv, gc = call_debug(_C.volume_backward, ctx.debug, "vol_bw", ctx.function, means, values,
                                conics, samples, binning, grad_out.contiguous(), ctx.debug)
        return None, gm, gv, gc, None, None, None


class _SampleVolumeSG(torch.autograd.Function):
    """_SampleVolume with the sample-position gradient (sample_grad=True): the same _C calls for
    the output and the parameters' gradients, plus _C.volume_samples_backward when samples need one."""

    @staticmethod
    def forward(ctx, function, means, values, conics, samples, binning, debug):
        out = call_debug(_C.volume_forward, debug, "vol_fw", function, means, values, conics, samples,
                         binning, debug)
        ctx.function, ctx.debug = function, debug
        ctx.save_for_backward(means, values, conics, samples, binning)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        means, values, conics, samples, binning = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        gm = gv = gc = gs = None
        if any(ctx.needs_input_grad[1:4]):
            gm, gv, gc = call_debug(_C.volume_backward, ctx.debug, "vol_bw", ctx.function, means, values,
                                    conics, samples, binning, grad_out, ctx.debug)
        if ctx.needs_input_grad[4]:
            gs = call_debug(_C.volume_samples_backward, ctx.debug, "vol_sg", [ctx.function], means, values,
                            conics, samples, [grad_out], binning, ctx.debug)
        return None, gm, gv, gc, gs, None, None


def sample_volume(function, means, values, conics, samples, binning, debug=False, sample_grad=False):
    """One of the five functions ("gaussian", "derivative", "laplacian", "third",
    "laplacian_trace" or 0..4) of a D = 3 field at `samples`, through the binning of
    preprocess_volume.  "laplacian_trace" is the trace of the laplacian, [N, C]: what a diffusion,
    Poisson, wave or Navier-Stokes residual uses of the [N, 3, 3, C] Hessian, at about the
    gaussian's cost ("Trace Laplacian").  sample_grad=True also
    returns the gradient of `samples` when they require one (one more walk of the candidates, about
    a forward's time; without the flag such samples raise NotImplementedError).  A LinearOperator
    instance in place of the name samples that operator, [N, C]."""
    if isinstance(function, LinearOperator):
        return sample_volume_multi((function,), means, values, conics, samples, binning, debug, sample_grad)[0]
    code = FUNCTION_CODES[function] if isinstance(function, str) else int(function)
    if code == TRACE:  # (the per-function bindings keep refusing it: the _ops ones take it)
        return sample_volume_multi((code,), means, values, conics, samples, binning, debug, sample_grad)[0]
    fn = _SampleVolumeSG if sample_grad else _SampleVolume
    return fn.apply(code, means, values, conics, samples, binning, debug)


class _SampleVolumeMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, codes, means, values, conics, samples, binning, debug):
        if ctx.needs_input_grad[4]:
            raise NotImplementedError("VolumeSampler returns no gradient for samples; detach them "
                                      "(or ask for it: sample_grad=True)")
        outs = call_debug(_multi_calls(codes, _coef(codes))[0], debug, "vol_multi_fw", list(codes), means, values, conics,
                          samples, binning, debug)
        ctx.codes, ctx.debug = codes, debug
        ctx.save_for_backward(means, values, conics, samples, binning)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        means, values, conics, samples, binning = ctx.saved_tensors
        live = [(c, g.contiguous()) for c, g in zip(ctx.codes, grads) if g is not None]
        if not live:
            return (None,) * 7
        live_codes = [c for c, _ in live]
        gm, gv, gc = call_debug(_multi_calls(live_codes, _coef(ctx.codes))[1], ctx.debug, "vol_multi_bw", live_codes,
                                means, values, conics, samples, [g for _, g in live], binning, ctx.debug)
        return None, gm, gv, gc, None, None, None


class _SampleVolumeMultiSG(torch.autograd.Function):
    """_SampleVolumeMulti with the sample-position gradient (sample_grad=True), over the live
    outputs only."""

    @staticmethod
    def forward(ctx, codes, means, values, conics, samples, binning, debug):
        outs = call_debug(_multi_calls(codes, _coef(codes))[0], debug, "vol_multi_fw", list(codes), means, values, conics,
                          samples, binning, debug)
        ctx.codes, ctx.debug = codes, debug
        ctx.save_for_backward(means, values, conics, samples, binning)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        means, values, conics, samples, binning = ctx.saved_tensors
        live = [(c, g.contiguous()) for c, g in zip(ctx.codes, grads) if g is not None]
        if not live:
            return (None,) * 7
        gm = gv = gc = gs = None
        live_codes = [c for c, _ in live]
        _, bwd, sgrad = _multi_calls(live_codes, _coef(ctx.codes))
        if any(ctx.needs_input_grad[1:4]):
            gm, gv, gc = call_debug(bwd, ctx.debug, "vol_multi_bw", live_codes,
                                    means, values, conics, samples, [g for _, g in live], binning, ctx.debug)
        if ctx.needs_input_grad[4]:
            gs = call_debug(sgrad, ctx.debug, "vol_multi_sg", live_codes, means,
                            values, conics, samples, [g for _, g in live], binning, ctx.debug)
        return None, gm, gv, gc, gs, None, None


def sample_volume_multi(functions, means, values, conics, samples, binning, debug=False, sample_grad=False):
    """Several of the five functions (distinct names or codes) of a D = 3 field at `samples`;
    returns their outputs in the order asked.  With "laplacian_trace" among them the call goes
    through dgs_volume_*_ops; asked together with "laplacian", the trace runs as its own call
    beside the fused rest.  Up to C = 4 (a velocity field, velocity and pressure)
    they share one walk of the candidates, forward and backward (include/dgs_volume.h,
    dgs_volume_*_multi at C = 1, dgs_volume_*_fused at C = 2..4); with more channels the
    per-function kernels run in turn and their gradients are added.  Each output is bitwise the one
    `sample_volume` returns.  An output whose gradient is None is left out of the backward.
    sample_grad=True: as for `sample_volume`, the gradient of `samples` over the live outputs (one
    walk up to C = 4, the per-function calls added above).

    One of `functions` may be a LinearOperator (dgs_volume_*_linop): with "gaussian" and / or
    "derivative" up to C = 4 it shares their walk (what a Burgers-type residual needs: u, grad u and
    u_t - nu u_xx); asked together with "laplacian", "third" or "laplacian_trace" it runs as its own
    call beside the fused rest; two operators raise ValueError."""
    codes = _parse(functions)
    fn = _SampleVolumeMultiSG if sample_grad else _SampleVolumeMulti
    return fn.apply(codes, means, values, conics, samples, binning, debug)


class VolumeSampler:
    """GaussianSampler's shape for D = 3: preprocess once per (means, conics, samples), then
    sample any of the four functions.  covariances are accepted for signature parity with
    GaussianSampler.preprocess (reference py:214-230) and unused, as the cut is derived from
    the conics.  The tensors are kept by reference: when means, conics or samples were changed
    in place since preprocess (an optimizer step), the next sampling call re-bins them first.
    (The functional `sample_volume` with a stale binning writes NaN instead: every call compares
    its tensors with the binned ones on the device, include/dgs_volume.h.)

    sample_grad=True fills `samples.grad` too when the samples require a gradient:
    one more walk of the candidates per backward, about a forward's time, which is why it is asked
    for and not inferred from requires_grad; the default raises NotImplementedError for such
    samples.  Samples stepped in place (`samples -= lr * samples.grad` under no_grad) are re-binned
    by the next call like any other changed tensor.

    periodic=True wraps every axis with period 2 (the torus of the reference's D = 2 rule).  A bool per
    axis, `periodic=(True, True, False)`, makes an axis open: no wrap and no images, coordinates of
    any finite value, so that a Gaussian near t = +1 of an (x, y, t) field does not reach the samples
    near t = -1 ("Open axes").  The axes are kept (`.periodic`, three bools), used by
    `preprocess` and by every automatic re-bin, and carried by the binning to every call."""

    def __init__(self, debug=False, sample_grad=False, periodic=True):
        self.debug = debug
        self.sample_grad = sample_grad
        self.periodic = _axes(periodic)

    def preprocess(self, means, values, covariances, conics, samples):
        self.binning = preprocess_volume(means, conics, samples, self.debug, self.periodic)
        self.means, self.values, self.conics, self.samples = means, values, conics, samples
        self._versions = self._now()
        self._fresh = True

    def _now(self):
        ts = (self.means, self.conics, self.samples)
        if any(t.is_inference() for t in ts):  # no version counter: unknown
            return None
        return tuple(t._version for t in ts)

    def _rebin_if_changed(self):
        now = self._now()
        # changed in place since the binning (or, for inference tensors, possibly changed: every
        # call after the first re-bins) -> re-bin
        if (now is None and not self._fresh) or now != self._versions:
            self.binning = preprocess_volume(self.means, self.conics, self.samples, self.debug, self.periodic)
            self._versions = self._now()
        self._fresh = False

    def _run(self, code):
        self._rebin_if_changed()
        return sample_volume(code, self.means, self.values, self.conics, self.samples, self.binning,
                             self.debug, self.sample_grad)

    def sample_gaussians_multi(self, *functions):
        """Several functions ("gaussian", "derivative", "laplacian", "third", "laplacian_trace" or 0..4,
        or one LinearOperator instance) in one call; returns a tuple in the order asked (sample_volume_multi: one walk of the candidates
        for fields of up to four channels)."""
        self._rebin_if_changed()
        return sample_volume_multi(functions, self.means, self.values, self.conics, self.samples,
                                   self.binning, self.debug, self.sample_grad)

    def sample_gaussians(self):
        return self._run(0)

    def sample_gaussians_derivative(self):
        return self._run(1)

    def sample_gaussians_laplacian(self):
        return self._run(2)

    def sample_gaussians_third_derivative(self):
        return self._run(3)

    def sample_gaussians_laplacian_trace(self):
        """The trace of the laplacian, [N, C] (one value per channel)."""
        return self._run(TRACE)

    def sample_gaussians_operator(self, op):
        """The LinearOperator `op` of the field, [N, C] (one value per channel)."""
        if not isinstance(op, LinearOperator):
            raise TypeError("sample_gaussians_operator takes a LinearOperator")
        return self._run(op)
