"""Times the fused D = 3 multi-function call against the per-function calls on one binning.

    python tools/volume_multi_bench.py [--P 1000000] [--grid3 64] [--functions gaussian,laplacian,...]
                                       [--rounds 3] [--steps 3] [--C 3] [--separate-only] [--trace-vs-hessian]
                                       [--operator-vs-multi] [--periodic 110]

The workload is `bench.py --op volume`'s (syn.gaussians3, a g^3 lattice; C = 1 unless --C).  After settle
steps, fused and separate steps alternate for `--rounds` rounds in one process, so clock drift
hits both alike; each figure is the median over the rounds of the mean ms per forward +
backward step (preprocess excluded).  Prints one JSON line: fused_ms, separate_ms (the sum of the
per-function calls, same outputs and gradients), per-function step times `single_ms`, the speedup,
and `fused_over_last`, the fused step against the most expensive (last named) function alone.
--periodic 110 bins the field with axis 2 open (one 0/1 per axis; DESIGN.md 4.8, "Open axes").
--separate-only times the per-function calls only (a package without the fused call, for A/B
runs through tools/ab.py --script); --C sets the channel count (the fused call shares one walk up
to C = 4; with more channels, or in a package from before that, it is the per-function calls added:
the yardstick of an A/B run through tools/ab.py --script against a build of the parent commit).

--trace-vs-hessian (with "laplacian_trace" among --functions): instead of fused against separate,
times in alternation the call as given (`fused_ms`, also `trace_ms`) against what a user without the
trace does (`separate_ms`, also `hessian_ms`): the same call with "laplacian" in its place, followed
by `out.diagonal(dim1=1, dim2=2).sum(-1)`; both are forward + backward from the same upstream
gradients.  `single_ms` then holds the other functions' single calls and the laplacian's.

--operator-vs-multi (--functions is not used): the heat operator u_t - kappa (u_xx + u_yy) of an
(x, y, t) field, kappa = 0.01, forward + backward over one binning, timed in alternation as
  route      what a user without LinearOperator does: sample_gaussians_multi("gaussian", "derivative",
             "laplacian") and the contraction in torch, the loss on the residual (`separate_ms`)
  route_gdr  the same with the loss on the gaussian, the derivative and the residual
  operator   sample_gaussians_operator(heat), the loss on it (`fused_ms`)
  op_gd      sample_gaussians_multi("gaussian", "derivative", heat), the loss on all three
and the single calls gaussian, derivative, laplacian, laplacian_trace; all in `single_ms`.  In a
package from before LinearOperator only the routes and the single calls run (the yardstick of an A/B
run through tools/ab.py --script against a build of the parent commit).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.environ.get("DGS_PKG_ROOT", os.path.join(REPO, "diff-gaussian-sampling_amd"))]  # variants: tools/variant.sh

import torch  # noqa: E402

from diff_gaussian_sampling import synthetic as syn  # noqa: E402
from diff_gaussian_sampling.volume import FUNCTION_CODES, VolumeSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--grid3", type=int, default=64)
    ap.add_argument("--functions", default="gaussian,derivative,laplacian,third")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--settle", type=int, default=2)
    ap.add_argument("--separate-only", action="store_true")
    ap.add_argument("--trace-vs-hessian", action="store_true")
    ap.add_argument("--operator-vs-multi", action="store_true")
    ap.add_argument("--C", type=int, default=1, help="channels")
    ap.add_argument("--periodic", default=os.environ.get("DGS_VOLUME_BENCH_PERIODIC", "111"),
                    help="one 0/1 per axis, 0: the axis is open (VolumeSampler(periodic=...)); the default also "
                         "from DGS_VOLUME_BENCH_PERIODIC, which tools/ab.py's base:K=V form can set per variant")
    args = ap.parse_args()
    C = args.C
    fns = args.functions.split(",")
    dev = torch.device("cuda:0")
    means, values, covs, conics = (t.to(dev) for t in syn.gaussians3(args.P, C, seed=0))
    samples = syn.grid_samples3(args.grid3).to(dev)
    N = samples.shape[0]
    for t in (means, values, conics):
        t.requires_grad_(True)
    axes = tuple(ch == "1" for ch in args.periodic)
    assert len(axes) == 3 and set(args.periodic) <= {"0", "1"}, "--periodic is three of 0/1"
    # (all periodic: the call every package has, so a build of a parent commit runs it too)
    vs = VolumeSampler(False) if all(axes) else VolumeSampler(False, periodic=axes)
    vs.preprocess(means, values, covs, conics, samples)
    gen = torch.Generator().manual_seed(5)
    if args.operator_vs_multi:
        return operator_vs_multi(args, vs, (means, values, conics), N, C, gen, dev)
    order = {"laplacian_trace": 0}  # (its output is [N, C])
    w = {f: torch.randn((N,) + (3,) * order.get(f, FUNCTION_CODES[f]) + (C,), generator=gen).to(dev) for f in fns}
    single = {"gaussian": vs.sample_gaussians, "derivative": vs.sample_gaussians_derivative,
              "laplacian": vs.sample_gaussians_laplacian, "third": vs.sample_gaussians_third_derivative}
    if "laplacian_trace" in fns:
        single["laplacian_trace"] = vs.sample_gaussians_laplacian_trace
    if args.trace_vs_hessian:
        return trace_vs_hessian(args, vs, fns, w, single, (means, values, conics), N)

    def step(which):
        for t in (means, values, conics):
            t.grad = None
        if which == "fused":
            outs = vs.sample_gaussians_multi(*fns)
            torch.autograd.backward(list(outs), [w[f] for f in fns])
        else:
            for f in (fns if which == "separate" else [which]):
                single[f]().backward(w[f])

    def timed(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(which)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    kinds = (["separate"] if args.separate_only else ["fused", "separate"])
    for k in kinds:
        for _ in range(args.settle):
            step(k)
    times = {k: [] for k in kinds + fns}
    for _ in range(args.rounds):
        for k in kinds + fns:
            times[k].append(timed(k))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"P": args.P, "N": N, "C": C, "grid3": args.grid3, "functions": fns, "rounds": args.rounds, "steps": args.steps,
           "periodic": args.periodic, "separate_ms": med["separate"], "single_ms": {f: med[f] for f in fns},
           "separate_rounds_ms": times["separate"]}
    if not args.separate_only:
        res.update(fused_ms=med["fused"], fused_rounds_ms=times["fused"], speedup=med["separate"] / med["fused"],
                   fused_over_last=med["fused"] / med[fns[-1]])
    print(json.dumps(res), flush=True)


def trace_vs_hessian(args, vs, fns, w, single, params, N):
    assert "laplacian_trace" in fns and "laplacian" not in fns, "--functions must hold laplacian_trace, not laplacian"
    hfns = ["laplacian" if f == "laplacian_trace" else f for f in fns]
    others = [f for f in fns if f != "laplacian_trace"] + ["laplacian"]

    def step(which):
        for t in params:
            t.grad = None
        if which == "trace":
            outs = vs.sample_gaussians_multi(*fns) if len(fns) > 1 else (single[fns[0]](),)
        elif which == "hessian":
            outs = vs.sample_gaussians_multi(*hfns) if len(fns) > 1 else (single["laplacian"](),)
            outs = [o.diagonal(dim1=1, dim2=2).sum(-1) if f == "laplacian" else o for f, o in zip(hfns, outs)]
        else:  # a single function, as the main mode times it
            o = single[which]()
            return o.backward(torch.ones_like(o) if which == "laplacian" else w[which])
        torch.autograd.backward(list(outs), [w[f] for f in fns])

    def timed(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(which)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    kinds = ["trace", "hessian"]
    for k in kinds:
        for _ in range(args.settle):
            step(k)
    times = {k: [] for k in kinds + others}
    for _ in range(args.rounds):
        for k in kinds + others:
            times[k].append(timed(k))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"P": args.P, "N": N, "C": args.C, "grid3": args.grid3, "functions": fns, "mode": "trace-vs-hessian",
                      "rounds": args.rounds, "steps": args.steps, "trace_ms": med["trace"], "hessian_ms": med["hessian"],
                      "fused_ms": med["trace"], "separate_ms": med["hessian"], "speedup": med["hessian"] / med["trace"],
                      "trace_rounds_ms": times["trace"], "hessian_rounds_ms": times["hessian"],
                      "single_ms": {f: med[f] for f in others}}), flush=True)


def operator_vs_multi(args, vs, params, N, C, gen, dev):
    kappa = 0.01
    try:
        from diff_gaussian_sampling.volume import LinearOperator
        heat = LinearOperator(b=(0.0, 0.0, 1.0), W=LinearOperator.laplacian((0, 1), -kappa).W)
    except ImportError:  # a package from before the operator: the routes and the single calls only
        heat = None
    w = {f: torch.randn((N,) + (3,) * k + (C,), generator=gen).to(dev) for f, k in (("g", 0), ("d", 1), ("r", 0))}
    single = {"gaussian": vs.sample_gaussians, "derivative": vs.sample_gaussians_derivative,
              "laplacian": vs.sample_gaussians_laplacian}
    if hasattr(vs, "sample_gaussians_laplacian_trace"):
        single["laplacian_trace"] = vs.sample_gaussians_laplacian_trace

    def step(which):
        for t in params:
            t.grad = None
        if which in ("route", "route_gdr"):
            g, d, lap = vs.sample_gaussians_multi("gaussian", "derivative", "laplacian")
            r = d[:, 2] - kappa * (lap[:, 0, 0] + lap[:, 1, 1])
            outs, ws = ([r], [w["r"]]) if which == "route" else ([g, d, r], [w["g"], w["d"], w["r"]])
        elif which == "operator":
            outs, ws = [vs.sample_gaussians_operator(heat)], [w["r"]]
        elif which == "op_gd":
            outs, ws = list(vs.sample_gaussians_multi("gaussian", "derivative", heat)), [w["g"], w["d"], w["r"]]
        else:
            o = single[which]()
            return o.backward(torch.ones_like(o))
        torch.autograd.backward(outs, ws)

    def timed(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(which)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    kinds = ["route", "route_gdr"] + (["operator", "op_gd"] if heat is not None else []) + list(single)
    for k in kinds[:4]:
        for _ in range(args.settle):
            step(k)
    times = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            times[k].append(timed(k))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"P": args.P, "N": N, "C": C, "grid3": args.grid3, "mode": "operator-vs-multi", "rounds": args.rounds,
           "steps": args.steps, "separate_ms": med["route"], "single_ms": med, "rounds_ms": times}
    if heat is not None:
        res.update(fused_ms=med["operator"], speedup=med["route"] / med["operator"],
                   speedup_gd=med["route_gdr"] / med["op_gd"])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
