"""Timing of the D = 3 sample-position gradient (dgs_volume_backward_samples) on the project's D = 3
workload (`bench.py --op volume`'s field: syn.gaussians3(1M), a 64^3 lattice, C = 1) against its
yardstick, in alternating child processes on one GPU (the pattern of tools/bench_sample_grad.py:
clock drift and the box hit every kind alike).

    python tools/volume_sample_grad_bench.py [--rounds 3] [--steps 10] [--out profiles/volume_sample_grad_bench.json]
                                             [--C 3] [--kinds sg:gaussian+derivative+laplacian] [--pkgs base,variants/NAME]

Kinds: sg:<function>, sg:all (mask 15) and sg:<f>+<g>+... (that mask; laplacian_trace among the names
takes the _ops binding, heat -- a LinearOperator, code 5 -- the _linop one) -- the new call, whole (the
input check and the kernels); fwd:<function> -- the forward call on the same binning.  --C sets the
channel count (several functions share one walk up to C = 4; above, the per-function calls are added).
--pkgs times every kind under several packages in turn (base: the in-tree one; variants/NAME: a
tools/variant.sh build, e.g. of the parent commit), reported as kind@package.  The yardstick of sg:<f> is the
forward of the next-higher function (the same walk, the same G and a, terms one order lower; DESIGN.md
4.9), with the section's margin of 1.25x; the forward code is the parent commit's, which this
feature leaves unchanged.  sg:third and sg:all have no yardstick: they are reported alone, sg:all
also against the sum of the four single calls.  Each call is bracketed by HIP events on the launch
stream after the settle steps; the median over the steps is reported per process, the median over
the rounds per kind.  A ratio outside the margin is reported as such (within_margin false).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["gaussian", "derivative", "laplacian", "third"]
KINDS = ["fwd:gaussian", "sg:gaussian", "fwd:derivative", "sg:derivative", "fwd:laplacian", "sg:laplacian",
         "fwd:third", "sg:third", "sg:all"]
YARDSTICK = {"sg:gaussian": "fwd:derivative", "sg:derivative": "fwd:laplacian", "sg:laplacian": "fwd:third"}
MARGIN = 1.25


def child(a):
    sys.path.insert(0, os.environ.get("DGS_PKG_ROOT", os.path.join(REPO, "diff-gaussian-sampling_amd")))
    import torch
    import diff_gaussian_sampling as dgs
    from diff_gaussian_sampling import synthetic as syn
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    means, values, _, conics = (t.to(dev) for t in syn.gaussians3(a.P, a.C, seed=0))
    samples = syn.grid_samples3(a.grid3).to(dev)
    N = samples.shape[0]
    buf = dgs._C.volume_preprocess(means, conics, samples, False)
    mode, _, f = a.child.partition(":")
    if mode == "fwd":
        code = FUNCS.index(f)
        call = lambda: dgs._C.volume_forward(code, means, values, conics, samples, buf, False)  # noqa: E731
    else:
        codes = [0, 1, 2, 3] if f == "all" else [(FUNCS + ["laplacian_trace", "heat"]).index(x) for x in f.split("+")]
        gen = torch.Generator().manual_seed(5)
        dLs = [torch.randn((N, 1 if k >= 4 else 3 ** k, a.C), generator=gen).to(dev) for k in codes]
        sg = dgs._C.volume_samples_backward_ops if 4 in codes else dgs._C.volume_samples_backward
        call = lambda: sg(codes, means, values, conics, samples, dLs, buf, False)  # noqa: E731
        if 5 in codes:  # the heat operator u_t - 0.01 (u_xx + u_yy): the _linop binding with its coefficients
            heat = [0.0, 0.0, 0.0, 1.0, -0.01, 0.0, 0.0, -0.01, 0.0, 0.0]
            call = lambda: dgs._C.volume_samples_backward_linop(codes, heat, means, values, conics, samples, dLs,  # noqa: E731
                                                                buf, False)
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res = {"kind": a.child, "ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "steps": a.steps}
    if a.count:
        res["W_eval"], res["W_live"] = dgs._C.volume_count_pairs(means, conics, samples, buf)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--grid3", type=int, default=64)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--C", type=int, default=1)
    ap.add_argument("--pkgs", default="base", help="packages timed in turn: base or variants/NAME")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--count", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    pkgs = a.pkgs.split(",")
    kinds = [k if p == "base" else k + "@" + p for k in a.kinds.split(",") for p in pkgs]
    runs = {k: [] for k in kinds}
    extra = {}
    for r in range(a.rounds):
        for i, k in enumerate(kinds):
            kind, _, pkg = k.partition("@")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps), "--warmup",
                   str(a.warmup), "--P", str(a.P), "--grid3", str(a.grid3), "--C", str(a.C)]
            if r == 0 and i == 0:
                cmd.append("--count")
            env = dict(os.environ)
            if pkg:
                env["DGS_PKG_ROOT"] = os.path.join(REPO, pkg)
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-3000:])
                sys.exit(out.returncode)
            j = json.loads(out.stdout.strip().splitlines()[-1])
            j["kind"] = k
            runs[k].append(j)
            for w in ("W_eval", "W_live"):
                if w in j:
                    extra[w] = j[w]
            print(r, json.dumps(j), flush=True)
    med = {k: statistics.median(j["ms"] for j in js) for k, js in runs.items()}
    ratio = {k: med[k] / med[y] for k, y in YARDSTICK.items() if k in med and y in med}
    res = {"P": a.P, "N": a.grid3 ** 3, "grid3": a.grid3, "D": 3, "C": a.C, "rounds": a.rounds, "steps": a.steps,
           "median_ms": med, "yardstick": {k: y for k, y in YARDSTICK.items() if k in ratio},
           "ratio_to_yardstick": ratio, "margin": MARGIN, "within_margin": {k: r <= MARGIN for k, r in ratio.items()}}
    singles = ["sg:" + f for f in FUNCS]
    if "sg:all" in med and all(s in med for s in singles):
        res["sum_of_single_sg_ms"] = sum(med[s] for s in singles)
        res["sg_all_over_sum_of_singles"] = med["sg:all"] / res["sum_of_single_sg_ms"]
    res.update(extra)
    res["runs"] = runs
    print("RESULT", json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
