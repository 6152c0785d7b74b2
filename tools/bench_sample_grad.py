"""Timing of the sample-position gradient (dgs_sample_backward_samples) at the headline
(1M Gaussians x 2M points, D = 2, C = 1) against its yardstick, in alternating child processes on
one GPU (the pattern of tools/ab.py: clock drift and the box hit every kind alike).

    python tools/bench_sample_grad.py [--rounds 3] [--steps 20] [--out profiles/sample_grad_bench.json]

Kinds: sg:<function> and sg:all (the fused mask of all four) -- the new call, whole (row packing,
the kernel, nothing else is launched with binned inputs); fwd:<function> -- the forward call of the
next-higher function on the same binning, the yardstick of the issue (the forward code is the
parent commit's: this feature does not touch it).  Each call is bracketed by HIP events on the
launch stream after the settle steps; the median over the steps is reported per process, the
median over the rounds per kind.  Also records W_cand / W_live of the lists the kernels walk
(_C.count_pairs).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["gaussian", "derivative", "laplacian", "third"]
KINDS = ["sg:gaussian", "fwd:derivative", "sg:derivative", "fwd:laplacian", "sg:laplacian", "fwd:third",
         "sg:third", "sg:all"]
YARDSTICK = {"sg:gaussian": "fwd:derivative", "sg:derivative": "fwd:laplacian", "sg:laplacian": "fwd:third"}


def child(a):
    sys.path.insert(0, os.path.join(REPO, "diff-gaussian-sampling_amd"))
    import torch
    import diff_gaussian_sampling as dgs
    from diff_gaussian_sampling import synthetic as syn
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    means, values, covs, conics = (t.to(dev) for t in syn.gaussians(a.P, 2, 1, seed=0))
    samples = syn.samples(a.N, 2, seed=4).to(dev)
    R, gb, sb, rg, srg, _ = dgs._C.preprocess_gaussians(means, values, covs, conics, samples, False)
    mode, _, f = a.child.partition(":")
    if mode == "fwd":
        name = "sample_gaussians" + ["", "_derivative", "_laplacian", "_third_derivative"][FUNCS.index(f)]
        fn = getattr(dgs._C, name)
        call = lambda: fn(means, values, conics, samples, R, gb, sb, rg, srg, False)  # noqa: E731
    else:
        codes = [0, 1, 2, 3] if f == "all" else [FUNCS.index(f)]
        dLs = [syn.grad_out(a.N, 2 ** k, 1, seed=5 + k).to(dev) for k in codes]
        call = lambda: dgs._C.sample_gaussians_samples_backward(codes, means, values, conics, samples, dLs, gb,  # noqa: E731
                                                                sb, False)
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
        res["W_cand"], res["W_live"] = dgs._C.count_pairs(means, conics, samples, gb, sb, -104.0)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--N", type=int, default=2_000_000)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--count", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    kinds = a.kinds.split(",")
    runs = {k: [] for k in kinds}
    extra = {}
    for r in range(a.rounds):
        for i, k in enumerate(kinds):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", k, "--steps", str(a.steps), "--warmup",
                   str(a.warmup), "--P", str(a.P), "--N", str(a.N)]
            if r == 0 and i == 0:
                cmd.append("--count")
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-3000:])
                sys.exit(out.returncode)
            j = json.loads(out.stdout.strip().splitlines()[-1])
            runs[k].append(j)
            for w in ("W_cand", "W_live"):
                if w in j:
                    extra[w] = j[w]
            print(r, json.dumps(j), flush=True)
    med = {k: statistics.median(j["ms"] for j in js) for k, js in runs.items()}
    ratio = {k: med[k] / med[y] for k, y in YARDSTICK.items() if k in med and y in med}
    res = {"P": a.P, "N": a.N, "D": 2, "C": 1, "rounds": a.rounds, "steps": a.steps, "median_ms": med,
           "ratio_to_yardstick": ratio, **extra, "runs": runs}
    print("RESULT", json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
