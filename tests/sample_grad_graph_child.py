"""Child process of tests/test_gpu_sample_grad.py (the pattern of tests/graph_child.py: a failure
inside the HIP runtime's graph capture fails one test instead of ending the pytest process).
A forward + backward WITH the sample gradient is captured into a torch.cuda.CUDAGraph on a fixed
binning and replayed: the forward and dL/dsamples (a gather: no atomics) must equal the eager
call bit for bit, also after dL changes in place.  Prints "ok" on success."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diff-gaussian-sampling_amd"))

import diff_gaussian_sampling as dgs  # noqa: E402
from diff_gaussian_sampling import synthetic as syn  # noqa: E402


def main():
    dev = torch.device("cuda")
    P, N = 3000, 9000
    means, values, covs, conics = (t.to(dev) for t in syn.gaussians(P, 2, 1, seed=3))
    samples = syn.samples(N, 2, seed=9).to(dev)
    R, gb, sb, rg, srg, _ = dgs.preprocess_gaussians(means, values, covs, conics, samples, False)
    dL = torch.randn(N, 2, 1, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    for t in (means, samples):
        t.requires_grad_(True)

    def step():
        out = dgs.sample_gaussians_derivative(means, values, conics, samples, R, gb, sb, rg, srg, False)
        gm, gs = torch.autograd.grad(out, (means, samples), dL)
        return out.detach(), gm, gs

    ref_out, _, ref_gs = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_gm, g_gs = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, ref_out), "forward replay differs from the eager call"
        assert torch.equal(g_gs, ref_gs), "dL/dsamples replay differs from the eager call"
    with torch.no_grad():
        dL.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    _, _, new_gs = step()
    assert torch.equal(g_gs, new_gs), "dL/dsamples replay after the dL change differs"
    assert not torch.equal(new_gs, ref_gs) and bool(new_gs.abs().sum() > 0)
    print("ok")


if __name__ == "__main__":
    main()
