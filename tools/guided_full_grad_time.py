"""Time training through the full-covariance guided filter: ``full_cov_grad=True`` (phl.GuidedFilterFullFn, forward and
backward on the HIP kernels) against the fp32 torch autograd path of the same model (the torch form of crf/guided.py with
its batched inverse: the baseline) and against the diagonal model's kernel route (``fused_grad=True``: what the extra terms
cost), same GPU, one process.

    python tools/guided_full_grad_time.py [--reps N] [--only NAME] [--list]

Event-timed after one warm-up of each path; the three paths alternate, step by step, and each keeps the best of its
--reps (default 5) steps.  A step is a forward and a backward with gradients for y and omega (``_x``-suffixed case: the
guide too) of BatchedGuidedAdjacency(3, 15, 1e-2, full_cov=True) on the correlated guide (x_c = base + 0.25 noise_c), at
the shapes of tools/guided_full_time.py: [1, 16, 288, 384] and [1, 18, 1110, 1390] at s = 2, [1, 64, 1110, 1390] at s = 2
and s = 1; and a 5-iteration CRFasRNN(charb(.05), gchannels=3, full_cov=True) training step (logits, Mu and omega) at the
first two.  ``*_MiB`` is torch.cuda.max_memory_allocated over one step of that path beyond what was allocated before it
(the inputs; the gradients of the step before are released first, so the three paths are measured from one state).  A path that runs out of memory is reported as null.  Every case is a separate `timeout`-guarded step when
driven from a shell loop:
`for n in $(python tools/guided_full_grad_time.py --list); do timeout -k 10 300 python tools/guided_full_grad_time.py --only $n || break; done`.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

from crf import guided  # noqa: E402
from crf.crf_module import CRFasRNN, charb  # noqa: E402

# name: (kind, cy, H, W, s, guide gradient)
CASES = {
    "bga_16x288x384_s2": ("bga", 16, 288, 384, 2, False),
    "bga_16x288x384_s2_x": ("bga", 16, 288, 384, 2, True),
    "bga_18x1110x1390_s2": ("bga", 18, 1110, 1390, 2, False),
    "bga_64x1110x1390_s2": ("bga", 64, 1110, 1390, 2, False),
    "bga_64x1110x1390_s1": ("bga", 64, 1110, 1390, 1, False),
    "crfasrnn5_16x288x384": ("crf", 16, 288, 384, 2, False),
    "crfasrnn5_18x1110x1390": ("crf", 18, 1110, 1390, 2, False),
}
CX, R, EPS = 3, 15, 1e-2
PATHS = ("full", "torch", "diag")


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def run(name, reps):
    kind, cy, H, W, s, grad_x = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand((1, cy, H, W), device=dev, generator=g, requires_grad=True)
    x = (torch.rand((1, 1, H, W), device=dev, generator=g) + 0.25 * torch.rand((1, CX, H, W), device=dev, generator=g))
    x.requires_grad_(grad_x)
    up = torch.rand((1, cy, H, W), device=dev, generator=g)
    if kind == "crf":
        m = CRFasRNN(charb(.05), niters=5, r=R, eps=EPS, gchannels=CX, full_cov=True, full_cov_grad=True).to(dev)
        W_, fwd = m.W, lambda: m(x, y)  # noqa: E731
    else:
        m = guided.BatchedGuidedAdjacency(CX, R, EPS, subsample_ratio=s, full_cov=True, full_cov_grad=True).to(dev)
        W_, fwd = m, lambda: m(y, x)  # noqa: E731

    def clear():
        y.grad = x.grad = None
        m.zero_grad(set_to_none=True)

    def step(path):
        W_.full_cov, W_.full_cov_grad, W_.fused_grad = path != "diag", path == "full", path == "diag"
        clear()
        (fwd() * up).sum().backward()

    best, peak = {p: float("inf") for p in PATHS}, {}
    for p in PATHS:
        clear()                                       # (the gradients of the path before are not this path's inputs)
        try:
            peak[p] = _peak(lambda: step(p))          # (also the warm-up)
        except torch.cuda.OutOfMemoryError:
            best[p] = peak[p] = None
            torch.cuda.empty_cache()
    for _ in range(reps):
        for p in PATHS:
            if best[p] is not None:
                best[p] = min(best[p], _once(lambda: step(p)))
    rnd = lambda v, n: None if v is None else round(v, n)  # noqa: E731
    ratio = lambda a, b: round(best[a] / best[b], 2) if best[a] is not None and best[b] is not None else None  # noqa: E731
    print(json.dumps(dict(case=name, full_ms=rnd(best["full"], 3), torch_ms=rnd(best["torch"], 3), diag_ms=rnd(best["diag"], 3),
                          speedup=ratio("torch", "full"), over_diag=ratio("full", "diag"), full_MiB=rnd(peak["full"], 1),
                          torch_MiB=rnd(peak["torch"], 1), diag_MiB=rnd(peak["diag"], 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print(" ".join(CASES))
        return
    for name in ([a.only] if a.only else CASES):
        run(name, a.reps)


if __name__ == "__main__":
    main()
