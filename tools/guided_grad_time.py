"""Time training through the box-window guided filter: ``fused_grad=True`` (phl.GuidedFilterFn, forward and backward on the
HIP kernels) against the torch autograd path (``fused_grad=False``, the torch form of crf/guided.py), same GPU, one process.

    python tools/guided_grad_time.py [--reps N] [--only NAME] [--list]

Event-timed after one warm-up of each path; the two paths alternate, step by step, and each keeps the best of its
--reps (default 5) steps.  A step is a forward and a backward with gradients for y and omega (``_x``-suffixed cases: the
guide too).  Cases: BatchedGuidedAdjacency r = 20, s = 2 at [1, 64, 288, 384], [1, 231, 1110, 1390] with 1 and 3 guide
channels, [1, 64, 1536, 2048] with 16; and a 5-iteration CRFasRNN training step (logits, Mu and omega) at
[1, 64, 288, 384].  ``*_MiB`` is torch.cuda.max_memory_allocated over one step of that path beyond what was allocated
before it (the inputs).  A path that runs out of memory is reported as null.  Every case is a separate
`timeout`-guarded step when driven from a shell loop:
`for n in $(python tools/guided_grad_time.py --list); do timeout -k 10 300 python tools/guided_grad_time.py --only $n || break; done`.
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

# name: (kind, cy, cx, H, W, r, s, guide gradient)
CASES = {
    "bga_64x288x384": ("bga", 64, 1, 288, 384, 20, 2, False),
    "bga_64x288x384_x": ("bga", 64, 1, 288, 384, 20, 2, True),
    "bga_231x1110x1390_cx1": ("bga", 231, 1, 1110, 1390, 20, 2, False),
    "bga_231x1110x1390_cx3": ("bga", 231, 3, 1110, 1390, 20, 2, False),
    "bga_64x1536x2048_cx16": ("bga", 64, 16, 1536, 2048, 20, 2, False),
    "crfasrnn5_64x288x384": ("crf", 64, 1, 288, 384, 20, 2, False),
}


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
    kind, cy, cx, H, W, r, s, grad_x = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand((1, cy, H, W), device=dev, generator=g, requires_grad=True)
    x = torch.rand((1, cx, H, W), device=dev, generator=g, requires_grad=grad_x)
    up = torch.rand((1, cy, H, W), device=dev, generator=g)
    if kind == "crf":
        m = CRFasRNN(charb(3.0), niters=5, fused_grad=True).to(dev)
        W_, fwd = m.W, lambda: m(x, y)  # noqa: E731
    else:
        m = guided.BatchedGuidedAdjacency(cx, r, 1e-5, subsample_ratio=s, fused_grad=True).to(dev)
        W_, fwd = m, lambda: m(y, x)  # noqa: E731

    def step(flag):
        W_.fused_grad = flag
        y.grad = x.grad = None
        m.zero_grad(set_to_none=True)
        (fwd() * up).sum().backward()

    best, peak = {True: float("inf"), False: float("inf")}, {}
    for flag in (True, False):
        try:
            peak[flag] = _peak(lambda: step(flag))          # (also the warm-up)
        except torch.cuda.OutOfMemoryError:
            best[flag] = peak[flag] = None
            torch.cuda.empty_cache()
    for _ in range(reps):
        for flag in (True, False):
            if best[flag] is not None:
                best[flag] = min(best[flag], _once(lambda: step(flag)))
    rnd = lambda v, n: None if v is None else round(v, n)  # noqa: E731
    both = best[True] is not None and best[False] is not None
    print(json.dumps(dict(case=name, fused_ms=rnd(best[True], 3), torch_ms=rnd(best[False], 3),
                          speedup=round(best[False] / best[True], 2) if both else None, fused_MiB=rnd(peak[True], 1),
                          torch_MiB=rnd(peak[False], 1))), flush=True)


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
