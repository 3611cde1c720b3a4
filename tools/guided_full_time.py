"""Time the full-covariance guided filter (phl.guided_filter(full_cov=True) behind crf.guided) against the diagonal
kernels and against its own torch form (crf/guided.py: get_coeffs with torch.linalg.inv) on the same GPU, in one process.

    python tools/guided_full_time.py [--reps N] [--only NAME] [--no-torch] [--list]

BatchedGuidedAdjacency, RGB guide (cx = 3), r = 15, at [1, 18, 1110, 1390] and [1, 64, 1110, 1390] with subsample 2 and 1
(18 labels: CRFdepthUpsampler's).  After one warm-up call of each path the paths take turns, call by call, event-timed;
each reports the median of its --reps (default 9) calls.  Per case one JSON line:
    full_ms, diag_ms, full_over_diag      the two kernel paths (the diagonal one is the kernel every earlier build has)
    torch_ms, torch_over_full            the fp32 torch form of the full model (skipped with --no-torch)
    torch_peak_MiB                       torch.cuda.max_memory_allocated over one torch-form call, above what was
                                         allocated before it (inputs excluded, the result included)
    full_peak_MiB                        the same for the kernel path (its result), plus the library's stream-ordered
                                         temporaries, which torch's allocator does not see: mx and P in fp64 and one chunk
                                         of coefficient planes (computed from phl.guided_filter_labels_per_chunk)
Event times include launch gaps; for per-kernel times run `rocprofv3 --kernel-trace --stats -- python
tools/guided_full_time.py --only NAME --no-torch` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

import phl  # noqa: E402
from crf import guided  # noqa: E402

R, CX = 15, 3
# name: (cy, H, W, s)
CASES = {
    "bga_18x1110x1390_s2": (18, 1110, 1390, 2),
    "bga_64x1110x1390_s2": (64, 1110, 1390, 2),
    "bga_18x1110x1390_s1": (18, 1110, 1390, 1),
    "bga_64x1110x1390_s1": (64, 1110, 1390, 1),
}


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _time(fns, reps):
    """Median of ``reps`` for every callable of ``fns``, the callables taking turns, after one warm-up call each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(_once(fn))
    return [statistics.median(t) for t in times]


def _peak(fn):
    """MiB that one call of fn allocates from torch's allocator at its peak, above what is allocated now."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _torch_form(fn):
    real = guided.GuidedFilter._fused
    guided.GuidedFilter._fused = lambda self, *a, **k: None
    try:
        return fn()
    finally:
        guided.GuidedFilter._fused = real


def run(name, reps, with_torch):
    cy, H, W, s = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand((1, cy, H, W), device=dev, generator=g)
    x = torch.rand((1, 1, H, W), device=dev, generator=g) + 0.25 * torch.rand((1, CX, H, W), device=dev, generator=g)
    full = guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s, full_cov=True).to(dev)
    diag = guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s).to(dev)
    h, w = H // s, W // s
    chunk = phl.guided_filter_labels_per_chunk(1, cy, CX, h, w)
    temps = h * w * (8 * CX + 8 * CX * (CX + 1) // 2 + 4 * (CX + 1) * chunk) / 2 ** 20
    with torch.no_grad():
        fns = [lambda: full(y, x), lambda: diag(y, x)] + ([lambda: _torch_form(lambda: full(y, x))] if with_torch else [])
        ms = _time(fns, reps)
        row = dict(case=name, full_ms=round(ms[0], 3), diag_ms=round(ms[1], 3), full_over_diag=round(ms[0] / ms[1], 3))
        row["full_peak_MiB"] = round(_peak(fns[0]) + temps, 1)
        if with_torch:
            row.update(torch_ms=round(ms[2], 3), torch_over_full=round(ms[2] / ms[0], 1), torch_peak_MiB=round(_peak(fns[2]), 1))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print(" ".join(CASES))
        return
    for name in ([a.only] if a.only else CASES):
        run(name, a.reps, not a.no_torch)


if __name__ == "__main__":
    main()
