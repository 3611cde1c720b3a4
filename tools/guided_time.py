"""Time the HIP box-window guided filter (phl.guided_filter behind crf.guided) against the torch form of crf/guided.py
on the same GPU, in one process.

    python tools/guided_time.py [--reps N] [--only NAME] [--no-torch]

Event-timed after one warm-up call of each path; the two paths alternate, call by call, and each keeps the best of its
--reps (default 5) calls.  Cases: BatchedGuidedAdjacency r = 20, s = 2 at
[1, 64, 288, 384] (the shape of the reference's benchmarking.ipynb), [1, 231, 1110, 1390] with 1 and 3 guide channels,
[1, 64, 1536, 2048] with 16; the plain GuidedFilter r = 20 at [1, 64, 1536, 2048]; one 5-iteration CRFasRNN no-grad
forward at [1, 64, 288, 384].  GB/s = compulsory bytes / time of the HIP path, the bytes being: the sampled rows of y
(1 / s of the plane), the coefficient planes written and read back ((cx + 1) / s^2 planes each way), src read and out
written, and the guide once; "of copy" is that rate over phl.stream_copy's in the same process.  For the CRFasRNN case
the bytes are the guided filter's alone while the time is the whole forward (compatibility product and softmax
included), so its rate understates the filter's.  Event times include
launch gaps; for kernel times run under `rocprofv3 --kernel-trace --stats -- python tools/guided_time.py --only NAME
--no-torch` in a run of its own.  Every case is a separate `timeout`-guarded step when driven from a shell loop:
`for n in $(python tools/guided_time.py --list); do timeout -k 10 300 python tools/guided_time.py --only $n || break; done`.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

import phl  # noqa: E402
from crf import guided  # noqa: E402
from crf.crf_module import CRFasRNN, charb  # noqa: E402

# name: (kind, cy, cx, H, W, r, s)
CASES = {
    "bga_64x288x384": ("bga", 64, 1, 288, 384, 20, 2),
    "bga_231x1110x1390_cx1": ("bga", 231, 1, 1110, 1390, 20, 2),
    "bga_231x1110x1390_cx3": ("bga", 231, 3, 1110, 1390, 20, 2),
    "bga_64x1536x2048_cx16": ("bga", 64, 16, 1536, 2048, 20, 2),
    "gf_64x1536x2048": ("gf", 64, 1, 1536, 2048, 20, 1),
    "crfasrnn5_64x288x384": ("crf", 64, 1, 288, 384, 20, 2),
}


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _time(fns, reps):
    """Best of ``reps`` for every callable of ``fns``, the callables taking turns."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            best[k] = min(best[k], _once(fn))
    return best


def _torch_form(fn):
    real = guided.GuidedFilter._fused
    guided.GuidedFilter._fused = lambda self, *a, **k: None
    try:
        return fn()
    finally:
        guided.GuidedFilter._fused = real


def copy_rate(dev):
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty_like(a)
    ms = _time([lambda: phl.stream_copy(b, a)], 5)[0]
    return 2 * a.numel() * 4 / ms / 1e6


def run(name, reps, with_torch, rate):
    kind, cy, cx, H, W, r, s = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand((1, cy, H, W), device=dev, generator=g)
    x = torch.rand((1, cx, H, W), device=dev, generator=g)
    plane = H * W * 4
    per_label = plane * (1.0 / s + 2.0 * (cx + 1) / s ** 2 + 1 + (1 if kind != "gf" else 0))
    nbytes = cy * per_label + cx * plane
    if kind == "crf":
        m = CRFasRNN(charb(3.0), niters=5).to(dev)
        labels = torch.arange(cy, dtype=torch.float32, device=dev)
        fn = lambda: m(x, y, labels=labels)  # noqa: E731
        nbytes *= 5
    else:
        m = (guided.GuidedFilter(cx, r, 1e-5) if kind == "gf" else guided.BatchedGuidedAdjacency(cx, r, 1e-5, subsample_ratio=s)).to(dev)
        fn = lambda: m(y, x)  # noqa: E731
    with torch.no_grad():
        if with_torch:
            hip, tor = _time([fn, lambda: _torch_form(fn)], reps)
        else:
            hip, tor = _time([fn], reps)[0], float("nan")
    gbs = nbytes / hip / 1e6
    row = dict(case=name, hip_ms=round(hip, 3), torch_ms=round(tor, 3), speedup=round(tor / hip, 2), compulsory_GBps=round(gbs, 1),
               of_copy=round(gbs / rate, 3))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print(" ".join(CASES))
        return
    rate = copy_rate(torch.device("cuda", 0))
    print(json.dumps(dict(stream_copy_GBps=round(rate, 1))), flush=True)
    for name in ([a.only] if a.only else CASES):
        run(name, a.reps, not a.no_torch, rate)


if __name__ == "__main__":
    main()
