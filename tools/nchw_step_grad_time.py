"""Time the training step (phl.NchwStepTrain, phl_nchw_train.hip) and CRFasRNN(fused_step=True) against the plain
autograd loop they replace, on one GPU in one process.

    python tools/nchw_step_grad_time.py [--reps N] [--only NAME] [--list]

At [1, 16, 288, 384], [1, 18, 1110, 1390] and [1, 64, 1110, 1390]:
  step_*   forward + backward of one step with gradients for E0, G and Mu: phl.nchw_step_train_fn(E0, G, M) against
           ``F.conv2d(F.softmax(-(E0 + G), 1), M.t()[..., None, None])`` under autograd, each followed by ``.backward(gY)``.
           Bytes the kernels must move: 2 L n 4 read and L n 4 written in the forward, 3 L n 4 read and L n 4 written in
           the backward -- 7 L n 4 in all; GB/s and "of copy" (over phl.stream_copy's rate in the same process) from that.
  crf_*    one training step of CRFasRNN(charb(.05), niters=5, fused_grad=True) -- forward, a sum against a fixed tensor,
           backward to the logits, the guide, gamma, s and omega -- with fused_step=True against fused_step=False.
Event-timed after five warm-up calls of each path (clocks and code objects up); the two paths alternate, call by call; the
median of --reps (default 15) calls of each is reported, with the fastest and the slowest beside it as the spread.
peak_MiB: torch.cuda.max_memory_allocated over one call of each path, from the same starting state (the inputs
allocated, no gradients held); the kernels' stream-ordered scratch for Mu's gradient, at most 32 MiB, is not torch's and
is not in it.  Drive the cases as separate steps, each under its own time limit (names: --list).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

import phl  # noqa: E402
from crf.crf_module import CRFasRNN, charb  # noqa: E402

SHAPES = ((16, 288, 384), (18, 1110, 1390), (64, 1110, 1390))
CASES = {f"{kind}_{L}x{H}x{W}": (kind, L, H, W) for kind in ("step", "crf") for L, H, W in SHAPES}


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _time(fns, reps, warmup=5):
    """(median, fastest, slowest) of ``reps`` calls for every callable of ``fns``, the callables taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(_once(fn))
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def _peak(fn, clear):
    """torch's peak allocation over one call, in MiB, the gradients of the call before dropped first."""
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def copy_rate(dev):
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty_like(a)
    ms = _time([lambda: phl.stream_copy(b, a)], 5)[0][0]
    return 2 * a.numel() * 4 / ms / 1e6


def run(name, reps, rate):
    kind, L, H, W = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    shape, n = (1, L, H, W), H * W
    up = torch.randn(shape, device=dev, generator=g)
    extra = {}
    if kind == "step":
        E0 = (torch.rand(shape, device=dev, generator=g) * 30 - 5).requires_grad_()
        G = (torch.randn(shape, device=dev, generator=g) * 5).requires_grad_()
        M = torch.randn((L, L), device=dev, generator=g).requires_grad_()
        leaves = (E0, G, M)

        def fused():
            phl.nchw_step_train_fn(E0, G, M).backward(up)

        def plain():
            F.conv2d(F.softmax(-(E0 + G), dim=1), M.t()[..., None, None]).backward(up)

        moved = 7 * L * n * 4
    else:
        logits = (torch.randn(shape, device=dev, generator=g) * 2).requires_grad_()
        guide = torch.rand((1, 1, H, W), device=dev, generator=g).requires_grad_()
        labels = torch.arange(L, dtype=torch.float32, device=dev)
        nets = [CRFasRNN(charb(.05), niters=5, fused_grad=True, fused_step=flag).to(dev) for flag in (True, False)]
        leaves = (logits, guide) + tuple(p for net in nets for p in net.parameters())

        def step(net):
            (net(guide, logits, labels=labels) * up).sum().backward()

        fused, plain = (lambda: step(nets[0])), (lambda: step(nets[1]))
        moved = None

    def clear():
        for t in leaves:
            t.grad = None

    def cleared(fn):
        def f():
            clear()
            fn()
        return f

    (hip, hip_min, hip_max), (tor, tor_min, tor_max) = _time([cleared(fused), cleared(plain)], reps)
    peaks = dict(fused_peak_MiB=round(_peak(fused, clear), 1), plain_peak_MiB=round(_peak(plain, clear), 1))
    if moved is not None:
        gbs = moved / hip / 1e6
        extra = dict(GBps=round(gbs, 1), of_copy=round(gbs / rate, 3))
    print(json.dumps(dict(case=name, fused_ms=round(hip, 4), fused_min_ms=round(hip_min, 4), fused_max_ms=round(hip_max, 4),
                          plain_ms=round(tor, 4), plain_min_ms=round(tor_min, 4), plain_max_ms=round(tor_max, 4),
                          speedup=round(tor / hip, 2), **peaks, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print(" ".join(CASES))
        return
    rate = copy_rate(torch.device("cuda", 0))
    print(json.dumps(dict(stream_copy_GBps=round(rate, 1))), flush=True)
    for name in ([a.only] if a.only else CASES):
        run(name, a.reps, rate)


if __name__ == "__main__":
    main()
