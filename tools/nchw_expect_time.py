"""Time the expected-label head (phl.nchw_expected_value / phl.NchwExpectedValue, phl_nchw_expect.hip) against the torch
form it replaces, on one GPU in one process.

    python tools/nchw_expect_time.py [--reps N] [--only NAME] [--list]

At [1, L, 1110, 1390] for L = 18, 64 and 231, with a linspace of labels:
  fwd_*     ``(softmax(-(E0 + G), 1) * labels).sum(1, keepdim=True)`` without autograd -- the loop's last step: the kernel
            on E0 and G (negate=True) against fp32 torch on the logits ``-(E0 + G)`` it would first have to write
            (phl.nchw_softmax_compat(logits=True), timed with it).  GB/s = the (2 L + 1) * n * 4 bytes the kernel must move.
  fwdbwd_*  forward + backward from logits that ask for a gradient (the training form): phl.nchw_expected_value_fn against
            the torch lines under autograd, each followed by ``.backward(g)``.  Bytes the pair must move: L * n * 4 read in
            the forward, 2 * L * n * 4 read and L * n * 4 written in the backward (the column is read twice).
Event-timed after five warm-up calls of each path (clocks and code objects up); the two paths alternate, call by call;
the median of --reps (default 31) calls of each is reported, with the fastest and the slowest beside it as the spread.
"of copy" is the kernel's rate over phl.stream_copy's in the same process.  Drive the cases as separate steps, each under
its own time limit, with the project's session script:
`bash tools/session.sh fwd_18 'python tools/nchw_expect_time.py --only fwd_18x1110x1390' fwd_64 '...'` (names: --list).
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

H, W = 1110, 1390
CASES = {f"{kind}_{L}x{H}x{W}": (kind, L) for kind in ("fwd", "fwdbwd") for L in (18, 64, 231)}


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


def copy_rate(dev):
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty_like(a)
    ms = _time([lambda: phl.stream_copy(b, a)], 5)[0][0]
    return 2 * a.numel() * 4 / ms / 1e6


def _torch_form(logits, lab4):
    return (F.softmax(logits, dim=1) * lab4).sum(1, keepdim=True)


def run(name, reps, rate):
    kind, L = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    E0 = torch.rand((1, L, H, W), device=dev, generator=g) * 30 - 5
    labels = torch.linspace(0, 40, L, device=dev)
    lab4 = labels[None, :, None, None]
    n = H * W
    if kind == "fwd":
        G = torch.randn((1, L, H, W), device=dev, generator=g) * 5
        out = torch.empty((1, 1, H, W), device=dev)
        with torch.no_grad():
            (hip, hip_min, hip_max), (tor, tor_min, tor_max) = _time(
                [lambda: phl.nchw_expected_value(E0, G, labels, negate=True, out=out),
                 lambda: _torch_form(phl.nchw_softmax_compat(E0, G, logits=True), lab4)], reps)
        moved = (2 * L + 1) * n * 4
    else:
        up = torch.randn((1, 1, H, W), device=dev, generator=g)
        leaf = E0.clone().requires_grad_()

        def hip_pair():
            leaf.grad = None
            phl.nchw_expected_value_fn(leaf, None, labels, False).backward(up)

        def torch_pair():
            leaf.grad = None
            _torch_form(leaf, lab4).backward(up)

        (hip, hip_min, hip_max), (tor, tor_min, tor_max) = _time([hip_pair, torch_pair], reps)
        moved = (4 * L + 2) * n * 4
    gbs = moved / hip / 1e6
    print(json.dumps(dict(case=name, hip_ms=round(hip, 4), hip_min_ms=round(hip_min, 4), hip_max_ms=round(hip_max, 4),
                          torch_ms=round(tor, 4), torch_min_ms=round(tor_min, 4), torch_max_ms=round(tor_max, 4),
                          speedup=round(tor / hip, 2), GBps=round(gbs, 1), of_copy=round(gbs / rate, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
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
