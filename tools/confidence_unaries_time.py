"""Time the confidence-weighted unaries (phl.nchw_confidence_unaries / phl.NchwConfidenceUnaries, phl_nchw_conf.hip) against
the torch line they replace, ``-logits * confidence``, on one GPU in one process.

    python tools/confidence_unaries_time.py [--reps N] [--only NAME] [--list]

Logits [1, L, 1110, 1390] and a confidence [1, 1, 1110, 1390], for L = 18 and 64:
  fwd_*     E0 without autograd: the kernel against the torch line.
  fwdbwd_*  the same with a confidence that asks for a gradient (CRFwUncertainty's), each followed by ``.backward(g)`` with
            a fixed g of E0's shape: phl.nchw_confidence_unaries_fn against the torch line under autograd.  peak_MiB is
            torch.cuda.max_memory_allocated over one such pair, above what was allocated before it (the inputs and g).
  head_*    one training step of CRFwUncertainty(fused_grad=True, fused_step=True) -- an L1 loss, backward -- with
            fused_unaries on against off, the same parameters and inputs.
Event-timed after five warm-up calls of each path (clocks and code objects up); the two paths alternate, call by call;
the median of --reps (default 15) calls of each is reported, with the fastest and the slowest beside it as the spread.
"of_copy" is the time over that of phl.stream_copy moving the bytes the kernels must move, in the same process: the
forward reads the logits and the confidence and writes E0, (2 L + 1) n 4 bytes; the backward reads the logits and g and
writes the confidence's gradient, 2 L n 4 + n 4 bytes -- twice the forward's bytes for the pair.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

import phl  # noqa: E402

H, W = 1110, 1390
CASES = {f"{kind}_{L}x{H}x{W}": (kind, L) for kind in ("fwd", "fwdbwd") for L in (18, 64)}
CASES[f"head_18x{H}x{W}"] = ("head", 18)


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


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _head(L, dev, g, reps):
    from crf.mb_stereo_crf import CRFwUncertainty

    logits = torch.randn((1, L, H, W), device=dev, generator=g) * 2
    img = torch.rand((1, 3, H, W), device=dev, generator=g)
    feats = torch.randn((1, 64, H, W), device=dev, generator=g)
    torch.manual_seed(0)
    new = CRFwUncertainty(fused_grad=True, fused_step=True, fused_unaries=True).to(dev)
    old = copy.deepcopy(new)
    old.CRF.fused_unaries = False

    def step(net):
        def f():
            net.zero_grad(set_to_none=True)
            depth, _ = net((logits, img, feats))
            (depth - (-1.0)).abs().mean().backward()
        return f

    times = _time([step(new), step(old)], reps)
    return times, dict(hip_peak_MiB=round(_peak(step(new)), 1), torch_peak_MiB=round(_peak(step(old)), 1))


def run(name, reps):
    kind, L = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    extra = {}
    if kind == "head":
        ((hip, hip_min, hip_max), (tor, tor_min, tor_max)), extra = _head(L, dev, g, reps)
    else:
        logits = torch.randn((1, L, H, W), device=dev, generator=g) * 2
        conf = torch.rand((1, 1, H, W), device=dev, generator=g) * 3
        words = (2 * L + 1) * H * W // 2 // 4 * 4                 # a copy of `words` floats moves (2 L + 1) n 4 bytes
        src, dst = torch.empty(words, device=dev), torch.empty(words, device=dev)
        passes = 1 if kind == "fwd" else 2
        copy_ms = passes * _time([lambda: phl.stream_copy(dst, src)], reps)[0][0]
        del src, dst
        if kind == "fwd":
            with torch.no_grad():
                (hip, hip_min, hip_max), (tor, tor_min, tor_max) = _time(
                    [lambda: phl.nchw_confidence_unaries(logits, conf), lambda: -logits * conf], reps)
        else:
            up = torch.randn((1, L, H, W), device=dev, generator=g)
            conf.requires_grad_()

            def hip_pair():
                conf.grad = None
                phl.nchw_confidence_unaries_fn(logits, conf).backward(up)

            def torch_pair():
                conf.grad = None
                (-logits * conf).backward(up)

            (hip, hip_min, hip_max), (tor, tor_min, tor_max) = _time([hip_pair, torch_pair], reps)
            extra = dict(hip_peak_MiB=round(_peak(hip_pair), 1), torch_peak_MiB=round(_peak(torch_pair), 1))
        extra.update(copy_ms=round(copy_ms, 4), hip_of_copy=round(hip / copy_ms, 2), torch_of_copy=round(tor / copy_ms, 2),
                     copy_TBps=round(passes * (2 * L + 1) * H * W * 4 / copy_ms / 1e9, 2))
    extra["volume_MiB"] = round(L * H * W * 4 / 2 ** 20, 1)
    print(json.dumps(dict(case=name, hip_ms=round(hip, 4), hip_min_ms=round(hip_min, 4), hip_max_ms=round(hip_max, 4),
                          torch_ms=round(tor, 4), torch_min_ms=round(tor_min, 4), torch_max_ms=round(tor_max, 4),
                          speedup=round(tor / hip, 3), difference_ms=round(tor - hip, 4),
                          exceeds_both_spreads=bool(tor - hip > max(hip_max - hip_min, tor_max - tor_min)), **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
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
