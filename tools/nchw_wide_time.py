"""Time the channel-major mean-field step for a general Mu above 256 labels (phl.nchw_softmax_compat_wide, k_nchw_tile on
its 32-pixel tile, phl_nchw.hip) against the torch ops it replaces, and a whole CRFasRNN forward with and without it, on
one GPU in one process.

    python tools/nchw_wide_time.py [--reps N] [--only NAME] [--list]

Event-timed after one warm-up call of each path; the two paths alternate, call by call, and each keeps the best of its
--reps (default 5) calls.  Shapes: [1, 341, 1536, 2048] (the reference's label count at 2048 columns, max_disp = w // 6)
and [1, 512, 1110, 1390] (the upper edge of the kernel's range).
(a) step_*: ``Y = Mu(softmax(-(E0 + G), 1))`` with a Charbonnier Mu -- the kernel against fp32 ``F.conv2d(F.softmax(-(E0 +
    G), 1), Mu.t()[..., None, None])``, the form the plain loop runs.  GB/s = the 3 * B*L*n*4 bytes the kernel must move
    (E0 and G read, Y written) over its time; floor_ms is that volume at phl.stream_copy's rate in the same process (the
    copy-rate floor of three sweeps), "of copy" the kernel's rate over it.
(b) crf5_*: one no-grad ``CRFasRNN(charb(.05), niters=5)`` forward with the fused step (PHL_NCHW_STEP on) and with the
    plain loop (off: the module switch behind the variable).
Event times include launch gaps.  Every case is a separate `timeout`-guarded step when driven from a shell loop:
`for n in $(python tools/nchw_wide_time.py --list); do timeout -k 10 300 python tools/nchw_wide_time.py --only $n || break; done`.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

import phl  # noqa: E402
from crf import crf_module as cm  # noqa: E402

# name: (kind, L, H, W)
CASES = {
    "step_341x1536x2048": ("step", 341, 1536, 2048),
    "step_512x1110x1390": ("step", 512, 1110, 1390),
    "crf5_341x1536x2048": ("crf", 341, 1536, 2048),
    "crf5_512x1110x1390": ("crf", 512, 1110, 1390),
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


def _plain_loop(fn):
    was, cm._NCHW_STEP = cm._NCHW_STEP, False
    try:
        return fn()
    finally:
        cm._NCHW_STEP = was


def copy_rate(dev):
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty_like(a)
    ms = _time([lambda: phl.stream_copy(b, a)], 5)[0]
    return 2 * a.numel() * 4 / ms / 1e6


def run(name, reps, rate):
    kind, L, H, W = CASES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        if kind == "step":
            E0 = torch.rand((1, L, H, W), device=dev, generator=g) * 30 - 5
            G = torch.randn((1, L, H, W), device=dev, generator=g) * 5
            M = cm.charb(.05).to(dev).matrix(L, None, dev)
            weight = M.t()[..., None, None]
            out = torch.empty_like(E0)
            hip, tor = _time([lambda: phl.nchw_softmax_compat_wide(E0, G, M, out=out),
                              lambda: F.conv2d(F.softmax(-(E0 + G), 1), weight)], reps)
            volume = 3 * E0.numel() * 4
            gbs = volume / hip / 1e6
            row = dict(case=name, hip_ms=round(hip, 4), torch_ms=round(tor, 4), speedup=round(tor / hip, 2),
                       floor_ms=round(volume / rate / 1e6, 4), GBps=round(gbs, 1), of_copy=round(gbs / rate, 3))
        else:
            net = cm.CRFasRNN(cm.charb(.05), niters=5).to(dev)
            refs = torch.rand((1, 1, H, W), device=dev, generator=g)
            logits = torch.randn((1, L, H, W), device=dev, generator=g) * 3
            labels = torch.arange(L, dtype=torch.float32, device=dev)
            fn = lambda: net(refs, logits, labels=labels)  # noqa: E731
            on, off = _time([fn, lambda: _plain_loop(fn)], reps)
            row = dict(case=name, step_on_ms=round(on, 3), step_off_ms=round(off, 3), speedup=round(off / on, 2))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print(" ".join(CASES))
        return
    if not cm._NCHW_STEP:
        sys.exit("nchw_wide_time: PHL_NCHW_STEP=0 is set; the tool switches the loop itself")
    rate = copy_rate(torch.device("cuda", 0))
    print(json.dumps(dict(stream_copy_GBps=round(rate, 1))), flush=True)
    for name in ([a.only] if a.only else CASES):
        run(name, a.reps, rate)


if __name__ == "__main__":
    main()
