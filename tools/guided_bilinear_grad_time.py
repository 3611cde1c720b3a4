"""Time a training call (forward + backward, the gradients of y, x and omega) of BatchedGuidedAdjacency(mode='bilinear') on
the kernels (phl.GuidedFilterBilinearFn behind ``fused_bilinear=True, bilinear_grad=True``) against fp32 torch autograd of
the mode -- what the same call runs without ``bilinear_grad`` -- and against the nearest ``fused_grad`` route at the same
shape, on one GPU, in one process.  The method is that of tools/guided_bilinear_time.py.

    python tools/guided_bilinear_grad_time.py [--reps N] [--only NAME] [--no-torch] [--list] [--full-cov]

cx = 3, r = 15, eps = 1e-2, at [1, 18, 1110, 1390] and [1, 64, 1110, 1390] with subsample 2 and 4.  After one warm-up call
of each route the routes take turns, call by call, event-timed; each reports the median of its --reps (default 9) calls.
Per case one JSON line:
    bilinear_ms, nearest_ms, bilinear_over_nearest   the two kernel routes
    copy_ms, bilinear_over_copy                       phl.stream_copy over the bytes the call must move (forward: y, x and
                                                      src in, out out; backward: y, x and g in, grad_y and grad_x out),
                                                      the floor
    torch_ms, torch_over_bilinear                     fp32 torch autograd of the mode (skipped with --no-torch)
    nearest_torch_ms, nearest_torch_over_nearest      fp32 torch autograd of the nearest mode, what the nearest route ran
                                                      before ``fused_grad`` (skipped with --no-torch; no bar, reported)
    *_peak_MiB                                        torch.cuda.max_memory_allocated over one call of the route, above what
                                                      was allocated before it (inputs excluded; the output and the gradients
                                                      included); for the kernel routes plus the library's stream-ordered
                                                      temporaries of the backward, which torch's allocator does not see: the
                                                      statistics, the samples of x, one chunk of per-label planes
                                                      (phl.guided_filter_labels_per_chunk), the label sums and the fp64
                                                      plane [cx][H][W] of grad_x
The case ``crfasrnn5_18x1110x1390`` is one training step (forward + backward, no optimiser) of a 5-iteration
CRFasRNN(charb(.05), gchannels=3, r=15, mode='bilinear', fused_bilinear=True), with ``bilinear_grad`` and without
(flag_ms, torch_ms, and torch's allocator peaks of both).
--full-cov times the full-covariance model of the mode instead (``full_cov=True``; phl.GuidedFilterBilinearFullFn behind
``bilinear_full_grad=True``), at the same shapes, on the same tensors, the routes taking turns as above.  Per case:
    keyword_ms, torch_ms                              forward + backward with ``bilinear_full_grad`` and without it (fp32
                                                      torch autograd of the mode: what the call ran before the keyword)
    *_min_ms, *_max_ms, torch_spread_ms               the extremes of the --reps calls; the torch form's max - min
    faster_by_ms, meets_time_bar                      torch_ms - keyword_ms, and whether it exceeds torch_spread_ms
    keyword_peak_MiB, torch_peak_MiB, meets_memory_bar   as *_peak_MiB above (the kernel route: plus the temporaries of
                                                      the full-covariance backward), and keyword < torch
    diagonal_ms, nearest_full_ms (+ _peak_MiB)        for context, no bar: the diagonal ``bilinear_grad`` route and the
                                                      nearest ``full_cov_grad`` route
and the CRFasRNN case with ``full_cov=True, bilinear_full_grad=flag``.  One image per call and r = 15 only: more images
and other radii are not measured.
Event times include launch gaps; for per-kernel times run `rocprofv3 --kernel-trace --stats -- python
tools/guided_bilinear_grad_time.py --only NAME --no-torch` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import phl  # noqa: E402
from crf import guided  # noqa: E402
from guided_bilinear_time import CASES, CX, R, _once, _peak, _time  # noqa: E402

LOOP = "crfasrnn5_18x1110x1390"


def _train_call(m, y, x, g):
    def f():
        y.grad = x.grad = m.omega.grad = None
        (m(y, x) * g).sum().backward()
    return f


def _temps_MiB(cy, H, W, s):
    """The backward's stream-ordered temporaries of either kernel route below full resolution (phl_guided.hip: backward)."""
    hw = (H // s) * (W // s)
    chunk = phl.guided_filter_labels_per_chunk(1, cy, CX, H // s, W // s, need_y=True, need_x=True, need_eps=True)
    per = hw * (4 + 8 * (CX + 1) + 8 * CX + 24 * CX)
    once = hw * CX * (8 + 4 + 4 + 24 + 8) + 8 * CX * H * W
    return chunk, (chunk * per + once) / 2 ** 20


def run(name, reps, with_torch):
    cy, H, W, s = CASES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand((1, cy, H, W), device=dev, generator=gen).requires_grad_(True)
    x = torch.rand((1, CX, H, W), device=dev, generator=gen).requires_grad_(True)
    g = torch.rand((1, cy, H, W), device=dev, generator=gen) * 2 - 1
    bil = guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s, mode="bilinear", fused_bilinear=True, bilinear_grad=True).to(dev)
    tor = guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s, mode="bilinear", fused_bilinear=True).to(dev)
    near = guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s, fused_grad=True).to(dev)
    chunk, temps = _temps_MiB(cy, H, W, s)
    moved = (6 * cy + 3 * CX) * H * W // 2 // 4 * 4        # floats of a copy that moves as many bytes (read + write)
    a, b = torch.empty(moved, device=dev), torch.empty(moved, device=dev)
    fns = [_train_call(bil, y, x, g), _train_call(near, y, x, g), lambda: phl.stream_copy(b, a)]
    ntor = guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s).to(dev)
    fns += [_train_call(tor, y, x, g), _train_call(ntor, y, x, g)] if with_torch else []
    ms = _time(fns, reps)
    row = dict(case=name, bilinear_ms=round(ms[0], 3), nearest_ms=round(ms[1], 3), bilinear_over_nearest=round(ms[0] / ms[1], 3),
               copy_ms=round(ms[2], 3), bilinear_over_copy=round(ms[0] / ms[2], 2), labels_per_chunk=chunk)
    y.grad = x.grad = None
    row["bilinear_peak_MiB"] = round(_peak(fns[0]) + temps, 1)
    y.grad = x.grad = None
    row["nearest_peak_MiB"] = round(_peak(fns[1]) + temps, 1)
    if with_torch:
        y.grad = x.grad = None
        row.update(torch_ms=round(ms[3], 3), torch_over_bilinear=round(ms[3] / ms[0], 2), torch_peak_MiB=round(_peak(fns[3]), 1))
        y.grad = x.grad = None
        row.update(nearest_torch_ms=round(ms[4], 3), nearest_torch_over_nearest=round(ms[4] / ms[1], 2),
                   nearest_torch_peak_MiB=round(_peak(fns[4]), 1))
    print(json.dumps(row), flush=True)


def _time_all(fns, reps):
    """_time with the extremes kept: (median, min, max) of ``reps`` calls for every callable, the callables taking turns,
    after two warm-up calls each."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(_once(fn))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def _full_temps_MiB(cy, H, W, s):
    """The stream-ordered temporaries of the full-covariance backward below full resolution (phl_guided.hip: backward)."""
    hw, npairs = (H // s) * (W // s), CX * (CX + 1) // 2
    npl = npairs + 2 * CX
    chunk = phl.guided_filter_labels_per_chunk(1, cy, CX, H // s, W // s, need_y=True, need_x=True, need_eps=True, full_cov=True)
    per = hw * (4 + 8 * (CX + 1) + 8 * CX + 8 * npl)
    once = hw * (8 * CX + 8 * npairs + 4 * CX + 8 * npl + 4 * (CX + npairs)) + 8 * CX * H * W
    return chunk, (chunk * per + once) / 2 ** 20


def _stats(row, key, t):
    row.update({key + "_ms": round(t[0], 3), key + "_min_ms": round(t[1], 3), key + "_max_ms": round(t[2], 3)})


def _bars(row, key_t, tor_t):
    spread = tor_t[2] - tor_t[1]
    row.update(torch_spread_ms=round(spread, 3), faster_by_ms=round(tor_t[0] - key_t[0], 3),
               torch_over_keyword=round(tor_t[0] / key_t[0], 2), meets_time_bar=bool(tor_t[0] - key_t[0] > spread))


def run_full(name, reps, with_torch):
    cy, H, W, s = CASES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand((1, cy, H, W), device=dev, generator=gen).requires_grad_(True)
    x = torch.rand((1, CX, H, W), device=dev, generator=gen).requires_grad_(True)
    g = torch.rand((1, cy, H, W), device=dev, generator=gen) * 2 - 1
    make = lambda **kw: guided.BatchedGuidedAdjacency(CX, R, 1e-2, subsample_ratio=s, **kw).to(dev)      # noqa: E731
    key = make(mode="bilinear", fused_bilinear=True, full_cov=True, bilinear_full_grad=True)
    diag = make(mode="bilinear", fused_bilinear=True, bilinear_grad=True)
    nfull = make(full_cov=True, full_cov_grad=True)
    tor = make(mode="bilinear", fused_bilinear=True, full_cov=True)
    chunk, temps = _full_temps_MiB(cy, H, W, s)
    _, dtemps = _temps_MiB(cy, H, W, s)
    fns = [_train_call(key, y, x, g), _train_call(diag, y, x, g), _train_call(nfull, y, x, g)]
    fns += [_train_call(tor, y, x, g)] if with_torch else []
    t = _time_all(fns, reps)
    row = dict(case=name, model="full_cov", reps=reps, labels_per_chunk=chunk)
    _stats(row, "keyword", t[0])
    _stats(row, "diagonal", t[1])
    _stats(row, "nearest_full", t[2])
    for k, (fn, extra) in zip(("keyword", "diagonal", "nearest_full"), zip(fns, (temps, dtemps, temps))):
        y.grad = x.grad = None
        row[k + "_peak_MiB"] = round(_peak(fn) + extra, 1)
    if with_torch:
        _stats(row, "torch", t[3])
        _bars(row, t[0], t[3])
        y.grad = x.grad = None
        row["torch_peak_MiB"] = round(_peak(fns[3]), 1)
        row["meets_memory_bar"] = bool(row["keyword_peak_MiB"] < row["torch_peak_MiB"])
    print(json.dumps(row), flush=True)


def run_loop(reps, with_torch, full_cov=False):
    from crf.crf_module import CRFasRNN, charb

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    refs = torch.rand((1, CX, 1110, 1390), device=dev, generator=gen).requires_grad_(True)
    logits = (torch.randn((1, 18, 1110, 1390), device=dev, generator=gen) * 2).requires_grad_(True)
    up = torch.rand((1, 18, 1110, 1390), device=dev, generator=gen) * 2 - 1

    def step(net):
        def f():
            refs.grad = logits.grad = None
            net.zero_grad(set_to_none=True)
            (net(refs, logits) * up).sum().backward()
        return f

    kw = (lambda flag: dict(full_cov=True, bilinear_full_grad=flag)) if full_cov else (lambda flag: dict(bilinear_grad=flag))
    nets = [CRFasRNN(charb(.05), niters=5, r=R, gchannels=CX, mode="bilinear", fused_bilinear=True, **kw(flag)).to(dev)
            for flag in ((True, False) if with_torch else (True,))]
    fns = [step(net) for net in nets]
    if full_cov:
        t = _time_all(fns, reps)
        row = dict(case=LOOP, model="full_cov", reps=reps)
        _stats(row, "keyword", t[0])
        refs.grad = logits.grad = None
        row["keyword_torch_peak_MiB"] = round(_peak(fns[0]), 1)
        if with_torch:
            _stats(row, "torch", t[1])
            _bars(row, t[0], t[1])
            refs.grad = logits.grad = None
            row["torch_peak_MiB"] = round(_peak(fns[1]), 1)
        print(json.dumps(row), flush=True)
        return
    ms = _time(fns, reps)
    refs.grad = logits.grad = None
    row = dict(case=LOOP, flag_ms=round(ms[0], 3), flag_torch_peak_MiB=round(_peak(fns[0]), 1))
    if with_torch:
        refs.grad = logits.grad = None
        row.update(torch_ms=round(ms[1], 3), torch_over_flag=round(ms[1] / ms[0], 2), torch_peak_MiB=round(_peak(fns[1]), 1))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--full-cov", action="store_true", help="the full-covariance model: bilinear_full_grad against the torch form")
    a = ap.parse_args()
    if a.list:
        print(" ".join(list(CASES) + [LOOP]))
        return
    for name in ([a.only] if a.only else list(CASES) + [LOOP]):
        if name == LOOP:
            run_loop(a.reps, not a.no_torch, a.full_cov)
        else:
            (run_full if a.full_cov else run)(name, a.reps, not a.no_torch)


if __name__ == "__main__":
    main()
