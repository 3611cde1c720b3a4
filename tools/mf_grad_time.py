"""Timing of the differentiable mean field (CRF training) on the fused kernels against the plain autograd path.

    python tools/mf_grad_time.py --h 1110 --w 1390 --L 231 --niters 5 [--reps 3] [--no-step | --fused-only]

One JSON line with
  * stages: per-stage HIP event times (ms, best of reps) of the backward of ONE compatibility step at n = h*w pixels and
    the padded label count: dE (phl_softmax_neg_grad), gX (phl_compat_grad_x), gMu (phl_compat_mu_grad);
  * step_bwd: the whole backward of that step through phl.CompatSoftmax against torch autograd of
    softmax(-(E0 + X @ Mu)) on the same operands, same process, and their ratio;
  * train (unless --no-step): one training step -- forward + backward of ``niters`` iterations of mean_field_infer with
    E_0, Mu and the lattice guide requiring grad -- with fused_grad=True against the plain path (ms, best of reps,
    alternating), and torch.cuda.max_memory_allocated of each (GB).
--fused-only runs the fused training step alone (reps times; for a kernel trace of it).  Synthetic guide features (bench.synthetic_features), uniform random unaries, Charbonnier Mu."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))
sys.path.insert(0, ROOT)


def event_ms(fn, reps):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=1110)
    ap.add_argument("--w", type=int, default=1390)
    ap.add_argument("--L", type=int, default=231)
    ap.add_argument("--niters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()

    import bench
    import phl
    from crf.crf_module import _label_pad, charbonneir, compatibility_matrix, mean_field_infer
    from crf.gaussian_matrix import LatticeGaussian

    dev = torch.device("cuda")
    n, L = a.h * a.w, a.L
    Lp = _label_pad(L)
    g = torch.Generator(device=dev).manual_seed(0)
    res = dict(tool="mf_grad_time", h=a.h, w=a.w, n=n, L=L, L_kernel=Lp, niters=a.niters)

    if a.fused_only:
        return fused_only(a, dev, n, L, g)
    # ---- one compatibility step at the kernels' label count
    E0 = torch.rand((n, Lp), device=dev, generator=g) * 10
    X = torch.rand((n, Lp), device=dev, generator=g) - 0.3
    Mu = compatibility_matrix(lambda p, q: charbonneir(p, q, 3.0), torch.arange(Lp, dtype=torch.float32, device=dev)) * 0.05
    gout = torch.randn((n, Lp), device=dev, generator=g)
    Q = phl.compat_softmax(E0, X, Mu)
    dE = phl.softmax_neg_grad(Q, gout)
    stages = dict(dE=event_ms(lambda: phl.softmax_neg_grad(Q, gout, out=dE), a.reps),
                  gX=event_ms(lambda: phl.compat_grad_x(dE, Mu), a.reps),
                  gMu=event_ms(lambda: phl.compat_mu_grad(X, dE), a.reps))
    flop = 2.0 * n * Lp * Lp
    stages["gX_TFs"] = flop / stages["gX"] / 1e9
    stages["gMu_TFs"] = flop / stages["gMu"] / 1e9
    res["stages_ms"] = stages
    del dE

    def bwd(fused):
        e, x, m = (t.detach().requires_grad_(True) for t in (E0, X, Mu))
        out = phl.compat_softmax_fn(e, x, m) if fused else torch.softmax(-(e + x @ m), dim=1)
        return lambda: torch.autograd.grad(out, (e, x, m), gout, retain_graph=True)

    times = {}
    for fused in (True, False):
        times[fused] = event_ms(bwd(fused), a.reps)
    res["step_bwd_ms"] = dict(fused=times[True], torch=times[False], ratio=times[True] / times[False])
    del E0, X, Q, gout
    torch.cuda.empty_cache()

    # ---- one training step of niters iterations
    if not a.no_step:
        ref = torch.from_numpy(bench.synthetic_features(a.h, a.w).reshape(-1, 5)).to(dev)
        E0 = torch.rand((n, L), device=dev, generator=g) * 10
        Mu = compatibility_matrix(lambda p, q: charbonneir(p, q, 3.0), torch.arange(L, dtype=torch.float32, device=dev)) * 0.05
        gQ = torch.randn((n, L), device=dev, generator=g)

        def step(fused):
            e, m, r = (t.detach().requires_grad_(True) for t in (E0, Mu, ref))
            Qo = mean_field_infer(e, LatticeGaussian(r), m, a.niters, fused_grad=fused)
            Qo.backward(gQ)
            return e.grad, m.grad, r.grad

        train = {True: [], False: []}
        mem = {}
        for fused in (True, False):                      # warm-up (lattice builds, allocator), peak memory per path
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step(fused)
            torch.cuda.synchronize()
            mem[fused] = torch.cuda.max_memory_allocated() / 1e9
        for _ in range(a.reps):
            for fused in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(fused)
                torch.cuda.synchronize()
                train[fused].append((time.perf_counter() - t0) * 1e3)
        res["train_step_ms"] = dict(fused=min(train[True]), plain=min(train[False]), all_fused=[round(x, 1) for x in train[True]],
                                    all_plain=[round(x, 1) for x in train[False]], speedup=min(train[False]) / min(train[True]))
        res["max_memory_gb"] = dict(fused=mem[True], plain=mem[False])
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def fused_only(a, dev, n, L, g):
    import bench
    from crf.crf_module import charbonneir, compatibility_matrix, mean_field_infer
    from crf.gaussian_matrix import LatticeGaussian

    ref = torch.from_numpy(bench.synthetic_features(a.h, a.w).reshape(-1, 5)).to(dev).requires_grad_(True)
    E0 = (torch.rand((n, L), device=dev, generator=g) * 10).requires_grad_(True)
    Mu = (compatibility_matrix(lambda p, q: charbonneir(p, q, 3.0), torch.arange(L, dtype=torch.float32, device=dev)) * 0.05).requires_grad_(True)
    gQ = torch.randn((n, L), device=dev, generator=g)
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mean_field_infer(E0, LatticeGaussian(ref), Mu, a.niters, fused_grad=True).backward(gQ)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(tool="mf_grad_time", mode="fused_only", h=a.h, w=a.w, L=L, niters=a.niters, train_step_ms=ms)))


if __name__ == "__main__":
    main()
