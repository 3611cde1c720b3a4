"""Time forward + backward of LatticeFilter with a guide of 8 or 16 feature dimensions: the fused backward in feature
groups (phl_filter_grad, d <= 16) against the same call under PHL_FUSED_GRAD=0, which filters the reference's
2L(1+d)-channel operand -- exactly the route these d took before the feature groups.  Same GPU, one process.

    python tools/filter_grad_highd_time.py [--reps N] [--only NAME] [--list]

Event-timed after one warm-up of each path (the warm-up also builds and caches the lattice, which both paths share); the
two paths alternate, step by step, and each keeps the best of its --reps (default 3) steps.  A step is
``LatticeFilter.apply(src, ref)`` and a backward with gradients for src and ref, L = 64 channels.  ``*_MiB`` is
torch.cuda.max_memory_allocated over one step of that path beyond what was allocated before it (the inputs).  The
library's own memory (vertex and partial rows: not torch's) is reported beside it as ``*_lattice_MiB``:
Lattice.device_bytes after that path's first step, i.e. the lattice's tables plus the largest workspace so far -- the
fused step runs first, so the fused figure is its own and the wide figure is the larger of the two.  A path that runs
out of memory is reported as null.
The guide is image-like (the pixel grid / 4 and sines, times ``scale``): ``staged_splat`` and ``M_per_n`` say what
lattice that gave, and ``fused_taken`` whether phl_filter_grad took the call (false: both columns time the wide operand).
Every case is a separate `timeout`-guarded step when driven from a shell loop:
`for n in $(python tools/filter_grad_highd_time.py --list); do timeout -k 10 600 python tools/filter_grad_highd_time.py --only $n || break; done`.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))

import phl  # noqa: E402
import crf.gaussian_matrix as gm  # noqa: E402

L = 64
# name: (d, H, W, scale of the guide)
CASES = {
    "d8_288x384": (8, 288, 384, 1.0),
    "d16_288x384": (16, 288, 384, 0.5),
    "d8_1110x1390": (8, 1110, 1390, 1.0),
    "d16_1110x1390": (16, 1110, 1390, 0.5),
    "d8_1536x2048": (8, 1536, 2048, 1.0),
    "d16_1536x2048": (16, 1536, 2048, 0.5),
}


def _guide(d, H, W, scale, dev):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev),
                            indexing="ij")
    cols = [xx.reshape(-1) / 4, yy.reshape(-1) / 4] + [torch.sin(xx.reshape(-1) / (7 + 3 * k)) * 2 for k in range(d - 2)]
    return (torch.stack(cols, 1) * scale).contiguous()


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
    d, H, W, scale = CASES[name]
    dev = torch.device("cuda", 0)
    n = H * W
    gen = torch.Generator(device=dev).manual_seed(0)
    ref = _guide(d, H, W, scale, dev).requires_grad_(True)
    src = torch.rand((n, L), device=dev, generator=gen, requires_grad=True)
    up = torch.randn((n, L), device=dev, generator=gen)
    lat = phl.lattice_for(ref.detach())
    st = lat.tile_stats(L)
    tables = lat.device_bytes / 2 ** 20

    widths, real = [], gm.latticefilter
    gm.latticefilter = lambda s, r: (widths.append(int(s.shape[-1])), real(s, r))[1]      # which operands get filtered

    def step(fused):
        os.environ["PHL_FUSED_GRAD"] = "1" if fused else "0"
        src.grad = ref.grad = None
        del widths[:]
        gm.LatticeFilter.apply(src, ref).backward(up)
        return 2 * L * (1 + d) not in widths

    taken = step(True)          # (false: phl_filter_grad declined the shape and the wide operand was filtered)
    best, peak, ws = {True: float("inf"), False: float("inf")}, {}, {}
    for flag in (True, False):
        try:
            peak[flag] = _peak(lambda: step(flag))          # (also the warm-up)
            ws[flag] = lat.device_bytes / 2 ** 20
        except (torch.cuda.OutOfMemoryError, phl.PhlError) as e:
            print(f"# {name} fused={flag}: {type(e).__name__}: {str(e)[:200]}", file=sys.stderr)
            best[flag] = peak[flag] = ws[flag] = None
            src.grad = ref.grad = None
            torch.cuda.empty_cache()
    for _ in range(reps):
        for flag in (True, False):
            if best[flag] is not None:
                best[flag] = min(best[flag], _once(lambda: step(flag)))
    rnd = lambda v, k: None if v is None else round(v, k)  # noqa: E731
    both = best[True] is not None and best[False] is not None
    print(json.dumps(dict(case=name, d=d, L=L, pixels=n, M_per_n=round(lat.M / n, 3), staged_splat=st["staged_splat"],
                          fused_taken=taken, fused_ms=rnd(best[True], 3), wide_ms=rnd(best[False], 3),
                          speedup=round(best[False] / best[True], 2) if both else None, fused_MiB=rnd(peak[True], 1),
                          wide_MiB=rnd(peak[False], 1), tables_MiB=round(tables, 1), fused_lattice_MiB=rnd(ws[True], 1),
                          wide_lattice_MiB=rnd(ws[False], 1),
                          wide_operand_MiB=round(n * 2 * L * (1 + d) * 4 / 2 ** 20, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
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
