"""Time the HIP separable Gaussian (phl.box_blur / phl.box_blur_grad) against the plain-torch transcription of
crf/guided.py on the same GPU, in one process, alternating between the two.

    python tools/blur_time.py [--reps N] [--only NAME]

Cases: the notebook's cell-11 step (TestGaussianBlur.ipynb: 384x288, two axes, forward + backward, sigma = 30),
[1, 64, 1536, 2048] on each axis for sigma 5 and 30 (forward, and forward + sigma-gradient), one GuidedFilter(gaussian=True)
forward + backward at [1, 32, 1536, 2048] with an RGB guide.  GB/s = (bytes read + bytes written) / time, the bytes being
the kernel's compulsory traffic (blur: read x, write y; sigma-gradient: read v and g, write grad_x).  Event times include
launch gaps; for kernel times run the same command under `rocprofv3 --kernel-trace --stats` in a run of its own.
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


def _torch_cascade(x, r, dim):
    for _ in range(3):
        x = guided._box_torch(x, r, dim)
    return x


def _torch_grad(v, g, r, dim, sigma):
    h = v.shape[dim]
    f = (torch.arange(h, device=v.device, dtype=v.dtype) / sigma).reshape((1,) * dim + (h,) + (1,) * (v.dim() - dim - 1))
    Bg = _torch_cascade(g, r, dim)
    D = v * f * Bg - v * _torch_cascade(g * f, r, dim) + g * f * _torch_cascade(v, r, dim) - g * _torch_cascade(v * f, r, dim)
    return Bg, ((D * f).sum() - (Bg * v).sum()) / sigma


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = float("inf")
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        best = min(best, ev[0].elapsed_time(ev[1]))
    return best


def cases():
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    out = []

    e0 = torch.zeros(288, 384, device=dev)
    e0[20, 100] = 1
    target = guided.gaussian_blur(guided.gaussian_blur(e0, 20, 0), 20, 1).detach()

    def nb(hip):
        def run():
            alpha = torch.log(torch.tensor(30.0)).requires_grad_(True)
            s = torch.exp(alpha)
            if hip:
                y = guided.gaussian_blur(guided.gaussian_blur(e0, s, 0), s, 1)
            else:
                y = guided.gaussian_blur(guided.gaussian_blur(e0.cpu(), s, 0), s, 1)
            ((y - (target if hip else target.cpu())) ** 2).sum().backward()
        return run
    out.append(("notebook_cell11_384x288_s30", nb(True), nb(False), None))

    x = torch.rand((1, 64, 1536, 2048), device=dev, generator=gen)
    g = torch.randn((1, 64, 1536, 2048), device=dev, generator=gen)
    nbytes = x.numel() * 4
    for sigma in (5.0, 30.0):
        r = guided.sigma_radius(torch.tensor(sigma))
        for dim in (2, 3):
            out.append((f"fwd_64x1536x2048_dim{dim}_s{int(sigma)}", lambda r=r, dim=dim: phl.box_blur(x, r, dim),
                        lambda r=r, dim=dim: _torch_cascade(x, r, dim), 2 * nbytes))
            out.append((f"sgrad_64x1536x2048_dim{dim}_s{int(sigma)}", lambda r=r, dim=dim, s=sigma: phl.box_blur_grad(x, g, r, dim, s),
                        lambda r=r, dim=dim, s=sigma: _torch_grad(x, g, r, dim, s), 3 * nbytes))

    y = torch.rand((1, 32, 1536, 2048), device=dev, generator=gen)
    rgb = torch.rand((1, 3, 1536, 2048), device=dev, generator=gen)
    gf = guided.GuidedFilter(channels=3, r=5, eps=1e-2, gaussian=True).to(dev)

    def guided_step(hip):
        def run():
            if hip:
                gf(y, rgb).sum().backward()
            else:
                saved = guided._hip_ok
                guided._hip_ok = lambda t: False      # the torch transcription on the same GPU
                try:
                    gf(y, rgb).sum().backward()
                finally:
                    guided._hip_ok = saved
        return run
    out.append(("guided_gaussian_32x1536x2048_rgb", guided_step(True), guided_step(False), None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    a = ap.parse_args()
    for name, hip, ref, nbytes in cases():
        if a.only and a.only not in name:
            continue
        t_hip = _time(hip, a.reps)
        t_ref = None if a.hip_only else _time(ref, max(1, a.reps // 2))
        t_hip = min(t_hip, _time(hip, a.reps))          # alternate: HIP, torch, HIP
        rec = {"case": name, "hip_ms": round(t_hip, 4), "torch_ms": None if t_ref is None else round(t_ref, 3)}
        if nbytes:
            rec["hip_GBps"] = round(nbytes / t_hip / 1e6, 1)
        if t_ref is not None:
            rec["speedup"] = round(t_ref / t_hip, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
