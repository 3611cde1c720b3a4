#!/usr/bin/env python3
"""Generate tests/golden/guided_bil_grad_*.npz: the gradients of the reference's FastGuidedFilter /
BatchedGuidedAdjacency with ``mode='bilinear'``, float64 autograd on the CPU.

Build container only (needs the reference tree); tests only ever read the committed .npz arrays.  Everything is done as
generate_guided_grad.py does it for the nearest mode: the committed inputs and ``omega`` of guided_bil_<case>.npz are
read back (not drawn again), the upstream gradient is g = k / 127 from seeded int8 noise (exact in the file), and the
gradients of sum(out * g) with respect to y, x and omega are saved: guided_bil_grad_<case>.npz holds g_i8 and
grad_omega; grad_y and grad_x are split along the channel axis into guided_bil_grad_<case>_gy<k>.npz / _gx<k>.npz, each
below the size limit of a committed file.

While writing, the repository's torch form (crf/guided.py, float64) is run on the same data and its largest difference
from the reference, relative to each gradient's largest magnitude, is printed (tests/test_guided_bilinear_grad_cpu.py
bounds it).
"""
import os

import numpy as np
import torch

import generate_guided as gg       # (puts tests/ on sys.path for the import below)

from _guided_fixtures import BIL_CASES, _stem, fixture_grads, load_case, load_grad_case  # noqa: E402


def save_parts(stem, key, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    per = max(1, gg.PART_BYTES // arr[:, :1].nbytes)
    for k, c0 in enumerate(range(0, arr.shape[1], per)):
        np.savez_compressed(os.path.join(gg.HERE, f"{stem}_{key}{k}.npz"), grad=arr[:, c0:c0 + per])


def main():
    torch.set_num_threads(1)
    _, gm = gg.gen.import_reference_python()
    gm.BoxFilter = gm.mBoxFilter
    guided = gg.repo_guided()
    rng = np.random.default_rng(2026)
    for name in BIL_CASES:
        stem = _stem(name)
        for f in os.listdir(gg.HERE):
            if f.startswith(stem + "_g") or f == stem + ".npz":
                os.remove(os.path.join(gg.HERE, f))
        z = load_case(name)
        kind, cx, r, s = str(z["kind"]), int(z["cx"]), int(z["r"]), int(z["s"])
        mod = getattr(gm, kind)(cx, r, float(z["eps"]), subsample_ratio=s, mode="bilinear")
        assert np.array_equal(mod.omega.detach().numpy(), z["omega"])
        mod = mod.double()
        mod.omega = torch.nn.Parameter(torch.from_numpy(z["omega"]).double())    # (the reference's is an expanded scalar)
        g_i8 = rng.integers(-127, 128, size=z["y"].shape, dtype=np.int8)
        g = torch.from_numpy((g_i8.astype(np.float32) / np.float32(127.0)).astype(np.float32)).double()
        y = torch.from_numpy(z["y"]).double().requires_grad_(True)
        x = torch.from_numpy(z["x"]).double().requires_grad_(True)
        (mod(y, x) * g).sum().backward()
        np.savez_compressed(os.path.join(gg.HERE, stem + ".npz"), g_i8=g_i8, grad_omega=mod.omega.grad.numpy())
        save_parts(stem, "gy", y.grad.numpy())
        save_parts(stem, "gx", x.grad.numpy())
        zz = load_grad_case(name, stem)
        mine = fixture_grads(guided, zz, torch.float64, "cpu", "bilinear")
        gaps = {k: float(np.abs(m.numpy() - zz["grad_" + k]).max() / np.abs(zz["grad_" + k]).max())
                for k, m in zip(("y", "x", "omega"), mine)}
        print(f"{name}: repository torch form vs reference, relative to each gradient's largest magnitude: {gaps}")
    sizes = {f: os.path.getsize(os.path.join(gg.HERE, f)) for f in sorted(os.listdir(gg.HERE)) if f.startswith("guided_bil_grad_")}
    print(sizes)
    assert max(sizes.values()) <= 1 << 20


if __name__ == "__main__":
    main()
