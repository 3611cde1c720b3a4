#!/usr/bin/env python3
"""Generate tests/golden/guided_grad_*.npz: the gradients of the reference's box-window guided-filter classes, float64
autograd on the CPU.

Build container only (needs the reference tree); tests only ever read the committed .npz arrays.  The reference is
imported exactly as generate_guided.py does it (``gm.BoxFilter = gm.mBoxFilter``, see the shim note there).

Per filter case of generate_guided.py (its committed inputs and ``omega`` are read back, not drawn again): an upstream
gradient g = k / 127 from seeded int8 noise (exact in the file), and the gradients of sum(out * g) with respect to y, x
and omega.  guided_grad_<case>.npz holds g_i8 and grad_omega; grad_y and grad_x are split along the channel axis into
guided_grad_<case>_gy<k>.npz / _gx<k>.npz, each below the size limit of a committed file.

While writing, the repository's torch form (crf/guided.py, float64) is run on the same data and its largest difference
from the reference, relative to each gradient's largest magnitude, is printed (tests/test_guided_grad_cpu.py bounds it).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import generate as gen  # noqa: E402
from generate_guided import PART_BYTES, repo_guided  # noqa: E402
from _guided_fixtures import GRAD_CASES, fixture_grads, load_case, load_grad_case  # noqa: E402


def save_parts(name, key, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    per = max(1, PART_BYTES // arr[:, :1].nbytes)
    for k, c0 in enumerate(range(0, arr.shape[1], per)):
        np.savez_compressed(os.path.join(HERE, f"guided_grad_{name}_{key}{k}.npz"), grad=arr[:, c0:c0 + per])


def main():
    torch.set_num_threads(1)
    _, gm = gen.import_reference_python()
    gm.BoxFilter = gm.mBoxFilter
    guided = repo_guided()
    rng = np.random.default_rng(2025)
    for name in GRAD_CASES:
        for f in os.listdir(HERE):
            if f.startswith(f"guided_grad_{name}_g") or f == f"guided_grad_{name}.npz":
                os.remove(os.path.join(HERE, f))
        z = load_case(name)
        kind, cx, r, s = str(z["kind"]), int(z["cx"]), int(z["r"]), int(z["s"])
        kw = {} if kind == "GuidedFilter" else {"subsample_ratio": s}
        mod = getattr(gm, kind)(cx, r, float(z["eps"]), **kw)
        assert np.array_equal(mod.omega.detach().numpy(), z["omega"])
        mod = mod.double()
        mod.omega = torch.nn.Parameter(torch.from_numpy(z["omega"]).double())    # (the reference's is an expanded scalar)
        g_i8 = rng.integers(-127, 128, size=z["y"].shape, dtype=np.int8)
        g = torch.from_numpy((g_i8.astype(np.float32) / np.float32(127.0)).astype(np.float32)).double()
        y = torch.from_numpy(z["y"]).double().requires_grad_(True)
        x = torch.from_numpy(z["x"]).double().requires_grad_(True)
        (mod(y, x) * g).sum().backward()
        np.savez_compressed(os.path.join(HERE, f"guided_grad_{name}.npz"), g_i8=g_i8, grad_omega=mod.omega.grad.numpy())
        save_parts(name, "gy", y.grad.numpy())
        save_parts(name, "gx", x.grad.numpy())
        zz = load_grad_case(name)
        mine = fixture_grads(guided, zz, torch.float64, "cpu")
        gaps = {k: float(np.abs(m.numpy() - zz["grad_" + k]).max() / np.abs(zz["grad_" + k]).max())
                for k, m in zip(("y", "x", "omega"), mine)}
        print(f"{name}: repository torch form vs reference, relative to each gradient's largest magnitude: {gaps}")
    sizes = {f: os.path.getsize(os.path.join(HERE, f)) for f in sorted(os.listdir(HERE)) if f.startswith("guided_grad_")}
    print(sizes)
    assert max(sizes.values()) <= 1 << 20


if __name__ == "__main__":
    main()
