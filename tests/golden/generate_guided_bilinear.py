#!/usr/bin/env python3
"""Generate tests/golden/guided_bil_*.npz: the reference's FastGuidedFilter / BatchedGuidedAdjacency with
``mode='bilinear'``, run in float64 on the CPU.

Build container only (needs the reference tree); tests only ever read the committed .npz arrays.  The shim, the stored
arrays and the part size are those of generate_guided.py (its helpers are imported): ``gm.BoxFilter = gm.mBoxFilter``, 8-bit
uniform noise inputs, ``omega`` as the reference initialised it, the float64 output in parts along the channel axis.

The reference asserts h > 2r + 1 at the low resolution with the full r; the three cases pass it.  While writing, every
case is required to equal the repository's torch form (crf/guided.py, float64, omega copied) bit for bit.
"""
import os

import numpy as np
import torch

import generate_guided as gg       # (puts tests/ on sys.path for the import below)

from _guided_fixtures import BIL_CASES, build_module, load_case  # noqa: E402


def main():
    torch.set_num_threads(1)
    _, gm = gg.gen.import_reference_python()
    gm.BoxFilter = gm.mBoxFilter
    guided = gg.repo_guided()
    rng = np.random.default_rng(2025)

    filters = [  # name, class, cx, r, eps, s, y shape
        ("bil_fast_r9_s2", "FastGuidedFilter", 3, 9, 1e-2, 2, (2, 4, 49, 67)),
        ("bil_bga_cx1_s3", "BatchedGuidedAdjacency", 1, 4, 1e-2, 3, (1, 3, 41, 67)),
        ("bil_bga_cx3_s2", "BatchedGuidedAdjacency", 3, 4, 1e-2, 2, (1, 3, 40, 56)),
    ]
    assert [f[0] for f in filters] == BIL_CASES
    for name, kind, cx, r, eps, s, shape in filters:
        mod = getattr(gm, kind)(cx, r, eps, subsample_ratio=s, mode="bilinear")
        omega = mod.omega.detach().numpy().copy()            # fp32, as the reference initialised it
        y_u8 = gg.noise_u8(rng, shape)
        x_u8 = gg.noise_u8(rng, (shape[0], cx) + shape[2:])
        with torch.no_grad():
            out = mod.double()(gg.as_f64(y_u8), gg.as_f64(x_u8))
        gg.save(name, out.numpy(), kind=np.array(kind), cx=np.int64(cx), r=np.int64(r), s=np.int64(s), eps=np.float64(eps),
                omega=omega, y_u8=y_u8, x_u8=x_u8, mode=np.array("bilinear"))
        z = load_case(name)
        with torch.no_grad():
            mine = build_module(guided, z, torch.float64, "cpu", "bilinear")(torch.from_numpy(z["y"]).double(), torch.from_numpy(z["x"]).double())
        diff = float((mine - out).abs().max())
        print(f"{name}: |out| <= {float(out.abs().max()):.4g}, repository torch form vs reference: {diff}")
        assert diff == 0.0, name
    sizes = {f: os.path.getsize(os.path.join(gg.HERE, f)) for f in sorted(os.listdir(gg.HERE)) if f.startswith("guided_bil_")}
    print(sizes)
    assert max(sizes.values()) <= 1 << 20


if __name__ == "__main__":
    main()
