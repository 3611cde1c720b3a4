#!/usr/bin/env python3
"""Generate tests/golden/guided_*.npz: the reference's box-window guided-filter classes, run in float64 on the CPU.

Build container only (needs the reference tree); tests only ever read the committed .npz arrays.

Shim.  ``generate.import_reference_python()`` imports the reference's crf/gaussian_matrix.py with an empty placeholder for
the absent pip package ``guided_filter_pytorch``.  This script then binds the reference's OWN box sum to the name the
guided classes use:  ``gm.BoxFilter = gm.mBoxFilter``  (gaussian_matrix.py:52-65: a zero-padded (2r+1)^2 window sum, the
function guided_filter_pytorch.BoxFilter computes).  Everything else is the reference's code as it stands.

Stored per case: the inputs (8-bit uniform noise k / 255 or a Tsukuba crop, logits rounded to float16: exact in the file),
the module's ``omega`` as the reference initialised it (its fp32 log(exp(eps) - 1), before .double()), r, s, and the
float64 output, split along the channel axis into parts below the size limit of a committed file.

``GuidedAdjacency`` exists only as comments in the reference (gaussian_matrix.py:275-283).  The mean-field case builds
it from the reference's GuidedFilter and the commented formula, (filtered * .5 * (2r+1)^2 - img_U) pixel-major; the
commented constructor's ``super().__init__(r, eps)`` is read as (channels, r, eps).

While writing, every filter case is required to equal the repository's torch form (crf/guided.py, float64, omega
copied) bit for bit.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import generate as gen  # noqa: E402
from _guided_fixtures import build_module, load_case  # noqa: E402

PART_BYTES = 900 << 10


def repo_guided():
    sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))
    spec = importlib.util.spec_from_file_location("repo_crf_guided", os.path.join(ROOT, "depth-estimation_amd", "crf", "guided.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(name, out, **arrays):
    for f in os.listdir(HERE):
        if f.startswith(f"guided_{name}_out") or f == f"guided_{name}.npz":
            os.remove(os.path.join(HERE, f))
    np.savez_compressed(os.path.join(HERE, f"guided_{name}.npz"), **arrays)
    out = np.ascontiguousarray(out, dtype=np.float64)
    per = max(1, PART_BYTES // (out[:, :1].nbytes))
    for k, c0 in enumerate(range(0, out.shape[1], per)):
        np.savez_compressed(os.path.join(HERE, f"guided_{name}_out{k}.npz"), out=out[:, c0:c0 + per])


def noise_u8(rng, shape):
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


def as_f64(u8):
    return torch.from_numpy((u8.astype(np.float32) / np.float32(255.0)).astype(np.float32)).double()


def tsukuba_crop():
    img = gen.read_image(os.path.join(gen.REFERENCE, "Experiments", "imL.png"))
    return np.ascontiguousarray(img[96:96 + 48, 150:150 + 64].transpose(2, 0, 1)[None]).astype(np.float32)   # [1, 3, 48, 64]


def main():
    torch.set_num_threads(1)
    crf_module, gm = gen.import_reference_python()
    gm.BoxFilter = gm.mBoxFilter
    guided = repo_guided()
    rng = np.random.default_rng(2024)

    filters = [  # name, class, cx, r, eps, s, y shape
        ("gf_r4", "GuidedFilter", 3, 4, 1e-2, 1, (2, 4, 48, 64)),
        ("fast_r9_s2", "FastGuidedFilter", 3, 9, 1e-2, 2, (2, 4, 49, 67)),
        ("bga_r20", "BatchedGuidedAdjacency", 1, 20, 1e-5, 2, (1, 16, 96, 128)),
        ("bga_cx16", "BatchedGuidedAdjacency", 16, 4, 1e-2, 2, (1, 3, 40, 56)),
        ("fast_r1_s2", "FastGuidedFilter", 3, 1, 1e-2, 2, (1, 4, 21, 30)),
        ("gf_tsukuba", "GuidedFilter", 3, 4, 1e-2, 1, (1, 4, 48, 64)),
    ]
    for name, kind, cx, r, eps, s, shape in filters:
        kw = {} if kind == "GuidedFilter" else {"subsample_ratio": s}
        mod = getattr(gm, kind)(cx, r, eps, **kw)
        omega = mod.omega.detach().numpy().copy()            # fp32, as the reference initialised it
        y_u8 = noise_u8(rng, shape)
        arrays = dict(kind=np.array(kind), cx=np.int64(cx), r=np.int64(r), s=np.int64(s), eps=np.float64(eps), omega=omega, y_u8=y_u8)
        if name == "gf_tsukuba":
            x = torch.from_numpy(tsukuba_crop()).double()
            arrays["x"] = x.float().numpy()
        else:
            x_u8 = noise_u8(rng, (shape[0], cx) + shape[2:])
            arrays["x_u8"] = x_u8
            x = as_f64(x_u8)
        with torch.no_grad():
            out = mod.double()(as_f64(y_u8), x)
        save(name, out.numpy(), **arrays)
        z = load_case(name)
        with torch.no_grad():
            mine = build_module(guided, z, torch.float64, "cpu")(torch.from_numpy(z["y"]).double(), torch.from_numpy(z["x"]).double())
        diff = float((mine - out).abs().max())
        print(f"{name}: |out| <= {float(out.abs().max()):.4g}, repository torch form vs reference: {diff}")
        assert diff == 0.0, name

    # ---- CRFasRNN with its default W (crf_module.py:81-104) -----------------------------------------------------------
    L, h, w = 16, 96, 128
    logits = (rng.standard_normal((1, L, h, w)) * 2.0).astype(np.float16)
    g_u8 = noise_u8(rng, (1, 1, h, w))
    labels = torch.arange(L).float()
    net = crf_module.CRFasRNN(crf_module.charb(3.0), niters=3)
    omega = net.W.omega.detach().numpy().copy()
    with torch.no_grad():
        out = net.double()(as_f64(g_u8), torch.from_numpy(logits.astype(np.float32)).double(), labels=labels.double())
    save("crfasrnn_guided", out.numpy(), logits_f16=logits, x_u8=g_u8, omega=omega, labels=labels.numpy(), gamma=np.float64(3.0),
         niters=np.int64(3), r=np.int64(20), s=np.int64(2), eps=np.float64(1e-5))
    print("crfasrnn_guided:", tuple(out.shape), float(out.abs().max()))

    # ---- flat mean field over a GuidedAdjacency (see the header) -----------------------------------------------------
    class GuidedAdjacency(gm.GuidedFilter):
        """W @ U for pixel-major U [n, L]: the reference's filter on the label planes, times (2r+1)^2 / 2, minus U."""

        def __init__(self, guide, radius, epsilon):
            super().__init__(guide.shape[1], radius, epsilon)
            self.guide = guide

        def __matmul__(self, U):
            n, L = U.shape
            height, width = self.guide.shape[2:]
            planes = U.t().reshape(1, L, height, width)
            weight = 0.5 * (2 * self._r + 1) ** 2
            product = self(planes, self.guide) * weight - planes
            return product.reshape(L, n).t()

    mf = np.load(os.path.join(HERE, "meanfield_tsukuba_crop.npz"))           # E0 and Mu of the same 48 x 64 crop, L = 16
    guide = torch.from_numpy(tsukuba_crop())
    r, eps = 4, 1e-2
    Wop = GuidedAdjacency(guide.double(), r, eps)
    omega = Wop.omega.detach().numpy().copy()
    with torch.no_grad():
        Q = crf_module.mean_field_infer(torch.from_numpy(mf["E0"]).double(), Wop.double(), torch.from_numpy(mf["Mu"]).double(), 3)
    save("meanfield_guided", Q.numpy(), E0=mf["E0"], Mu=mf["Mu"], x=guide.numpy(), omega=omega, r=np.int64(r), eps=np.float64(eps),
         niters=np.int64(3))
    print("meanfield_guided:", tuple(Q.shape))
    sizes = {f: os.path.getsize(os.path.join(HERE, f)) for f in sorted(os.listdir(HERE)) if f.startswith("guided_")}
    print(sizes)
    assert max(sizes.values()) <= 1 << 20


if __name__ == "__main__":
    main()
