"""Golden vectors for the wide compatibility kernel (256 < L <= 512): the flat mean field at L = 341, the reference's own
label count at 2048 columns (max_disp = w // 6, crf/depth.py:40), on a Tsukuba crop, computed by the reference's
``mean_field_infer`` (crf_module.py:41-53) over the reference engine -- the same recipe as generate.py's round4b case,
whose helpers this script imports (generate.py itself is not changed).

    python tests/golden/generate_wide.py      -> tests/golden/meanfield_tsukuba_L341.npz

The crop is 20 x 33 = 660 pixels: not a multiple of the kernel's 64-pixel tile, so the tail rows are covered.  E_0 is
rounded to float16 first and stored as float16, so the stored input is exact.  Mu is the Charbonnier compatibility
(gamma = 3); Q and the expected disparity are stored after 1, 5 and 10 iterations (10 = the reference's default)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate as gen  # noqa: E402


def meanfield_L341():
    import torch

    torch.manual_seed(3)
    torch.set_num_threads(1)
    crf_module, gm = gen.import_reference_python()
    imL = gen.read_image(os.path.join(gen.REFERENCE, "Experiments", "imL.png"))
    imR = gen.read_image(os.path.join(gen.REFERENCE, "Experiments", "imR.png"))
    H, W_ = imL.shape[:2]
    position = np.mgrid[:H, :W_].transpose((1, 2, 0)) / np.sqrt(H ** 2 + W_ ** 2)
    L, sigma_c, sigma_p, gamma = 341, 0.1, 0.1, 3
    r0, c0, h, w = 150, 300, 20, 33
    full = gen.disparity_badness(imL, imR, L)
    E0_np = full[r0:r0 + h, c0:c0 + w].reshape(-1, L).astype(np.float16).astype(np.float32)
    E0 = torch.from_numpy(E0_np)
    refimg = np.zeros((h, w, 5))
    refimg[..., :3] = imL[r0:r0 + h, c0:c0 + w] / sigma_c
    refimg[..., 3:] = position[r0:r0 + h, c0:c0 + w] / sigma_p
    flat_ref = torch.from_numpy(refimg.reshape(h * w, -1).astype(np.float32))
    labels = torch.arange(L).float()
    Mu = crf_module.compatibility_matrix(lambda a, b: crf_module.charbonneir(a, b, gamma), labels)
    Wop = gm.LatticeGaussian(flat_ref)
    out = dict(E0_f16=E0_np.astype(np.float16), ref=flat_ref.numpy(), labels=labels.numpy(), gamma=np.float32(gamma),
               h=np.int64(h), w=np.int64(w))
    with torch.no_grad():
        for it in (1, 5, 10):
            Q = crf_module.mean_field_infer(E0, Wop, Mu, it)
            out[f"Q{it}"] = Q.numpy()
            out[f"disp{it}"] = (Q @ labels).numpy()
    path = os.path.join(HERE, "meanfield_tsukuba_L341.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"n={h * w} L={L}")


if __name__ == "__main__":
    assert gen.po.build_reference(), "reference engine not built"
    meanfield_L341()
