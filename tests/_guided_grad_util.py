"""Loader of the guided-filter gradient fixtures (tests/golden/guided_grad_*.npz, written by
tests/golden/generate_guided_grad.py) and the float64 reference run of the repository's torch form."""
import glob
import os

import numpy as np

from _guided_util import GOLDEN, build_module, load_case

GRAD_CASES = ["gf_r4", "fast_r9_s2", "bga_r20", "bga_cx16", "fast_r1_s2", "gf_tsukuba"]


def load_grad_case(name):
    """The filter case of that name (inputs, omega) plus ``g`` (fp32, k / 127: exact) and the reference's float64
    gradients ``grad_y``, ``grad_x`` (joined from their parts along axis 1) and ``grad_omega``."""
    z = load_case(name)
    head = np.load(os.path.join(GOLDEN, f"guided_grad_{name}.npz"))
    z["g"] = (head["g_i8"].astype(np.float32) / np.float32(127.0)).astype(np.float32)
    z["grad_omega"] = head["grad_omega"]
    for k in ("gy", "gx"):
        parts = sorted(glob.glob(os.path.join(GOLDEN, f"guided_grad_{name}_{k}*.npz")), key=lambda p: int(p[:-4].rsplit(k, 1)[1]))
        z["grad_" + k[1]] = np.concatenate([np.load(p)["grad"] for p in parts], axis=1)
    return z


def torch_form_grads(guided, z, dtype, device, **kw):
    """(grad_y, grad_x, grad_omega) of sum(out * g) through the repository's class of the case."""
    import torch

    m = build_module(guided, z, dtype, device)
    for k, v in kw.items():
        setattr(m, k, v)
    y = torch.from_numpy(z["y"]).to(device=device, dtype=dtype).requires_grad_(True)
    x = torch.from_numpy(z["x"]).to(device=device, dtype=dtype).requires_grad_(True)
    g = torch.from_numpy(z["g"]).to(device=device, dtype=dtype)
    (m(y, x) * g).sum().backward()
    return y.grad, x.grad, m.omega.grad
