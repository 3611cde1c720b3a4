"""The guided-filter fixtures (tests/golden/guided_*.npz) without a GPU: their names, their loaders, and the repository's
class of a fixture record with its gradients.  Shared by the tests and by the generators under tests/golden/
(generate_guided*.py), which import from here only."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["gf_r4", "fast_r9_s2", "bga_r20", "bga_cx16", "fast_r1_s2", "gf_tsukuba", "crfasrnn_guided", "meanfield_guided"]
END_TO_END = ("crfasrnn_guided", "meanfield_guided")
GRAD_CASES = ["gf_r4", "fast_r9_s2", "bga_r20", "bga_cx16", "fast_r1_s2", "gf_tsukuba"]
BIL_CASES = ["bil_fast_r9_s2", "bil_bga_cx1_s3", "bil_bga_cx3_s2"]


def load_case(name):
    """dict of arrays; ``out`` (float64) is joined from the guided_<name>_out<k>.npz parts along axis 1."""
    z = dict(np.load(os.path.join(GOLDEN, f"guided_{name}.npz")))
    parts = sorted(glob.glob(os.path.join(GOLDEN, f"guided_{name}_out*.npz")))
    z["out"] = np.concatenate([np.load(p)["out"] for p in parts], axis=1)
    for k in ("y", "x"):
        if k + "_u8" in z:
            z[k] = (z.pop(k + "_u8").astype(np.float32) / np.float32(255.0)).astype(np.float32)
    if "logits_f16" in z:
        z["logits"] = z.pop("logits_f16").astype(np.float32)
    return z


def _stem(name):
    """The file stem of a case's gradient fixture: guided_grad_<name>, or guided_bil_grad_<name without bil_>."""
    if name in BIL_CASES:
        return "guided_bil_grad_" + name[len("bil_"):]
    assert name in GRAD_CASES
    return "guided_grad_" + name


def load_grad_case(name, stem=None):
    """The filter case of that name (inputs, omega) plus ``g`` (fp32, k / 127: exact) and the reference's float64
    gradients ``grad_y``, ``grad_x`` (joined from their parts along axis 1) and ``grad_omega``, read from <stem>*.npz
    (default: the stem of the family the name belongs to)."""
    stem = stem or _stem(name)
    z = load_case(name)
    head = np.load(os.path.join(GOLDEN, stem + ".npz"))
    z["g"] = (head["g_i8"].astype(np.float32) / np.float32(127.0)).astype(np.float32)
    z["grad_omega"] = head["grad_omega"]
    for k in ("gy", "gx"):
        parts = sorted(glob.glob(os.path.join(GOLDEN, f"{stem}_{k}*.npz")), key=lambda p: int(p[:-4].rsplit(k, 1)[1]))
        z["grad_" + k[1]] = np.concatenate([np.load(p)["grad"] for p in parts], axis=1)
    return z


def build_module(guided, z, dtype, device, mode="nearest", **kw):
    """The repository's class of a filter case (``mode``: that of the fixture's family) with ``omega`` loaded from the
    fixture; ``kw`` goes to the constructor."""
    kind, cx, r, s = str(z["kind"]), int(z["cx"]), int(z["r"]), int(z["s"])
    if kind != "GuidedFilter":
        kw["subsample_ratio"] = s
    if mode != "nearest":
        kw["mode"] = mode
    m = getattr(guided, kind)(cx, r, 1e-2, **kw)
    with torch.no_grad():
        m.omega.copy_(torch.from_numpy(z["omega"]))
    return m.to(device=device, dtype=dtype)


def fixture_grads(guided, z, dtype, device, mode="nearest", **kw):
    """(grad_y, grad_x, grad_omega) of sum(out * g) through the repository's class of the case; ``kw`` goes to the
    constructor.  (The one keyword that used to be set as an attribute after construction, ``fused_grad``, has no
    constructor check: the module is the same either way.)"""
    m = build_module(guided, z, dtype, device, mode, **kw)
    y = torch.from_numpy(z["y"]).to(device=device, dtype=dtype).requires_grad_(True)
    x = torch.from_numpy(z["x"]).to(device=device, dtype=dtype).requires_grad_(True)
    g = torch.from_numpy(z["g"]).to(device=device, dtype=dtype)
    (m(y, x) * g).sum().backward()
    return y.grad, x.grad, m.omega.grad
