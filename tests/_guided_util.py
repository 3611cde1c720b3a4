"""Loader of the guided-filter fixtures (tests/golden/guided_*.npz, written by tests/golden/generate_guided.py)."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["gf_r4", "fast_r9_s2", "bga_r20", "bga_cx16", "fast_r1_s2", "gf_tsukuba", "crfasrnn_guided", "meanfield_guided"]
END_TO_END = ("crfasrnn_guided", "meanfield_guided")


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


def build_module(guided, z, dtype, device):
    """The repository's class of a filter case with ``omega`` loaded from the fixture."""
    import torch

    kind, cx, r, s = str(z["kind"]), int(z["cx"]), int(z["r"]), int(z["s"])
    if kind == "GuidedFilter":
        m = guided.GuidedFilter(cx, r, 1e-2)
    elif kind == "FastGuidedFilter":
        m = guided.FastGuidedFilter(cx, r, 1e-2, subsample_ratio=s)
    else:
        m = guided.BatchedGuidedAdjacency(cx, r, 1e-2, subsample_ratio=s)
    with torch.no_grad():
        m.omega.copy_(torch.from_numpy(z["omega"]))
    return m.to(device=device, dtype=dtype)
