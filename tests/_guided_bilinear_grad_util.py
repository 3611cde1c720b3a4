"""What the tests of the bilinear guided filter's backward share (test_guided_bilinear_grad_cpu.py,
test_gpu_guided_bilinear_grad.py) with the fixture generator tests/golden/generate_guided_bilinear_grad.py: the loader of
tests/golden/guided_bil_grad_*.npz, the gradients of a fixture case through the repository's class, and on the GPU the
spy and the accuracy rule of the kernel route (phl.GuidedFilterBilinearFn behind ``bilinear_grad=True``)."""
import contextlib
import glob
import os

import numpy as np
import torch

from _guided_bilinear_util import BIL_CASES, MIN_U, build_module, load_bilinear, module
from _guided_util import GOLDEN, _sweep_inputs, grads, report


def _stem(name):
    assert name in BIL_CASES
    return "guided_bil_grad_" + name[len("bil_"):]


def load_bilinear_grad(name):
    """The bilinear fixture case of that name (inputs, omega) plus ``g`` (fp32, k / 127: exact) and the reference's
    float64 gradients ``grad_y``, ``grad_x`` (joined from their parts along axis 1) and ``grad_omega``."""
    z = load_bilinear(name)
    head = np.load(os.path.join(GOLDEN, _stem(name) + ".npz"))
    z["g"] = (head["g_i8"].astype(np.float32) / np.float32(127.0)).astype(np.float32)
    z["grad_omega"] = head["grad_omega"]
    for k in ("gy", "gx"):
        parts = sorted(glob.glob(os.path.join(GOLDEN, f"{_stem(name)}_{k}*.npz")), key=lambda p: int(p[:-4].rsplit(k, 1)[1]))
        z["grad_" + k[1]] = np.concatenate([np.load(p)["grad"] for p in parts], axis=1)
    return z


def fixture_grads(guided, z, dtype, device, **kw):
    """(grad_y, grad_x, grad_omega) of sum(out * g) through the repository's ``mode='bilinear'`` class of the case."""
    m = build_module(guided, z, dtype, device, **kw)
    y = torch.from_numpy(z["y"]).to(device=device, dtype=dtype).requires_grad_(True)
    x = torch.from_numpy(z["x"]).to(device=device, dtype=dtype).requires_grad_(True)
    g = torch.from_numpy(z["g"]).to(device=device, dtype=dtype)
    (m(y, x) * g).sum().backward()
    return y.grad, x.grad, m.omega.grad


@contextlib.contextmanager
def spy():
    """Counts of phl.guided_filter_bilinear ("bilinear"), phl.guided_filter_bilinear_grad ("bilinear_grad"),
    phl.guided_filter ("nearest"), phl.guided_filter_grad ("nearest_grad") and crf.guided._box_sum ("box_sum") calls."""
    import phl
    from crf import guided

    where = {"bilinear": (phl, "guided_filter_bilinear"), "bilinear_grad": (phl, "guided_filter_bilinear_grad"),
             "nearest": (phl, "guided_filter"), "nearest_grad": (phl, "guided_filter_grad"), "box_sum": (guided, "_box_sum")}
    calls = {key: 0 for key in where}
    real = {key: getattr(mod, name) for key, (mod, name) in where.items()}

    def counted(key):
        def f(*a, **k):
            calls[key] += 1
            return real[key](*a, **k)
        return f

    for key, (mod, name) in where.items():
        setattr(mod, name, counted(key))
    try:
        yield calls
    finally:
        for key, (mod, name) in where.items():
            setattr(mod, name, real[key])


ROUTE = {"bilinear": 1, "bilinear_grad": 1, "nearest": 0, "nearest_grad": 0, "box_sum": 0}


def sweep_case_grad(kind, B, cy, cx, H, W, r, s, eps, seed=0, noncontiguous=False, min_torch_u=MIN_U):
    """The gradients of y, x and omega on the kernels against fp32 and float64 torch autograd of the mode on the device:
    e_hip <= e_torch, no margin, under the precondition e_torch >= min_torch_u u.  Returns the module (fp32, the keyword
    off), its inputs, the kernels' gradients and the largest e_hip in u."""
    y, x, g = _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, True)
    name = f"bilinear {kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g}"
    m = module(kind, cx, r, s, eps, fused_bilinear=True, bilinear_grad=True).to(torch.device("cuda", 0))
    with spy() as calls:
        hip = grads(m, y, x, g, torch.float32)
    assert calls == ROUTE, (name, calls)
    m.bilinear_grad = False
    with spy() as calls:
        t32 = grads(m, y, x, g, torch.float32)
    assert calls["bilinear"] == 0 and calls["bilinear_grad"] == 0 and calls["box_sum"] > 0
    want = grads(m.double(), y, x, g, torch.float64)
    worst = 0.0
    for k, a, b, c in zip(("y", "x", "omega"), hip, t32, want):
        e_hip, _, mag = report(f"{name} grad_{k}", a, b, c, what="grad", min_torch_u=min_torch_u)
        worst = max(worst, e_hip / (2.0 ** -24 * mag))
    return {"name": name, "m": m.float(), "y": y, "x": x, "g": g, "hip": hip, "u": worst}
