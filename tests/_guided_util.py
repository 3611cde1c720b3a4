"""Loader of the guided-filter fixtures (tests/golden/guided_*.npz, written by tests/golden/generate_guided.py), and what
the GPU tests of the forward (test_gpu_guided.py) and of the backward (test_gpu_guided_grad.py) share."""
import contextlib
import glob
import os

import numpy as np
import torch

DEV = torch.device("cuda", 0)

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


@contextlib.contextmanager
def torch_form():
    """The classes with the HIP dispatch switched off (what they were before it existed)."""
    from crf import guided

    real = guided.GuidedFilter._fused
    guided.GuidedFilter._fused = lambda self, *a, **k: None
    try:
        yield
    finally:
        guided.GuidedFilter._fused = real


@contextlib.contextmanager
def spy(grad=False):
    """Counts of phl.guided_filter ("hip"), crf.guided._box_sum ("box_sum") and, with ``grad``, phl.guided_filter_grad
    ("hip_grad") calls."""
    import phl
    from crf import guided

    where = {"hip": (phl, "guided_filter"), "box_sum": (guided, "_box_sum")}
    if grad:
        where["hip_grad"] = (phl, "guided_filter_grad")
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


def report(name, hip, t32, want, factor=1, what="out", min_torch_u=None):
    """The accuracy rule e_hip <= factor * e_torch.  ``min_torch_u``: a precondition on the input, checked first -- the
    fp32 torch form must err by at least that many u = 2^-24 * max|want|, or the rule judges nothing (a shape at which
    fp32 prefix sums are exact leaves the kernel no room for its own roundings).  Returns (e_hip, e_torch, max|want|)."""
    e_hip = float((hip.double() - want).abs().max())
    e_torch = float((t32.double() - want).abs().max())
    mag = float(want.abs().max())
    print(f"{name}: e_hip = {e_hip:.3e}  e_torch = {e_torch:.3e}  |{what}| <= {mag:.4g}")
    assert torch.isfinite(hip).all()
    if min_torch_u is not None:
        u = 2.0 ** -24 * mag
        print(f"{name}: e_hip = {e_hip / u:.2f} u  e_torch = {e_torch / u:.1f} u  (precondition: e_torch >= {min_torch_u} u)")
        assert e_torch >= min_torch_u * u, ("precondition", name, e_torch / u)
    assert e_hip <= factor * e_torch, (name, e_hip, e_torch)
    return e_hip, e_torch, mag


def module(kind, cx, r, s, eps, **kw):
    from crf import guided

    if kind == "gf":
        return guided.GuidedFilter(cx, r, eps, **kw)
    if kind == "fast":
        return guided.FastGuidedFilter(cx, r, eps, subsample_ratio=s, **kw)
    return guided.BatchedGuidedAdjacency(cx, r, eps, subsample_ratio=s, **kw)


def grads(m, y, x, g, dtype):
    yy, xx = y.detach().to(dtype).requires_grad_(True), x.detach().to(dtype).requires_grad_(True)
    m.omega.grad = None
    (m(yy, xx) * g.to(dtype)).sum().backward()
    return yy.grad, xx.grad, m.omega.grad.clone()


def _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, with_g):
    """y, x and (``with_g``) the upstream gradient g, drawn in this order from one generator."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    if noncontiguous:
        y = torch.rand((B, H, W, cy), device=DEV, generator=gen).permute(0, 3, 1, 2)
        x = torch.rand((B, cx, H, 2 * W), device=DEV, generator=gen)[..., ::2]
        g = (torch.rand((B, cy, W, H), device=DEV, generator=gen) * 2 - 1).transpose(2, 3) if with_g else None
    else:
        y = torch.rand((B, cy, H, W), device=DEV, generator=gen)
        x = torch.rand((B, cx, H, W), device=DEV, generator=gen)
        g = torch.rand((B, cy, H, W), device=DEV, generator=gen) * 2 - 1 if with_g else None
    return y, x, g


def sweep_case(kind, B, cy, cx, H, W, r, s, eps, seed=0, noncontiguous=False, use_out=False, min_torch_u=None):
    """The forward on the kernels against the fp32 and the float64 torch form (``min_torch_u``: report's precondition).
    Returns the module, its inputs and the kernels' output."""
    import phl

    y, x, _ = _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, False)
    m = module(kind, cx, r, s, eps).to(DEV)
    name = f"{kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g}"
    with torch.no_grad():
        if use_out:
            out = torch.full((B, cy, H, W), float("nan"), device=DEV)
            k = 0.5 * (2 * r + 1) ** 2 if kind == "bga" else 1.0
            hip = phl.guided_filter(y, x, r, m.eps, subsample=s, scale=k, subtract=y if kind == "bga" else None, out=out)
            assert hip is out
        else:
            with spy() as calls:
                hip = m(y, x)
            assert calls == {"hip": 1, "box_sum": 0}, name
        with torch_form():
            t32 = m(y, x)
            want = m.double()(y.double(), x.double())
        m.float()
    report(name, hip, t32, want, min_torch_u=min_torch_u)
    return {"name": name, "m": m, "y": y, "x": x, "hip": hip}


def sweep_case_grad(kind, B, cy, cx, H, W, r, s, eps, seed=0, noncontiguous=False, min_torch_u=None):
    """The gradients of y, x and omega on the kernels against fp32 and float64 torch autograd (``min_torch_u``: report's
    precondition).  Returns the module (fp32, ``fused_grad`` off), its inputs and the kernels' gradients."""
    y, x, g = _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, True)
    name = f"{kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g}"
    m = module(kind, cx, r, s, eps, fused_grad=True).to(DEV)
    with spy(grad=True) as calls:
        hip = grads(m, y, x, g, torch.float32)
    assert calls == {"hip": 1, "hip_grad": 1, "box_sum": 0}, name
    m.fused_grad = False
    with spy(grad=True) as calls:
        t32 = grads(m, y, x, g, torch.float32)
    assert calls["hip"] == 0 and calls["hip_grad"] == 0 and calls["box_sum"] > 0
    want = grads(m.double(), y, x, g, torch.float64)
    for k, a, b, c in zip(("y", "x", "omega"), hip, t32, want):
        report(f"{name} grad_{k}", a, b, c, what="grad", min_torch_u=min_torch_u)
    return {"name": name, "m": m.float(), "y": y, "x": x, "g": g, "hip": hip}
