"""What the tests of FastGuidedFilter(mode='bilinear') share (test_guided_bilinear_cpu.py, test_gpu_guided_bilinear.py,
test_gpu_guided_bilinear_chunks.py) with the fixture generator tests/golden/generate_guided_bilinear.py: the fixture
cases, the module of a case, and the accuracy rule of tests/test_gpu_guided.py applied to the kernel route
(phl.guided_filter_bilinear behind ``fused_bilinear=True``)."""
import contextlib

import torch

from _guided_util import load_case, report, torch_form

BIL_CASES = ["bil_fast_r9_s2", "bil_bga_cx1_s3", "bil_bga_cx3_s2"]
MIN_U = 8


def build_module(guided, z, dtype, device, **kw):
    """The repository's class of a fixture case with ``mode='bilinear'`` and ``omega`` loaded from the fixture."""
    kind, cx, r, s = str(z["kind"]), int(z["cx"]), int(z["r"]), int(z["s"])
    m = getattr(guided, kind)(cx, r, 1e-2, subsample_ratio=s, mode="bilinear", **kw)
    with torch.no_grad():
        m.omega.copy_(torch.from_numpy(z["omega"]))
    return m.to(device=device, dtype=dtype)


def load_bilinear(name):
    assert name in BIL_CASES
    return load_case(name)


def module(kind, cx, r, s, eps, **kw):
    from crf import guided

    cls = guided.FastGuidedFilter if kind == "fast" else guided.BatchedGuidedAdjacency
    return cls(cx, r, eps, subsample_ratio=s, mode="bilinear", **kw)


@contextlib.contextmanager
def spy():
    """Counts of phl.guided_filter_bilinear ("bilinear"), phl.guided_filter ("nearest") and crf.guided._box_sum
    ("box_sum") calls."""
    import phl
    from crf import guided

    where = {"bilinear": (phl, "guided_filter_bilinear"), "nearest": (phl, "guided_filter"), "box_sum": (guided, "_box_sum")}
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


def check(name, m, y, x, min_torch_u=MIN_U, absolute=False):
    """The forward of the ``fused_bilinear`` module m on the kernels against its fp32 and float64 torch forms on the
    device: e_hip <= e_torch, no margin, under the precondition e_torch >= min_torch_u u.  Returns the kernels' output and
    e_hip in u (``absolute``: as it is)."""
    assert m.fused_bilinear and m.mode == "bilinear"
    with torch.no_grad():
        with spy() as calls:
            hip = m(y, x)
        assert calls == {"bilinear": 1, "nearest": 0, "box_sum": 0}, (name, calls)
        with torch_form():
            t32 = m(y, x)
            want = m.double()(y.double(), x.double())
        m.float()
    e_hip, _, mag = report(name, hip, t32, want, min_torch_u=min_torch_u)
    return hip, e_hip if absolute else e_hip / (2.0 ** -24 * mag)
