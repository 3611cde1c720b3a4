"""What the GPU tests of the channel-major mean-field step share (test_gpu_nchw_step.py, test_gpu_nchw_wide.py,
test_gpu_nchw_train.py, test_gpu_nchw_expect.py): the inputs and the accuracy rule of the product, the spies on the
library's launches, on the binding and on crf.crf_module's torch ops, and the two loops of CRFasRNN side by side.

Rule of the step's accuracy checks (the project's own, test_gpu_crf_api.py): with Y64 the float64 result on the device,
e_hip = max|hip - Y64| and e_torch = max|fp32 torch ops - Y64| over ALL elements, and
e_hip <= max(2e-6 * max(1, |Y64|.max()), 2 * e_torch).  The loop is held to e_new <= 2 * e_old against float64, e_old
being the plain loop in the same tree.  Every pair of errors is printed."""
import contextlib

import torch
import torch.nn.functional as F

from _guided_util import DEV, route, spy

B = 2
WIDE = "phl_nchw_softmax_compat_wide"
PRODUCT, UNIFORM, SOFTMAX, LOGITS = 0, 1, 2, 3                   # enum phl_nchw_mode


def inputs(L, H, W, seed, B=B):
    g = torch.Generator(device=DEV).manual_seed(seed)
    E0 = torch.rand((B, L, H, W), device=DEV, generator=g) * 30 - 5
    G = torch.randn((B, L, H, W), device=DEV, generator=g) * 5
    Mu = torch.rand((L, L), device=DEV, generator=g) * 4 + torch.arange(L, device=DEV, dtype=torch.float32)[:, None] * 0.05
    return E0, G, Mu


def energy(E0, G):
    return E0 if G is None else E0 + G


def truth(E0, G, Mu64):
    return torch.einsum("ac,bahw->bchw", Mu64, F.softmax(-energy(E0.double(), None if G is None else G.double()), 1))


def torch32(E0, G, Mu):
    return F.conv2d(F.softmax(-energy(E0, G), 1), Mu.t()[..., None, None])


def check_product(name, hip, E0, G, Mu, Mu64=None):
    want = truth(E0, G, Mu.double() if Mu64 is None else Mu64)
    e_hip = float((hip.double() - want).abs().max())
    e_torch = float((torch32(E0, G, Mu).double() - want).abs().max())
    bound = max(2e-6 * max(1.0, float(want.abs().max())), 2 * e_torch)
    print(f"{name}: e_hip = {e_hip:.3e}  e_torch = {e_torch:.3e}  |Y| <= {float(want.abs().max()):.4g}")
    assert torch.isfinite(hip).all(), name
    assert e_hip <= bound, (name, e_hip, e_torch)


def on_float4_path(*tensors):
    return all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0 and t[0, 0].numel() % 4 == 0) for t in tensors)


def shifted(t):
    """A contiguous copy of t whose base lies 4 bytes past the 16-byte grid."""
    buf = torch.zeros((t.numel() + 5,), device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@contextlib.contextmanager
def launch_spy(modeless=(WIDE,)):
    """(entry point, mode) of every library launch made through phl._launch; the mode is the launch's last argument, and
    None for the entry points in ``modeless``, which have none."""
    import phl

    real, seen = phl._launch, []

    def launch(device, name, *args):
        seen.append((name, None if name in modeless else args[-1]))
        return real(device, name, *args)

    phl._launch = launch
    try:
        yield seen
    finally:
        phl._launch = real


@contextlib.contextmanager
def binding_spy(record):
    """Calls of the binding: ``record`` maps the name of a function of phl to ``f(args, kwargs)``, called before every call
    of it; what it returns, unless None, is appended to the list this yields."""
    import phl

    seen = []
    real = {k: getattr(phl, k) for k in record}

    def wrap(k):
        def f(*a, **kw):
            note = record[k](a, kw)
            if note is not None:
                seen.append(note)
            return real[k](*a, **kw)
        return f

    for k in record:
        setattr(phl, k, wrap(k))
    try:
        yield seen
    finally:
        for k, f in real.items():
            setattr(phl, k, f)


class CountingF:
    """torch.nn.functional as crf.crf_module sees it, with softmax and conv2d counted."""

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        return getattr(F, name)

    def softmax(self, *a, **k):
        self._calls["softmax"] += 1
        return F.softmax(*a, **k)

    def conv2d(self, *a, **k):
        self._calls["conv2d"] += 1
        return F.conv2d(*a, **k)


@contextlib.contextmanager
def loop_spy(order=False):
    """Counts of F.softmax / F.conv2d calls made from crf.crf_module, and of the loop's calls into the binding: in
    ``calls["step"]`` the number of phl.nchw_softmax_compat calls -- or, with ``order``, in ``calls["phl"]`` their order:
    "wide" (nchw_softmax_compat_wide), "step" / "logits" (nchw_softmax_compat without / with logits=True), "expect"
    (nchw_expected_value)."""
    from crf import crf_module as cm

    calls = {"softmax": 0, "conv2d": 0}
    if order:
        record = {"nchw_softmax_compat": lambda a, k: "logits" if k.get("logits") else "step",
                  "nchw_softmax_compat_wide": lambda a, k: "wide", "nchw_expected_value": lambda a, k: "expect"}
    else:
        calls["step"] = 0
        record = {"nchw_softmax_compat": lambda a, k: calls.update(step=calls["step"] + 1)}
    real_f, cm.F = cm.F, CountingF(calls)
    try:
        with binding_spy(record) as seen:
            if order:
                calls["phl"] = seen
            yield calls
    finally:
        cm.F = real_f


@contextlib.contextmanager
def old_loop():
    """The module switch behind PHL_NCHW_STEP=0: the plain loop and the torch lines of logits2average_depth."""
    from crf import crf_module as cm

    was, cm._NCHW_STEP = cm._NCHW_STEP, False
    try:
        yield
    finally:
        cm._NCHW_STEP = was


def both_loops(call, niters, end=None):
    """(new loop, old loop) outputs of one no-grad call, with the call counts of both checked.  end: None for a loop on
    phl.nchw_softmax_compat alone, its calls counted; "logits" or "expect" for a loop on the wide entry, the order of
    its calls checked up to this last one."""
    order = end is not None
    with torch.no_grad():
        with loop_spy(order) as calls, spy() as wcalls:
            new = call()
        if order:
            assert calls == {"softmax": 0, "conv2d": 0, "phl": ["wide"] * niters + [end]}, calls
        else:
            assert calls == {"softmax": 0, "conv2d": 0, "step": niters + 1}, calls
        assert wcalls == route(nearest=niters), wcalls
        with old_loop(), loop_spy(order) as calls:
            old = call()
        if order:
            assert calls["phl"] == [] and calls["softmax"] == niters + 1 and calls["conv2d"] == niters, calls
        else:
            assert calls["step"] == 0 and calls["softmax"] == niters + 1, calls
    return new, old


def report_loop(name, new, old, want):
    e_new, e_old = float((new.double() - want).abs().max()), float((old.double() - want).abs().max())
    print(f"{name}: e_new = {e_new:.3e}  e_old = {e_old:.3e}  |out| <= {float(want.abs().max()):.4g}")
    assert torch.isfinite(new).all()
    assert e_new <= 2 * e_old, (name, e_new, e_old)
