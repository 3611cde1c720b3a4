"""What the tests of the bilinear full-covariance guided filter's backward share (test_guided_bilinear_full_grad_cpu.py,
test_gpu_guided_bilinear_full_grad.py): the closed form of the gradients that backward<ST, CX, true> (CX >= 1) of phl_guided.hip
implements, written as float64 torch ops (closed_form_grads of _guided_full_grad_util.py with the nearest sample /
upsample replaced by ``F.interpolate(..., mode='bilinear')`` and their adjoints taken as the vector-Jacobian products of
those two calls; the CPU test pins it to float64 autograd through the torch form), a spy that knows
phl.guided_filter_bilinear_full_grad, and the case helper of the GPU sweeps."""
import contextlib

import torch
import torch.nn.functional as F

from _guided_full_grad_util import module_call, omega_grad  # noqa: F401  (omega_grad: for the tests that import from here)


def _interp(t, size):
    """F.interpolate(mode='bilinear') of the last two dimensions of t [n, ..., a, b]."""
    return F.interpolate(t.reshape(t.shape[0], -1, *t.shape[-2:]), size=size, mode="bilinear").reshape(t.shape[:-2] + tuple(size))


def _interp_adjoint(v, size_in):
    """The vector-Jacobian product of ``_interp(., v's size)`` on an input of ``size_in`` with v: the map is linear, so
    the point it is taken at does not matter."""
    z = torch.zeros(v.shape[:-2] + tuple(size_in), dtype=v.dtype, device=v.device, requires_grad=True)
    with torch.enable_grad():
        out = _interp(z, tuple(v.shape[-2:]))
    return torch.autograd.grad(out, z, v)[0]


def closed_form_grads(y, x, g, r, eps, s, scale=1.0, subtract_is_y=False):
    """(grad_y, grad_x, grad_eps) of ``sum(out * g)``, out = guided_bilinear_full(y, x) * scale - (y if subtract_is_y else
    0): the full-covariance model solved on D(y), D(x) at (H // s, W // s) with radius r // s and eps [cx], its window
    means brought back by U.  Notation of phl_guided.hip."""
    from crf.guided import _box_sum

    n, cy, H, W = y.shape
    cx = x.shape[1]
    h, w, rr, dev = H // s, W // s, r // s, y.device
    D = lambda t: _interp(t, (h, w))                                    # noqa: E731
    U = lambda t: _interp(t, (H, W))                                    # noqa: E731
    Dt = lambda t: _interp_adjoint(t, (H, W))                           # noqa: E731
    Ut = lambda t: _interp_adjoint(t, (h, w))                           # noqa: E731

    S = lambda t: _box_sum(t.reshape(n, -1, h, w), rr).reshape(t.shape)     # noqa: E731
    N = _box_sum(torch.ones((1, 1, h, w), dtype=y.dtype, device=dev), rr)
    mean = lambda t: S(t) / N                                           # noqa: E731
    ys, xs = D(y), D(x)
    m, my = mean(xs), mean(ys)
    Sig = mean(xs[:, :, None] * xs[:, None]) - m[:, :, None] * m[:, None]                              # [n, cx, cx, h, w]
    P = torch.linalg.inv(Sig.permute(0, 3, 4, 1, 2) + torch.diag_embed(eps.expand(cx)))             # [n, h, w, cx, cx]
    cv = mean(ys[:, :, None] * xs[:, None]) - my[:, :, None] * m[:, None]                              # [n, cy, cx, h, w]
    A = torch.einsum("nldhw,nhwdc->nlchw", cv, P)

    gA = S(scale * Ut(g[:, :, None] * x[:, None]) / N)
    gb = S(scale * Ut(g) / N)
    gAp = gA - gb[:, :, None] * m[:, None]
    gcv = torch.einsum("nlchw,nhwcd->nldhw", gAp, P)
    gSig = -0.5 * (torch.einsum("nlchw,nldhw->ncdhw", A, gcv) + torch.einsum("nldhw,nlchw->ncdhw", A, gcv))
    gmy = gb - (gcv * m[:, None]).sum(2)
    gm = -(gb[:, :, None] * A).sum(1) - (gcv * my[:, :, None]).sum(1) - 2 * (gSig * m[:, None]).sum(2)
    U0, Ul, V = S(gmy / N), S(gcv / N), S(gSig / N)
    gys = U0 + (xs[:, None] * Ul).sum(2)
    gxs = (ys[:, :, None] * Ul).sum(1) + S(gm / N) + 2 * (xs[:, None] * V).sum(2)
    grad_y = Dt(gys) - (g if subtract_is_y else 0)
    grad_x = scale * (g[:, :, None] * U(mean(A))).sum(1) + Dt(gxs)
    grad_eps = torch.diagonal(gSig, dim1=1, dim2=2).sum((0, 1, 2))
    return grad_y, grad_x, grad_eps


WHERE = {"bilinear": "guided_filter_bilinear", "bilinear_full_grad": "guided_filter_bilinear_full_grad",
         "bilinear_grad": "guided_filter_bilinear_grad", "nearest_full_grad": "guided_filter_full_grad",
         "nearest": "guided_filter", "nearest_grad": "guided_filter_grad"}


@contextlib.contextmanager
def spy():
    """Counts of the calls of phl.guided_filter_bilinear ("bilinear"), phl.guided_filter_bilinear_full_grad
    ("bilinear_full_grad"), phl.guided_filter_bilinear_grad ("bilinear_grad"), phl.guided_filter_full_grad
    ("nearest_full_grad"), phl.guided_filter ("nearest"), phl.guided_filter_grad ("nearest_grad") and
    crf.guided._box_sum ("box_sum")."""
    import phl
    from crf import guided

    where = {key: (phl, name) for key, name in WHERE.items()}
    where["box_sum"] = (guided, "_box_sum")
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


def route(**counts):
    """The spy's counts with everything 0 but ``counts``."""
    return {**{key: 0 for key in list(WHERE) + ["box_sum"]}, **counts}


ROUTE = route(bilinear=1, bilinear_full_grad=1)


def module(kind, cx, r, s, eps, **kw):
    """The ``mode='bilinear', fused_bilinear=True, full_cov=True`` class of a case."""
    from _guided_bilinear_util import module as bilinear_module

    return bilinear_module(kind, cx, r, s, eps, fused_bilinear=True, full_cov=True, **kw)


def check_bilinear_full_grad(name, m, y, x, g, guide=None, min_torch_u=None, absolute=()):
    """The gradients of y, x and omega of the ``bilinear_full_grad`` module m on the kernels against fp32 and float64 torch
    autograd of the mode on the device: e_hip <= e_torch, no margin, under the precondition e_torch >= min_torch_u u
    (``absolute``: the gradients whose exact value is 0 -- no precondition, no u); on the correlated guide with more than
    one channel and a window of more than one pixel also |full - diagonal| >= 1000 e_hip for each gradient, the diagonal
    one from phl.guided_filter_bilinear_grad.  Returns the kernels' gradients and the largest e_hip in u."""
    import phl
    from _guided_bilinear_util import MIN_U
    from _guided_util import grads, report

    if min_torch_u is None:
        min_torch_u = MIN_U
    assert m.full_cov and m.fused_bilinear and m.bilinear_full_grad
    with spy() as calls:
        hip = grads(m, y, x, g, torch.float32)
    assert calls == ROUTE, (name, calls)
    m.bilinear_full_grad = False
    with spy() as calls:
        t32 = grads(m, y, x, g, torch.float32)
    assert calls == route(box_sum=calls["box_sum"]) and calls["box_sum"] > 0, (name, calls)
    want = grads(m.double(), y, x, g, torch.float64)
    m.float()
    m.bilinear_full_grad = True
    e, worst = [], 0.0
    for k, a, b, c in zip(("y", "x", "omega"), hip, t32, want):
        e_hip, _, mag = report(f"{name} grad_{k}", a, b, c, what="grad", min_torch_u=None if k in absolute else min_torch_u)
        e.append(e_hip)
        if k not in absolute:
            worst = max(worst, e_hip / (2.0 ** -24 * mag))
    r, s, scale, sub = module_call(m)
    if guide == "correlated" and x.shape[1] > 1 and r // s >= 1:
        dy, dx, de = phl.guided_filter_bilinear_grad(y, x, g, r, m.eps.detach(), subsample=s, scale=scale, subtract_is_y=sub,
                                                     need_y=True, need_x=True, need_eps=True)
        for k, a, d, e_hip in zip(("y", "x", "omega"), hip, (dy, dx, omega_grad(de, m.omega.detach())), e):
            gap = float((a - d).abs().max())
            print(f"{name} grad_{k}: |full - diagonal| = {gap:.3e} = {gap / max(e_hip, 1e-300):.3g} e_hip")
            assert gap >= 1000 * e_hip, (name, k, gap, e_hip)
    print(f"{name}: largest e_hip = {worst:.2f} u")
    return hip, worst


def bilinear_full_grad_case(kind, B, cy, cx, H, W, r, s, eps, guide, seed=0, noncontiguous=False, min_torch_u=None, absolute=()):
    from _guided_full_grad_util import grad_inputs
    from _guided_util import DEV

    y, x, g = grad_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    m = module(kind, cx, r, s, eps, bilinear_full_grad=True).to(DEV)
    name = f"bilinear full grad {kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g} {guide}"
    hip, worst = check_bilinear_full_grad(name, m, y, x, g, guide, min_torch_u, absolute)
    return {"name": name, "m": m, "y": y, "x": x, "g": g, "hip": hip, "u": worst}
