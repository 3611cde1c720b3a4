"""What the tests of the full-covariance guided filter's backward share (test_guided_full_grad_cpu.py,
test_gpu_guided_full_grad.py): the closed form of the gradients that the kernels of phl_guided.hip implement, written as
float64 torch ops on crf.guided._box_sum (the CPU test pins it to float64 autograd through the torch form, so the kernels
are held to a formula that is checked where no GPU is needed), a spy that knows phl.guided_filter_full_grad, and the
case helper of the GPU sweeps."""
import contextlib

import torch
import torch.nn.functional as F


def _nearest(n_in, n_out, device):
    if n_in == n_out:
        return torch.arange(n_in, device=device)
    src = torch.arange(n_in, dtype=torch.float32, device=device).reshape(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(n_out).long()


def closed_form_grads(y, x, g, r, eps, s=1, scale=1.0, subtract_is_y=False):
    """(grad_y, grad_x, grad_eps) of ``sum(out * g)``, out = guided_full(y, x) * scale - (y if subtract_is_y else 0): the
    model solved at (H // s, W // s) on nearest samples with radius r // s and eps [cx].  Notation of phl_guided.hip."""
    from crf.guided import _box_sum

    n, cy, H, W = y.shape
    cx = x.shape[1]
    h, w, rr, dev = H // s, W // s, r // s, y.device
    rows, cols, rlow, clow = _nearest(H, h, dev), _nearest(W, w, dev), _nearest(h, H, dev), _nearest(w, W, dev)
    sample = lambda t: t[..., rows, :][..., cols]                       # noqa: E731
    upsample = lambda t: t[..., rlow, :][..., clow]                     # noqa: E731

    def down(t):                                                        # adjoint of upsample: sums over the pre-images
        a = torch.zeros(t.shape[:-2] + (h, W), dtype=t.dtype, device=dev).index_add_(-2, rlow, t)
        return torch.zeros(t.shape[:-2] + (h, w), dtype=t.dtype, device=dev).index_add_(-1, clow, a)

    def scatter(t):                                                     # adjoint of sample (the maps are strictly increasing)
        out = torch.zeros(t.shape[:-2] + (H, W), dtype=t.dtype, device=dev)
        out[..., rows[:, None], cols[None, :]] = t
        return out

    S = lambda t: _box_sum(t.reshape(n, -1, h, w), rr).reshape(t.shape)     # noqa: E731
    N = _box_sum(torch.ones((1, 1, h, w), dtype=y.dtype, device=dev), rr)
    mean = lambda t: S(t) / N                                           # noqa: E731
    ys, xs = sample(y), sample(x)
    m, my = mean(xs), mean(ys)
    Sig = mean(xs[:, :, None] * xs[:, None]) - m[:, :, None] * m[:, None]                              # [n, cx, cx, h, w]
    P = torch.linalg.inv(Sig.permute(0, 3, 4, 1, 2) + torch.diag_embed(eps.expand(cx)))             # [n, h, w, cx, cx]
    cv = mean(ys[:, :, None] * xs[:, None]) - my[:, :, None] * m[:, None]                              # [n, cy, cx, h, w]
    A = torch.einsum("nldhw,nhwdc->nlchw", cv, P)

    gA = S(scale * down(g[:, :, None] * x[:, None]) / N)
    gb = S(scale * down(g) / N)
    gAp = gA - gb[:, :, None] * m[:, None]
    gcv = torch.einsum("nlchw,nhwcd->nldhw", gAp, P)
    gSig = -0.5 * (torch.einsum("nlchw,nldhw->ncdhw", A, gcv) + torch.einsum("nldhw,nlchw->ncdhw", A, gcv))
    gmy = gb - (gcv * m[:, None]).sum(2)
    gm = -(gb[:, :, None] * A).sum(1) - (gcv * my[:, :, None]).sum(1) - 2 * (gSig * m[:, None]).sum(2)
    U0, U, V = S(gmy / N), S(gcv / N), S(gSig / N)
    gys = U0 + (xs[:, None] * U).sum(2)
    gxs = (ys[:, :, None] * U).sum(1) + S(gm / N) + 2 * (xs[:, None] * V).sum(2)
    grad_y = scatter(gys) - (g if subtract_is_y else 0)
    grad_x = scale * (g[:, :, None] * upsample(mean(A))).sum(1) + scatter(gxs)
    grad_eps = torch.diagonal(gSig, dim1=1, dim2=2).sum((0, 1, 2))
    return grad_y, grad_x, grad_eps


def omega_grad(grad_eps, omega):
    """The gradient of omega from that of eps = softplus(omega)."""
    return grad_eps * torch.sigmoid(omega)


def module_call(m):
    """(r, s, scale, subtract_is_y) of the phl call that module m makes."""
    r, s = m._r, getattr(m, "subsample_ratio", 1)
    adjacency = type(m).__name__ == "BatchedGuidedAdjacency"
    return r, s, 0.5 * (2 * r + 1) ** 2 if adjacency else 1.0, adjacency


@contextlib.contextmanager
def spy():
    """Counts of phl.guided_filter ("hip"), phl.guided_filter_grad ("hip_grad"), phl.guided_filter_full_grad
    ("hip_full_grad") and crf.guided._box_sum ("box_sum") calls."""
    import phl
    from crf import guided

    where = {"hip": (phl, "guided_filter"), "hip_grad": (phl, "guided_filter_grad"),
             "hip_full_grad": (phl, "guided_filter_full_grad"), "box_sum": (guided, "_box_sum")}
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


ROUTE = {"hip": 1, "hip_grad": 0, "hip_full_grad": 1, "box_sum": 0}


def grad_inputs(B, cy, cx, H, W, guide, seed, noncontiguous=False):
    """y, x of _guided_full_util.full_inputs and an upstream gradient g in [-1, 1) (``noncontiguous``: a transposed one)."""
    from _guided_full_util import full_inputs
    from _guided_util import DEV

    y, x = full_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    gen = torch.Generator(device=DEV).manual_seed(seed + 1000)
    if noncontiguous:
        g = (torch.rand((B, cy, W, H), device=DEV, generator=gen) * 2 - 1).transpose(2, 3)
        assert not g.is_contiguous()
    else:
        g = torch.rand((B, cy, H, W), device=DEV, generator=gen) * 2 - 1
    return y, x, g


def rule(name, hip, t32, want, factor=1, units=True):
    """e_hip <= factor * e_torch over all elements, both printed (``units``: also in u = 2^-24 max|want|) before the
    assertion.  Returns e_hip."""
    from _guided_util import report

    if units:
        u = 2.0 ** -24 * float(want.abs().max())
        print(f"{name}: e_hip = {float((hip.double() - want).abs().max()) / u:.2f} u  "
              f"e_torch = {float((t32.double() - want).abs().max()) / u:.1f} u")
    return report(name, hip, t32, want, factor=factor, what="grad")[0]


def check_full_grad(name, m, y, x, g, guide=None, units=(True, True, True)):
    """The gradients of y, x and omega of the ``full_cov, full_cov_grad`` module m on the kernels against fp32 and float64
    torch autograd on the device, under the rule; on the correlated guide with more than one channel and a window of more
    than one pixel also |full - diagonal| >= 1000 e_hip for each gradient, the diagonal one from phl.guided_filter_grad.
    Returns the kernels' gradients."""
    import phl
    from _guided_util import grads

    assert m.full_cov and m.full_cov_grad
    with spy() as calls:
        hip = grads(m, y, x, g, torch.float32)
    assert calls == ROUTE, (name, calls)
    m.full_cov_grad = False
    with spy() as calls:
        t32 = grads(m, y, x, g, torch.float32)
    assert calls["hip"] == 0 and calls["hip_grad"] == 0 and calls["hip_full_grad"] == 0 and calls["box_sum"] > 0
    want = grads(m.double(), y, x, g, torch.float64)
    m.float()
    m.full_cov_grad = True
    e = [rule(f"{name} grad_{k}", a, b, c, units=un) for k, a, b, c, un in zip(("y", "x", "omega"), hip, t32, want, units)]
    r, s, scale, sub = module_call(m)
    if guide == "correlated" and x.shape[1] > 1 and r // s >= 1:
        dy, dx, de = phl.guided_filter_grad(y, x, g, r, m.eps, subsample=s, scale=scale, subtract_is_y=sub, need_y=True, need_x=True,
                                            need_eps=True)
        for k, a, d, e_hip in zip(("y", "x", "omega"), hip, (dy, dx, omega_grad(de, m.omega.detach())), e):
            gap = float((a - d).abs().max())
            print(f"{name} grad_{k}: |full - diagonal| = {gap:.3e} = {gap / max(e_hip, 1e-300):.3g} e_hip")
            assert gap >= 1000 * e_hip, (name, k, gap, e_hip)
    return hip


def full_grad_case(kind, B, cy, cx, H, W, r, s, eps, guide, seed=0, noncontiguous=False, units=(True, True, True)):
    from _guided_util import DEV, module

    y, x, g = grad_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    m = module(kind, cx, r, s, eps, full_cov=True, full_cov_grad=True).to(DEV)
    name = f"full grad {kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g} {guide}"
    return check_full_grad(name, m, y, x, g, guide, units)
