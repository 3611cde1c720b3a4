"""What the tests of the full-covariance guided filter share (test_guided_full_cpu.py, test_gpu_guided_full.py): the
inputs of the affine-reproduction check, the correlated guide, and an explicit-loop model in numpy that the float64 torch
form is pinned to (the reference's own lines for this model are commented out, gaussian_matrix.py:204-212, so no fixture
of it can be generated)."""
import numpy as np
import torch
import torch.nn.functional as F


def correlated_guide(B, cx, H, W, gen, device="cpu", dtype=torch.float32):
    """x_c = base + 0.25 noise_c: channels that share most of their variance, as the channels of a colour image do."""
    base = torch.rand((B, 1, H, W), generator=gen, device=device, dtype=dtype)
    return base + 0.25 * torch.rand((B, cx, H, W), generator=gen, device=device, dtype=dtype)


def affine_inputs(device="cpu", dtype=torch.float64, seed=1):
    """A [1, 3, 40, 50] correlated guide and y = 0.3 x_0 - 0.5 x_1 + 0.2 x_2 + 0.1, which a linear model over all three
    channels reproduces (up to eps) and three separate models cannot."""
    gen = torch.Generator(device=device).manual_seed(seed)
    x = correlated_guide(1, 3, 40, 50, gen, device, dtype)
    y = (0.3 * x[:, 0] - 0.5 * x[:, 1] + 0.2 * x[:, 2] + 0.1)[:, None]
    return y, x


def _nearest(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float64).reshape(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(n_out).long().numpy()


def _window_mean(t, r):
    """Mean over the (2r+1)^2 window clipped to the image, of every [h, w] plane of t [..., h, w]."""
    h, w = t.shape[-2:]
    out = np.empty_like(t)
    for i in range(h):
        for j in range(w):
            out[..., i, j] = t[..., max(0, i - r):i + r + 1, max(0, j - r):j + r + 1].mean(axis=(-2, -1))
    return out


def brute_force(y, x, r, eps, s=1, scale=1.0, subtract=False):
    """The full-covariance guided filter by explicit loops, float64 numpy: y [n, cy, H, W], x [n, cx, H, W], eps [cx].
    Solved at (H // s, W // s) on torch's nearest samples with radius r // s, upsampled by torch's nearest maps."""
    n, cy, H, W = y.shape
    cx = x.shape[1]
    h, w = H // s, W // s
    rows, cols, rlow, clow = _nearest(H, h), _nearest(W, w), _nearest(h, H), _nearest(w, W)
    yl, xl = y[:, :, rows][:, :, :, cols], x[:, :, rows][:, :, :, cols]
    rr = r // s
    mx, my = _window_mean(xl, rr), _window_mean(yl, rr)
    mxx = _window_mean(xl[:, :, None] * xl[:, None], rr)
    myx = _window_mean(yl[:, :, None] * xl[:, None], rr)
    A, b = np.empty((n, cy, cx, h, w)), np.empty((n, cy, h, w))
    for k in range(n):
        for i in range(h):
            for j in range(w):
                S = mxx[k, :, :, i, j] - np.outer(mx[k, :, i, j], mx[k, :, i, j]) + np.diag(eps)
                cov = myx[k, :, :, i, j] - np.outer(my[k, :, i, j], mx[k, :, i, j])          # [cy, cx]
                A[k, :, :, i, j] = np.linalg.solve(S, cov.T).T                              # S is symmetric
                b[k, :, i, j] = my[k, :, i, j] - A[k, :, :, i, j] @ mx[k, :, i, j]
    mA, mb = _window_mean(A, rr), _window_mean(b, rr)
    mA, mb = mA[:, :, :, rlow][:, :, :, :, clow], mb[:, :, rlow][:, :, :, clow]
    out = ((mA * x[:, None]).sum(2) + mb) * scale
    return out - y if subtract else out


# ---- GPU: the accuracy rule of tests/test_gpu_guided.py for the full-covariance kernels ---------------------------
MIN_U = 8
GUIDES = ("uniform", "correlated")


def full_inputs(B, cy, cx, H, W, guide, seed, noncontiguous=False):
    """y uniform in [0, 1); the guide of independent uniform channels, or the correlated one.  ``noncontiguous``: the
    strides of test_sweep_noncontiguous_and_out (y channels-last, x every other column of a wider tensor)."""
    from _guided_util import DEV

    gen = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.rand((B, cy, H, W), device=DEV, generator=gen)
    x = torch.rand((B, cx, H, W), device=DEV, generator=gen) if guide == "uniform" else correlated_guide(B, cx, H, W, gen, DEV)
    if noncontiguous:
        y = y.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        wide = torch.zeros((B, cx, H, 2 * W), device=DEV)
        wide[..., ::2] = x
        x = wide[..., ::2]
        assert not y.is_contiguous() and not x.is_contiguous()
    return y, x


def check_full(name, m, y, x, guide=None, use_out=False, off_diagonal=None):
    """The forward of the ``full_cov`` module m on the kernels against its fp32 and float64 torch forms on the device:
    e_hip <= e_torch, no margin, under the precondition e_torch >= MIN_U u.  ``off_diagonal`` (default: on the correlated
    guide, where the model has off-diagonal terms to use -- more than one channel and a window of more than one pixel):
    also max|full - diagonal| >= 1000 e_hip, the diagonal model on its own kernels.  Returns the kernels' output and
    e_hip in u."""
    import phl
    from _guided_util import report, spy, torch_form

    assert m.full_cov
    r, s = m._r, getattr(m, "subsample_ratio", 1)
    adjacency = type(m).__name__ == "BatchedGuidedAdjacency"
    kw = dict(subsample=s, scale=0.5 * (2 * r + 1) ** 2 if adjacency else 1.0, subtract=y if adjacency else None)
    with torch.no_grad():
        if use_out:
            out = torch.full(y.shape, float("nan"), device=y.device)
            hip = phl.guided_filter(y, x, r, m.eps, out=out, full_cov=True, **kw)
            assert hip is out
        else:
            with spy() as calls:
                hip = m(y, x)
            assert calls == {"hip": 1, "box_sum": 0}, name
        with torch_form():
            t32 = m(y, x)
            want = m.double()(y.double(), x.double())
        m.float()
        e_hip, _, mag = report(name, hip, t32, want, min_torch_u=MIN_U)
        if off_diagonal is None:
            off_diagonal = guide == "correlated" and x.shape[1] > 1 and r // s >= 1
        if off_diagonal:
            diag = phl.guided_filter(y, x, r, m.eps, **kw)
            gap = float((hip - diag).abs().max())
            print(f"{name}: |full - diagonal| = {gap:.3e} = {gap / max(e_hip, 1e-300):.3g} e_hip")
            assert gap >= 1000 * e_hip, (name, gap, e_hip)
    return hip, e_hip / (2.0 ** -24 * mag)


def full_case(kind, B, cy, cx, H, W, r, s, eps, guide, seed=0, noncontiguous=False, use_out=False):
    from _guided_util import DEV, module

    y, x = full_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    m = module(kind, cx, r, s, eps, full_cov=True).to(DEV)
    name = f"full {kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g} {guide}"
    hip, u = check_full(name, m, y, x, guide, use_out)
    return {"name": name, "m": m, "y": y, "x": x, "hip": hip, "e_hip_u": u}
