"""Guided-filter adjacency operators and the separable Gaussian blur behind GuidedFilter(gaussian=True).

The reference's CRFasRNN defaults to a guided-filter W (crf/gaussian_matrix.py:161-287, crf_module.py:91).  The
box-window classes (GuidedFilter, FastGuidedFilter, BatchedGuidedAdjacency, GuidedAdjacency) keep the reference's
constructor / call signatures.  Their torch form below is pinned to the reference run in float64 with its own
``mBoxFilter`` as the box sum (tests/golden/generate_guided.py, tests/test_guided_cpu.py).  On fp32 CUDA tensors the
forward runs on the HIP kernels instead (phl_guided.hip: fp64 window sums over LDS tiles, the ``* k - src`` of the
adjacency fused), a forward that autograd records under a keyword only: _guided_route holds the table of the routes
and their keywords, _check_guided_keywords the rules between the keywords.  Around such a forward, CRFasRNN runs the rest
of its iteration -- Mu, the add and the softmax -- as one channel-major kernel (phl.nchw_softmax_compat,
crf_module._mean_field_nchw_step), whichever form W itself takes.

``full_cov=True`` (keyword of all four classes) solves the guide channels together, A = cov_yx (cov_xx + diag(eps))^-1,
the model the reference keeps as commented lines (gaussian_matrix.py:204, 209-212) beside a memory print: its torch form
needs [n, h, w, cx, cx] tensors and a batched inverse; the kernels take up to phl.GUIDED_FULL_MAX_CX guide channels (the
inverse once per image, in registers).  ``mode='bilinear'`` of FastGuidedFilter / BatchedGuidedAdjacency solves the
coefficients on the bilinearly down-sampled images and interpolates them back up (the taps are computed on the device).

The learned-width variant, ``GuidedFilter(gaussian=True)``, needs the reference's own separable Gaussian
(gaussian_matrix.py:86-156), which is provided here with the reference's semantics, quirks included:
    box_filter(x, r, dim)            one normalised box pass (window of 2r samples, divisor of 2r+1: see _box_torch)
    gaussian_blur(x, sigma, dim)     three box passes, r = floor(sqrt(4 sigma^2 + 1)) // 2, with a sigma gradient
    GaussianBlur                     the autograd Function behind it
fp32 CUDA tensors run on the HIP kernels (phl.box_blur / phl.box_blur_grad: one fused pass over the data per blur and
per gradient); anything else (CPU tensors, float64) runs the plain-torch transcription below.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import phl


def _box_torch(x, r, dim):
    """B_r along dim, from the formula: out[i] = (P[min(h, i+r+1)] - P[max(0, i-r+1)]) / c(i), P the exclusive prefix
    sum, c(i) = min(i, r) + min(h-1-i, r) + 1.  The window holds at most 2r samples (i-r+1 .. i+r) while c counts the
    symmetric 2r+1 -- the reference's cumsum slices, kept as they are."""
    h = x.shape[dim]
    P = torch.cat([torch.zeros_like(x.narrow(dim, 0, 1)), x.cumsum(dim)], dim)
    i = torch.arange(h, device=x.device)
    hi = torch.clamp(i + r + 1, max=h)
    lo = torch.clamp(i - r + 1, min=0)
    c = (torch.clamp(i, max=r) + torch.clamp(h - 1 - i, max=r) + 1).to(x.dtype)
    shape = (1,) * dim + (h,) + (1,) * (x.dim() - dim - 1)
    return (P.index_select(dim, hi) - P.index_select(dim, lo)) / c.reshape(shape)


def _hip_ok(x):
    return x.is_cuda and x.dtype == torch.float32


def _cascade(x, r, dim, passes=3):
    if _hip_ok(x):
        return phl.box_blur(x, r, dim, passes=passes)
    for _ in range(passes):
        x = _box_torch(x, r, dim)
    return x


def box_filter(array, r, dim):
    """One normalised box pass of radius r >= 1 along ``dim`` (gaussian_matrix.py:86-105)."""
    r = int(r)
    if r < 1:
        raise ValueError(f"box_filter: r must be >= 1, got {r}")
    return _cascade(array, r, dim, passes=1)


def sigma_radius(sigma, niters=3):
    """The box radius of the reference: floor(sqrt(12 sigma^2 / niters + 1)) // 2, computed with torch ops in sigma's
    own dtype on the CPU (float32 and float64 differ where 4 sigma^2 + 1 = (2k)^2).  One device read for a GPU sigma."""
    s = sigma.detach().cpu() if torch.is_tensor(sigma) else torch.as_tensor(sigma)
    return int(torch.floor(torch.sqrt(12 * s ** 2 / niters + 1)) // 2)


def gaussian_blur(array, sigma, dim):
    return GaussianBlur.apply(array, sigma, dim)


class GaussianBlur(torch.autograd.Function):
    """Three box passes along ``dim`` approximating a Gaussian of width sigma (gaussian_matrix.py:110-156).  sigma is a
    number or a 0-d tensor; only a tensor that requires grad receives a gradient.  The backward is the reference's:
        grad_x     = B(g)                      (the forward operator, not its transpose)
        grad_sigma = -sum(grad_f f) / sigma - sum(B(g) v) / sigma,  f[i] = i / sigma,
        grad_f     = -(v f B(g) - v B(g f) + g f B(v) - g B(v f))
    the continuous Gaussian's sigma-derivative, not that of the (piecewise constant in sigma) discrete operator -- so
    gradcheck does not apply.  No double backward, as in the reference."""

    @staticmethod
    def forward(ctx, array, sigma, dim, niters=3):
        r = sigma_radius(sigma, niters)
        if r < 1:
            raise ValueError(f"gaussian_blur: sigma = {float(sigma)} gives box radius {r}; needs r >= 1")
        ctx.dim, ctx.r = dim, r
        ctx.sigma_is_tensor = torch.is_tensor(sigma)
        if ctx.sigma_is_tensor:
            ctx.save_for_backward(array, sigma)
        else:
            ctx.save_for_backward(array)
            ctx.sigma = sigma
        with torch.no_grad():
            return _cascade(array, r, dim, niters)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        if ctx.sigma_is_tensor:
            v, sigma = ctx.saved_tensors
        else:
            (v,), sigma = ctx.saved_tensors, ctx.sigma
        need_x = ctx.needs_input_grad[0]
        need_s = ctx.sigma_is_tensor and ctx.needs_input_grad[1]
        dim, r = ctx.dim, ctx.r
        g = grad_output
        grad_x = grad_sigma = None
        if not (need_x or need_s):
            return None, None, None, None
        if _hip_ok(v) and _hip_ok(g):
            grad_x, grad_sigma = phl.box_blur_grad(v, g, r, dim, float(sigma), need_x=need_x, need_sigma=need_s)
        else:
            g = g.to(v.dtype)
            Bg = _cascade(g, r, dim)
            grad_x = Bg if need_x else None
            if need_s:
                h = v.shape[dim]
                shape = (1,) * dim + (h,) + (1,) * (v.dim() - dim - 1)
                f = (torch.arange(h) / sigma.detach().cpu()).reshape(shape).to(v.dtype).to(v.device)
                gf, vf = g * f, v * f
                grad_f = -(vf * Bg - v * _cascade(gf, r, dim) + gf * _cascade(v, r, dim) - g * _cascade(vf, r, dim))
                s = sigma.detach().to(v.device)
                grad_sigma = -(grad_f * f).sum() / s - (Bg * v).sum() / s
        if grad_sigma is not None:
            grad_sigma = grad_sigma.to(dtype=sigma.dtype, device=sigma.device).reshape(sigma.shape)
        return grad_x, grad_sigma, None, None


def _box_sum(x, r):
    """Sum over a (2r+1)^2 window with zero padding, NCHW, via 2-D prefix sums."""
    c = F.pad(x, (r + 1, r, r + 1, r)).cumsum(2).cumsum(3)
    k = 2 * r + 1
    return c[:, :, k:, k:] - c[:, :, :-k, k:] - c[:, :, k:, :-k] + c[:, :, :-k, :-k]


def _check_guided_keywords(*, gaussian=False, full_cov=False, full_cov_grad=False, fast=False, mode="nearest", fused_bilinear=False,
                           bilinear_grad=False, bilinear_full_grad=False, needs_only=False):
    """Every rule between the keywords of the guided-filter classes, in the order that decides which exception a call gets
    that breaks two of them.  GuidedFilter hands over its keywords, FastGuidedFilter (``fast``) its own on top.  needs_only:
    the "a needs b" rules alone, which CRFasRNN raises ahead of the window and the mode, and for a lattice W too."""
    rest = not needs_only
    if rest and gaussian and full_cov:
        raise NotImplementedError("gaussian=True with full_cov=True: the full covariance has the box window only")
    if full_cov_grad and not full_cov:
        raise ValueError("full_cov_grad=True is the backward of the full-covariance model: it needs full_cov=True")
    if rest and fast and gaussian:
        # the reference's constructor reads self._r, which its gaussian form never sets (AttributeError, :238)
        raise NotImplementedError("FastGuidedFilter(gaussian=True) does not construct in the reference either")
    if rest and fused_bilinear and mode != "bilinear":
        raise ValueError(f"fused_bilinear=True is the kernel route of mode='bilinear', got mode={mode!r}")
    if bilinear_grad and not fused_bilinear:
        raise ValueError("bilinear_grad=True is the backward of the fused_bilinear route: it needs fused_bilinear=True")
    if rest and bilinear_grad and full_cov:
        raise NotImplementedError("bilinear_grad=True with full_cov=True: this keyword has the diagonal model only "
                                  "(the full covariance: bilinear_full_grad=True)")
    if bilinear_full_grad and not (fused_bilinear and full_cov):
        raise ValueError("bilinear_full_grad=True is the backward of the fused_bilinear route with the full covariance: it needs "
                         "fused_bilinear=True and full_cov=True")


def _guided_route(gaussian, mode, fused_bilinear, full_cov, subsample, operands_ok, recording, fused_grad, full_cov_grad,
                  bilinear_grad, bilinear_full_grad):
    """The route of one guided-filter call, from plain values: "torch", or (bilinear_kernels, full_cov, recorded) -- the key
    of _KERNELS, and whether the forward is the route's Function (autograd records it) or its plain phl call.

        mode      | further preconditions          | a recorded forward needs            | route
        nearest   | not full_cov                   | fused_grad                          | (False, False, recording)
        nearest   | full_cov                       | full_cov_grad                       | (False, True, recording)
        bilinear  | fused_bilinear, subsample >= 2 | bilinear_grad or bilinear_full_grad | (True, full_cov, recording)
        bilinear  | fused_bilinear, subsample 1    | bilinear_grad or bilinear_full_grad | (False, full_cov, recording)
        anything else                                                                    | "torch"

    Every row: the box window (not gaussian) and operands_ok -- y, x and omega fp32 CUDA, y and x 4-D.  Two asymmetries, on
    purpose: either bilinear keyword admits a recorded bilinear forward whatever full_cov says (the constructor ties each
    to its model: _check_guided_keywords), and ``fused_grad`` and ``full_cov_grad`` do not; and at subsample 1, where both
    interpolations are the identity, the bilinear rows land on the nearest kernels and the nearest Function of their
    model.  More than 16 guide channels (with full_cov: phl.GUIDED_FULL_MAX_CX) are the torch form too: _fused finds out."""
    bilinear = mode == "bilinear" and fused_bilinear
    if gaussian or not (mode == "nearest" or bilinear) or not operands_ok:
        return "torch"
    keyword = (bilinear_grad or bilinear_full_grad) if bilinear else (full_cov_grad if full_cov else fused_grad)
    if recording and not keyword:
        return "torch"
    return bool(bilinear and subsample >= 2), bool(full_cov), bool(recording)


# (bilinear_kernels, full_cov) -> the forward and the Function of a recorded one.  By their names in phl, which _fused looks
# up at the call: what replaces a function of phl for a while (the call counters of the tests) is then what runs.
_KERNELS = {(False, False): ("guided_filter", "GuidedFilterFn"),
            (False, True): ("guided_filter", "GuidedFilterFullFn"),
            (True, False): ("guided_filter_bilinear", "GuidedFilterBilinearFn"),
            (True, True): ("guided_filter_bilinear", "GuidedFilterBilinearFullFn")}


class GuidedFilter(nn.Module):
    """y filtered by guide x with per-guide-channel (diagonal covariance) linear model,
    eps = softplus(omega) as in the reference's parametrisation (:161-232); with ``full_cov`` one linear model over all
    guide channels, through their covariance matrix (:204, :209-212)."""

    def __init__(self, channels=1, r=20, eps=1e-8, gaussian=False, *, fused_grad=False, full_cov=False, full_cov_grad=False):
        super().__init__()
        _check_guided_keywords(gaussian=gaussian, full_cov=full_cov, full_cov_grad=full_cov_grad)
        self.fused_grad, self.full_cov, self.full_cov_grad = fused_grad, full_cov, full_cov_grad
        # what FastGuidedFilter overwrites: _guided_route reads them of every class
        self.subsample_ratio, self.mode, self.fused_bilinear, self.bilinear_grad, self.bilinear_full_grad = 1, "nearest", False, False, False
        self.omega = nn.Parameter(torch.log(torch.expm1(torch.tensor(float(eps)))).expand(channels).clone())
        if gaussian:
            # pinned to the reference (tests/golden/blur_guided.npz): its fp32 log(exp(eps) - 1), not expm1 (:166)
            with torch.no_grad():
                self.omega.copy_(torch.log(torch.exp(torch.tensor(float(eps))) - 1).expand(channels))
            # learned window: the Gaussian's sigma is exp(omega2), initialised at r (:169-170)
            self.omega2 = nn.Parameter(torch.log(torch.tensor(r).float()))
        else:
            self._r = r
        self.gaussian = gaussian

    def r(self):
        return torch.exp(self.omega2) if self.gaussian else self._r

    @property
    def eps(self):
        return F.softplus(self.omega)

    def _window(self):
        return self._r

    def get_coeffs(self, y, x):
        n, cx, h, w = x.shape
        cy = y.shape[1]
        if self.gaussian:
            s = self.r()
            assert h > 2 * s + 1 and w > 2 * s + 1
            blur = lambda t: gaussian_blur(gaussian_blur(t, s, 2), s, 3)  # noqa: E731
        else:
            r = self._window()
            blur = lambda t: _box_sum(t, r)  # noqa: E731
        # N: the window weight of every pixel; in the Gaussian form it depends on sigma and is differentiated too
        N = blur(torch.ones((1, 1, h, w), dtype=x.dtype, device=x.device))
        mean = lambda t: blur(t) / N  # noqa: E731
        mx, my = mean(x), mean(y)
        cov = mean((y[:, :, None] * x[:, None]).reshape(n, cy * cx, h, w)).reshape(n, cy, cx, h, w) - my[:, :, None] * mx[:, None]
        if self.full_cov:
            # A = cov_yx @ inverse(cov_xx + eps * I), per pixel (:204, :209-212); eps * I broadcasts to diag(eps)
            cov_xx = mean((x[:, :, None] * x[:, None]).reshape(n, cx * cx, h, w)).reshape(n, cx, cx, h, w) - mx[:, :, None] * mx[:, None]
            P = torch.linalg.inv(cov_xx.permute(0, 3, 4, 1, 2) + torch.diag_embed(self.eps.expand(cx)))     # [n, h, w, cx, cx]
            A = (cov.permute(0, 3, 4, 1, 2) @ P).permute(0, 3, 4, 1, 2)
        else:
            var = mean(x * x) - mx * mx
            A = cov / (var[:, None] + self.eps.view(1, 1, -1, 1, 1))      # [n, cy, cx, h, w]
        b = my - (A * mx[:, None]).sum(2)
        mean_A = mean(A.reshape(n, cy * cx, h, w)).reshape(n, cy, cx, h, w)
        return mean_A, mean(b)

    def _fused(self, y, x, subsample=1, scale=1.0, subtract=None):
        """The forward on the HIP kernels, or None where the torch form has to run: where _guided_route says so, or at a
        shape the kernels do not take (PHL_ERR_UNSUPPORTED).  A recorded forward is the route's phl Function (eps =
        softplus(omega) keeps its graph); ``subtract`` is None or y itself."""
        operands_ok = _hip_ok(y) and _hip_ok(x) and y.dim() == 4 and x.dim() == 4 and _hip_ok(self.omega)
        recording = torch.is_grad_enabled() and (y.requires_grad or x.requires_grad or self.omega.requires_grad)
        route = _guided_route(self.gaussian, self.mode, self.fused_bilinear, self.full_cov, subsample, operands_ok, recording,
                              self.fused_grad, self.full_cov_grad, self.bilinear_grad, self.bilinear_full_grad)
        if route == "torch":
            return None
        bilinear_kernels, full_cov, recorded = route
        forward, function = (getattr(phl, name) for name in _KERNELS[bilinear_kernels, full_cov])
        try:
            if recorded:
                return function.apply(y, x, self.eps, self._r, subsample, scale, subtract is not None)
            return forward(y, x, self._r, self.eps, subsample=subsample, scale=scale, subtract=subtract, full_cov=full_cov)
        except phl.PhlError as e:
            if e.status != phl.ERR_UNSUPPORTED:
                raise
        return None

    def _torch_forward(self, y, x):
        mean_A, mean_b = self.get_coeffs(y, x)
        return (mean_A * x[:, None]).sum(2) + mean_b

    def forward(self, y, x):
        out = self._fused(y, x, subsample=self.subsample_ratio)
        return out if out is not None else self._torch_forward(y, x)


class FastGuidedFilter(GuidedFilter):
    """Coefficients solved at 1/subsample_ratio resolution and upsampled (:234-253)."""

    def __init__(self, *args, subsample_ratio=2, mode="nearest", fused_bilinear=False, bilinear_grad=False,
                 bilinear_full_grad=False, **kwargs):
        super().__init__(*args, **kwargs)
        _check_guided_keywords(gaussian=self.gaussian, full_cov=self.full_cov, fast=True, mode=mode, fused_bilinear=fused_bilinear,
                               bilinear_grad=bilinear_grad, bilinear_full_grad=bilinear_full_grad)
        self.subsample_ratio, self.mode, self.fused_bilinear = subsample_ratio, mode, fused_bilinear
        self.bilinear_grad, self.bilinear_full_grad = bilinear_grad, bilinear_full_grad

    def _window(self):
        return self._r // self.subsample_ratio

    def _torch_forward(self, y, x):
        s = self.subsample_ratio
        n, cx, h, w = x.shape
        cy = y.shape[1]
        lo = (h // s, w // s)
        A, b = self.get_coeffs(F.interpolate(y, size=lo, mode=self.mode), F.interpolate(x, size=lo, mode=self.mode))
        A = F.interpolate(A.reshape(n, cy * cx, *lo), size=(h, w), mode=self.mode).reshape(n, cy, cx, h, w)
        b = F.interpolate(b, size=(h, w), mode=self.mode)
        return (A * x[:, None]).sum(2) + b


class BatchedGuidedAdjacency(FastGuidedFilter):
    """W(src) = guided(src) * (2r+1)^2 / 2 - src  (:285-287)."""

    def forward(self, src_imgs, guide_imgs):
        out = self._fused(src_imgs, guide_imgs, subsample=self.subsample_ratio, scale=0.5 * (2 * self._r + 1) ** 2,
                          subtract=src_imgs)
        if out is not None:
            return out
        return self._torch_forward(src_imgs, guide_imgs) * 0.5 * (2 * self.r() + 1) ** 2 - src_imgs


class GuidedAdjacency(GuidedFilter):
    """Flat ``W @ U`` form used by Experiments/DenseCrf.ipynb cell 9: guide [1, C, H, W], U [n, L]."""

    def __init__(self, guide_img, r, eps, *, full_cov=False):
        super().__init__(guide_img.shape[1], r, eps, full_cov=full_cov)
        self.guide_img = guide_img.float()

    def __matmul__(self, U):
        h, w = self.guide_img.shape[-2:]
        # the guide's dtype: fp32 as constructed; a guide_img set to float64 keeps the whole product in float64
        img = U.t().reshape(1, -1, h, w).to(self.guide_img.dtype).to(self.guide_img.device)
        with torch.no_grad():
            out = self._fused(img, self.guide_img, scale=0.5 * (2 * self._r + 1) ** 2, subtract=img)
            if out is None:
                out = self._torch_forward(img, self.guide_img) * 0.5 * (2 * self._r + 1) ** 2 - img
        return out[0].reshape(U.shape[1], -1).t().to(U.device)
