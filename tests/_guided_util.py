"""What the guided-filter tests share beyond the fixtures (_guided_fixtures.py), organised around one table of the four
kernel routes, VARIANTS: nearest or bilinear interpolation, each with the diagonal or the full-covariance model -- the
table of crf/guided.py read from the tests' side.  On it: one spy of every phl.guided_filter* function with ``route``,
one module builder, the accuracy rule (``report``), the two input recipes, one forward and one gradient check, one closed
form of the full-covariance gradients (float64 torch ops, pinned to float64 autograd by the CPU tests, so that the kernels
are held to a formula that is checked where no GPU is needed), the explicit-loop model in numpy that the float64 torch
form of the full covariance is pinned to (the reference's own lines for this model are commented out,
gaussian_matrix.py:204-212, so no fixture of it can be generated), and the test bodies that the variants' files have in
common.  DEV, spy, route and report also serve tests outside the guided filter."""
import collections
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0)
MIN_U = 8
GUIDES = ("uniform", "correlated")
ALL = dict(need_y=True, need_x=True, need_eps=True)

# ---- the four variants --------------------------------------------------------------------------------------------------
# ctor: the constructor keywords that select the route; grad_kw: the keyword that puts its recorded forward on the kernels;
# forward, backward, function: their names in phl; call: the extra arguments of the direct phl calls; diagonal: the
# variant that the full-covariance checks compare against; tag: how the case names of its sweeps begin.
Variant = collections.namedtuple("Variant", "ctor grad_kw forward backward function call diagonal tag")
NEAREST, NEAREST_FULL, BILINEAR, BILINEAR_FULL = ("nearest", "diagonal"), ("nearest", "full"), ("bilinear", "diagonal"), ("bilinear", "full")
_BIL = dict(mode="bilinear", fused_bilinear=True)
VARIANTS = {
    NEAREST: Variant({}, "fused_grad", "guided_filter", "guided_filter_grad", "GuidedFilterFn", {}, None, ""),
    NEAREST_FULL: Variant(dict(full_cov=True), "full_cov_grad", "guided_filter", "guided_filter_full_grad", "GuidedFilterFullFn",
                          dict(full_cov=True), NEAREST, "full "),
    BILINEAR: Variant(_BIL, "bilinear_grad", "guided_filter_bilinear", "guided_filter_bilinear_grad", "GuidedFilterBilinearFn", {},
                      None, "bilinear "),
    BILINEAR_FULL: Variant(dict(_BIL, full_cov=True), "bilinear_full_grad", "guided_filter_bilinear", "guided_filter_bilinear_full_grad",
                           "GuidedFilterBilinearFullFn", dict(full_cov=True), BILINEAR, "bilinear full "),
}

# ---- the spy --------------------------------------------------------------------------------------------------------------
SPIED = {"nearest": "guided_filter", "nearest_grad": "guided_filter_grad", "nearest_full_grad": "guided_filter_full_grad",
         "bilinear": "guided_filter_bilinear", "bilinear_grad": "guided_filter_bilinear_grad",
         "bilinear_full_grad": "guided_filter_bilinear_full_grad"}
_KEY = {name: key for key, name in SPIED.items()}


@contextlib.contextmanager
def spy():
    """Counts of the calls of the six phl.guided_filter* functions (keys of SPIED) and of crf.guided._box_sum ("box_sum")."""
    import phl
    from crf import guided

    where = {key: (phl, name) for key, name in SPIED.items()}
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
    return {**{key: 0 for key in list(SPIED) + ["box_sum"]}, **counts}


def kernel_route(variant, n=1, grad=True):
    """n calls of the variant's forward and (``grad``) of its backward, nothing else."""
    v = VARIANTS[variant]
    return route(**{_KEY[v.forward]: n}, **({_KEY[v.backward]: n} if grad else {}))


def torch_route(calls):
    """What ``calls`` must equal where the torch form ran alone: its own box sums, at least one, and no kernel."""
    assert calls["box_sum"] > 0, calls
    return route(box_sum=calls["box_sum"])


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


# ---- the accuracy rule ----------------------------------------------------------------------------------------------------
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


def rule(name, hip, t32, want, factor=1, units=True, min_torch_u=None):
    """``report`` of a gradient; ``units``: both errors are first printed in u = 2^-24 max|want| too, with no precondition
    in u.  Returns e_hip and max|want|."""
    if units:
        u = 2.0 ** -24 * float(want.abs().max())
        print(f"{name}: e_hip = {float((hip.double() - want).abs().max()) / u:.2f} u  "
              f"e_torch = {float((t32.double() - want).abs().max()) / u:.1f} u")
    e_hip, _, mag = report(name, hip, t32, want, factor=factor, what="grad", min_torch_u=min_torch_u)
    return e_hip, mag


# ---- modules and inputs ---------------------------------------------------------------------------------------------------
def module(kind, cx, r, s, eps, variant=NEAREST, **kw):
    """GuidedFilter ("gf", which has no s), FastGuidedFilter ("fast") or BatchedGuidedAdjacency of the variant; ``kw``
    adds to the variant's constructor keywords or overrides them."""
    from crf import guided

    kw = {**VARIANTS[variant].ctor, **kw}
    if kind == "gf":
        return guided.GuidedFilter(cx, r, eps, **kw)
    return (guided.FastGuidedFilter if kind == "fast" else guided.BatchedGuidedAdjacency)(cx, r, eps, subsample_ratio=s, **kw)


def module_call(m):
    """(r, s, scale, subtract_is_y) of the phl call that module m makes."""
    r, s = m._r, getattr(m, "subsample_ratio", 1)
    adjacency = type(m).__name__ == "BatchedGuidedAdjacency"
    return r, s, 0.5 * (2 * r + 1) ** 2 if adjacency else 1.0, adjacency


def grads(m, y, x, g, dtype):
    yy, xx = y.detach().to(dtype).requires_grad_(True), x.detach().to(dtype).requires_grad_(True)
    m.omega.grad = None
    (m(yy, xx) * g.to(dtype)).sum().backward()
    return yy.grad, xx.grad, m.omega.grad.clone()


def omega_grad(grad_eps, omega):
    """The gradient of omega from that of eps = softplus(omega)."""
    return grad_eps * torch.sigmoid(omega)


def _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, with_g):
    """The first recipe: y, x and (``with_g``) the upstream gradient g, drawn in this order from one generator."""
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


def full_inputs(B, cy, cx, H, W, guide, seed, noncontiguous=False):
    """The second recipe: y uniform in [0, 1); the guide of independent uniform channels, or the correlated one.
    ``noncontiguous``: y channels-last, x every other column of a wider tensor."""
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


def grad_inputs(B, cy, cx, H, W, guide, seed, noncontiguous=False):
    """y, x of full_inputs and an upstream gradient g in [-1, 1) from seed + 1000 (``noncontiguous``: a transposed one)."""
    y, x = full_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    gen = torch.Generator(device=DEV).manual_seed(seed + 1000)
    if noncontiguous:
        g = (torch.rand((B, cy, W, H), device=DEV, generator=gen) * 2 - 1).transpose(2, 3)
        assert not g.is_contiguous()
    else:
        g = torch.rand((B, cy, H, W), device=DEV, generator=gen) * 2 - 1
    return y, x, g


# ---- the two checks -------------------------------------------------------------------------------------------------------
def _has_off_diagonal_terms(variant, guide, x, r, s):
    """Where the full model has off-diagonal terms to use: on the correlated guide, with more than one channel and a
    window of more than one pixel."""
    return VARIANTS[variant].diagonal is not None and guide == "correlated" and x.shape[1] > 1 and r // s >= 1


def check_forward(variant, name, m, y, x, guide=None, min_torch_u=MIN_U, absolute=False, use_out=False, off_diagonal=None):
    """The forward of the variant's module m on the kernels (``use_out``: the direct phl call into a NaN-filled ``out``)
    against its fp32 and float64 torch forms on the device: e_hip <= e_torch, no margin, under the precondition e_torch >=
    min_torch_u u.  ``off_diagonal`` (default: where the full model has such terms): also max|full - diagonal| >= 1000
    e_hip, the diagonal model on its own kernels.  Returns the kernels' output and e_hip in u (``absolute``: as it is)."""
    import phl

    v = VARIANTS[variant]
    assert all(getattr(m, k) == val for k, val in v.ctor.items())
    r, s, scale, sub = module_call(m)
    kw = dict(subsample=s, scale=scale, subtract=y if sub else None)
    with torch.no_grad():
        if use_out:
            out = torch.full(y.shape, float("nan"), device=y.device)
            hip = getattr(phl, v.forward)(y, x, r, m.eps, out=out, **kw, **v.call)
            assert hip is out
        else:
            with spy() as calls:
                hip = m(y, x)
            assert calls == kernel_route(variant, grad=False), (name, calls)
        with torch_form():
            t32 = m(y, x)
            want = m.double()(y.double(), x.double())
        m.float()
        e_hip, _, mag = report(name, hip, t32, want, min_torch_u=min_torch_u)
        if off_diagonal is None:
            off_diagonal = _has_off_diagonal_terms(variant, guide, x, r, s)
        if off_diagonal:
            diag = getattr(phl, VARIANTS[v.diagonal].forward)(y, x, r, m.eps, **kw)
            gap = float((hip - diag).abs().max())
            print(f"{name}: |full - diagonal| = {gap:.3e} = {gap / max(e_hip, 1e-300):.3g} e_hip")
            assert gap >= 1000 * e_hip, (name, gap, e_hip)
    return hip, e_hip if absolute else e_hip / (2.0 ** -24 * mag)


def check_grad(variant, name, m, y, x, g, guide=None, min_torch_u=None, absolute=(), units=(False, False, False)):
    """The gradients of y, x and omega of the variant's module m, its gradient keyword on, on the kernels against fp32
    and float64 torch autograd of the same module on the device: e_hip <= e_torch, no margin, under the precondition
    e_torch >= min_torch_u u (``absolute``: the gradients whose exact value is 0 -- no precondition, no u; ``units``: the
    gradients whose errors are printed in u without a precondition).  Where the full model has off-diagonal terms also
    |full - diagonal| >= 1000 e_hip for each gradient, the diagonal one from the diagonal variant's backward.  Leaves m in
    fp32 with the keyword off.  Returns the kernels' gradients and the largest e_hip in u."""
    import phl

    v = VARIANTS[variant]
    assert all(getattr(m, k) == val for k, val in v.ctor.items()) and getattr(m, v.grad_kw)
    with spy() as calls:
        hip = grads(m, y, x, g, torch.float32)
    assert calls == kernel_route(variant), (name, calls)
    setattr(m, v.grad_kw, False)
    with spy() as calls:
        t32 = grads(m, y, x, g, torch.float32)
    assert calls == torch_route(calls), (name, calls)
    want = grads(m.double(), y, x, g, torch.float64)
    m.float()
    e, worst = [], 0.0
    for k, a, b, c, un in zip(("y", "x", "omega"), hip, t32, want, units):
        e_hip, mag = rule(f"{name} grad_{k}", a, b, c, units=un, min_torch_u=None if k in absolute else min_torch_u)
        e.append(e_hip)
        if k not in absolute:
            worst = max(worst, e_hip / (2.0 ** -24 * mag))
    r, s, scale, sub = module_call(m)
    if _has_off_diagonal_terms(variant, guide, x, r, s):
        dy, dx, de = getattr(phl, VARIANTS[v.diagonal].backward)(y, x, g, r, m.eps.detach(), subsample=s, scale=scale, subtract_is_y=sub,
                                                                  **ALL)
        for k, a, d, e_hip in zip(("y", "x", "omega"), hip, (dy, dx, omega_grad(de, m.omega.detach())), e):
            gap = float((a - d).abs().max())
            print(f"{name} grad_{k}: |full - diagonal| = {gap:.3e} = {gap / max(e_hip, 1e-300):.3g} e_hip")
            assert gap >= 1000 * e_hip, (name, k, gap, e_hip)
    return hip, worst


# ---- the cases of the sweeps: inputs of a recipe, the variant's module, a check -------------------------------------------
def sweep_case(kind, B, cy, cx, H, W, r, s, eps, seed=0, noncontiguous=False, use_out=False, min_torch_u=None):
    """The nearest diagonal forward on inputs of the first recipe.  Returns the module, its inputs and the kernels' output."""
    y, x, _ = _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, False)
    m = module(kind, cx, r, s, eps).to(DEV)
    name = f"{kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g}"
    hip, _ = check_forward(NEAREST, name, m, y, x, min_torch_u=min_torch_u, use_out=use_out)
    return {"name": name, "m": m, "y": y, "x": x, "hip": hip}


def full_case(kind, B, cy, cx, H, W, r, s, eps, guide, seed=0, noncontiguous=False, use_out=False):
    """The nearest full-covariance forward on inputs of the second recipe."""
    y, x = full_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    m = module(kind, cx, r, s, eps, NEAREST_FULL).to(DEV)
    name = f"full {kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g} {guide}"
    hip, u = check_forward(NEAREST_FULL, name, m, y, x, guide, use_out=use_out)
    return {"name": name, "m": m, "y": y, "x": x, "hip": hip, "e_hip_u": u}


def sweep_case_grad(kind, B, cy, cx, H, W, r, s, eps, seed=0, noncontiguous=False, min_torch_u=None, variant=NEAREST):
    """The gradients of a diagonal variant on inputs of the first recipe.  Returns the module (fp32, the keyword off), its
    inputs, the kernels' gradients and the largest e_hip in u."""
    v = VARIANTS[variant]
    y, x, g = _sweep_inputs(B, cy, cx, H, W, seed, noncontiguous, True)
    name = f"{v.tag}{kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g}"
    m = module(kind, cx, r, s, eps, variant, **{v.grad_kw: True}).to(DEV)
    hip, worst = check_grad(variant, name, m, y, x, g, min_torch_u=min_torch_u)
    return {"name": name, "m": m, "y": y, "x": x, "g": g, "hip": hip, "u": worst}


def full_grad_case(kind, B, cy, cx, H, W, r, s, eps, guide, seed=0, noncontiguous=False, variant=NEAREST_FULL, **check):
    """The gradients of a full-covariance variant on inputs of the second recipe; ``check`` goes to check_grad."""
    v = VARIANTS[variant]
    y, x, g = grad_inputs(B, cy, cx, H, W, guide, seed, noncontiguous)
    m = module(kind, cx, r, s, eps, variant, **{v.grad_kw: True}).to(DEV)
    name = f"{v.tag}grad {kind} B{B} cy{cy} cx{cx} {H}x{W} r{r} s{s} eps{eps:g} {guide}"
    hip, worst = check_grad(variant, name, m, y, x, g, guide, **check)
    return {"name": name, "m": m, "y": y, "x": x, "g": g, "hip": hip, "u": worst}


# ---- test bodies that the variants' files share ---------------------------------------------------------------------------
def check_need_combinations(variant, y, x, g, eps):
    """Every combination of the need flags returns None where nothing is asked and the bits of the all-needs call where
    something is, at r = 4, subsample 2 in the adjacency form."""
    import phl

    backward = getattr(phl, VARIANTS[variant].backward)
    kw = dict(subsample=2, scale=40.5, subtract_is_y=True)
    full = backward(y, x, g, 4, eps, **ALL, **kw)
    assert all(t is not None and torch.isfinite(t).all() for t in full)
    for ny in (False, True):
        for nx in (False, True):
            for ne in (False, True):
                got = backward(y, x, g, 4, eps, need_y=ny, need_x=nx, need_eps=ne, **kw)
                for want, asked, have in zip(full, (ny, nx, ne), got):
                    assert (have is None) if not asked else torch.equal(have, want), (ny, nx, ne)
    assert tuple(t.shape for t in full) == (y.shape, x.shape, tuple(eps.shape))


def check_deterministic(variant, y, x, g=None):
    """Two calls of the variant's forward (without g) or backward return the same, finite bits, at r = 20, subsample 2 in
    the adjacency form."""
    import phl

    v = VARIANTS[variant]
    if g is None:
        call = lambda: (getattr(phl, v.forward)(y, x, 20, 1e-5, subsample=2, scale=840.5, subtract=y, **v.call),)  # noqa: E731
    else:
        call = lambda: getattr(phl, v.backward)(y, x, g, 20, 1e-5, subsample=2, scale=840.5, subtract_is_y=True, **ALL)  # noqa: E731
    for a, b in zip(call(), call()):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def check_noncontiguous_and_determinism(variant, res):
    """``res``: a gradient case on non-contiguous y, x and g.  The direct backward call returns the same bits twice, the
    same bits on contiguous copies, and those that the module's backward got."""
    import phl

    backward = getattr(phl, VARIANTS[variant].backward)
    y, x, g, m = res["y"], res["x"], res["g"], res["m"]
    assert not y.is_contiguous() and not x.is_contiguous() and not g.is_contiguous()
    r, s, scale, sub = module_call(m)
    kw = dict(subsample=s, scale=scale, subtract_is_y=sub, **ALL)
    e = m.eps.detach()
    a = backward(y, x, g, r, e, **kw)
    b = backward(y, x, g, r, e, **kw)
    c = backward(y.contiguous(), x.contiguous(), g.contiguous(), r, e, **kw)
    for u, v, w_ in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w_)                         # the same bits on every call
    assert torch.equal(a[0], res["hip"][0]) and torch.equal(a[1], res["hip"][1])  # the module made this call


def check_function_honours_needs_input_grad(variant, y, x, g, eps):
    """The variant's Function saves y, x and eps themselves and nothing else, returns the bits of the variant's forward
    call, and asks its backward only for the gradients autograd needs, in one call; that of eps has eps's shape."""
    import phl

    v = VARIANTS[variant]
    seen = []
    real = getattr(phl, v.backward)

    def f(*a, **k):
        seen.append((k["need_y"], k["need_x"], k["need_eps"]))
        return real(*a, **k)

    setattr(phl, v.backward, f)
    try:
        for ny, nx, ne in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
            yy, xx, ee = y.clone().requires_grad_(ny), x.clone().requires_grad_(nx), eps.clone().requires_grad_(ne)
            out = getattr(phl, v.function).apply(yy, xx, ee, 4, 2, 1.0, False)
            saved = out.grad_fn.saved_tensors
            assert len(saved) == 3 and [t.data_ptr() for t in saved] == [yy.data_ptr(), xx.data_ptr(), ee.data_ptr()]
            assert [t.shape for t in saved] == [y.shape, x.shape, eps.shape]
            with torch.no_grad():
                assert torch.equal(out, getattr(phl, v.forward)(y, x, 4, eps, subsample=2, **v.call))
            (out * g).sum().backward()
            assert seen[-1] == (ny, nx, ne)
            assert (yy.grad is not None) == ny and (xx.grad is not None) == nx and (ee.grad is not None) == ne
            assert ee.grad is None or ee.grad.shape == eps.shape
    finally:
        setattr(phl, v.backward, real)
    assert len(seen) == 4


def check_autograd_keeps_the_torch_form(variant, y, x, label, **kw):
    """The variant's adjacency module without its gradient keyword (``kw``: other constructor keywords): with autograd
    recording, also for omega alone, the torch form runs and no kernel; its fp32 gradients of y and omega are those of the
    float64 torch form within 1e-3 of each gradient's largest magnitude (the reasoning: tests/test_gpu_guided.py); with
    grad mode off, the kernels.  y requires grad."""
    m = module("bga", x.shape[1], 4, 2, 1e-2, variant, **kw).to(DEV)
    with spy() as calls:
        m(y, x).square().sum().backward()
    assert calls == torch_route(calls)
    y64 = y.detach().double().requires_grad_(True)
    m64 = module("bga", x.shape[1], 4, 2, 1e-2, variant).to(DEV).double()
    with torch.no_grad():
        m64.omega.copy_(m.omega.double())
    m64(y64, x.double()).square().sum().backward()
    for name, got, want in (("y", y.grad, y64.grad), ("omega", m.omega.grad, m64.omega.grad)):
        err, mag = float((got.double() - want).abs().max()), float(want.abs().max())
        print(f"{label} {name}: |fp32 - float64| = {err:.3e} of {mag:.3e}")
        assert err <= 1e-3 * mag, (name, err, mag)
    with spy() as calls:                       # omega alone asks for a gradient: still the torch form
        m(y.detach(), x)
    assert calls == torch_route(calls)
    with torch.no_grad(), spy() as calls:
        m(y, x)
    assert calls == kernel_route(variant, grad=False)


# ---- the closed form of the full-covariance gradients -----------------------------------------------------------------------
def _nearest(n_in, n_out, device="cpu"):
    """torch's nearest map: the index in n_in that each of n_out takes."""
    if n_in == n_out:
        return torch.arange(n_in, device=device)
    src = torch.arange(n_in, dtype=torch.float32, device=device).reshape(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(n_out).long()


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


def _resampling(mode, H, W, h, w, dev):
    """(D, U, Dt, Ut): the sample to (h, w), the upsample to (H, W) and their adjoints.  Bilinear: F.interpolate and its
    vector-Jacobian product.  Nearest: torch's index maps, with adjoints by index (the vector-Jacobian product gives the
    same up to 1.2e-13 of a gradient's magnitude, too close to the CPU tests' 1e-12 to swap it in)."""
    if mode == "bilinear":
        return (lambda t: _interp(t, (h, w)), lambda t: _interp(t, (H, W)),
                lambda t: _interp_adjoint(t, (H, W)), lambda t: _interp_adjoint(t, (h, w)))
    rows, cols, rlow, clow = _nearest(H, h, dev), _nearest(W, w, dev), _nearest(h, H, dev), _nearest(w, W, dev)

    def scatter(t):                                                     # adjoint of the sample (the maps are strictly increasing)
        out = torch.zeros(t.shape[:-2] + (H, W), dtype=t.dtype, device=dev)
        out[..., rows[:, None], cols[None, :]] = t
        return out

    def down(t):                                                        # adjoint of the upsample: sums over the pre-images
        a = torch.zeros(t.shape[:-2] + (h, W), dtype=t.dtype, device=dev).index_add_(-2, rlow, t)
        return torch.zeros(t.shape[:-2] + (h, w), dtype=t.dtype, device=dev).index_add_(-1, clow, a)

    return lambda t: t[..., rows, :][..., cols], lambda t: t[..., rlow, :][..., clow], scatter, down


def closed_form_grads(y, x, g, r, eps, s=1, scale=1.0, subtract_is_y=False, mode="nearest"):
    """(grad_y, grad_x, grad_eps) of ``sum(out * g)``, out = guided_full(y, x) * scale - (y if subtract_is_y else 0): the
    full-covariance model solved on D(y), D(x) at (H // s, W // s) with radius r // s and eps [cx], its window means
    brought back by U; D and U of ``mode``.  Notation of phl_guided.hip."""
    from crf.guided import _box_sum

    n, cy, H, W = y.shape
    cx = x.shape[1]
    h, w, rr, dev = H // s, W // s, r // s, y.device
    D, U, Dt, Ut = _resampling(mode, H, W, h, w, dev)

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


# ---- the explicit-loop model ------------------------------------------------------------------------------------------------
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
    rows, cols, rlow, clow = (_nearest(a, b).numpy() for a, b in ((H, h), (W, w), (h, H), (w, W)))
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
