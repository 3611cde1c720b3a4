"""The backward of the box-window guided filter on the HIP kernels (phl.guided_filter_grad, phl.GuidedFilterFn, the
``fused_grad`` keyword of the classes).

Rule of every accuracy check, the one of tests/test_gpu_guided.py applied to each gradient (y, x, omega): with g64 the
float64 gradient (the reference's fixture, or the torch form in float64 on the device), e_hip = max|hip - g64| and
e_torch = max|fp32 torch autograd - g64| over ALL elements, on the same device, and e_hip <= e_torch with no margin.
The end-to-end CRFasRNN case is held to e_hip <= 2 e_torch: the fp32 compatibility and softmax steps are common to both
paths.  Both numbers are printed."""
import functools

import pytest
import torch

import _guided_util as util
from _guided_grad_util import GRAD_CASES, load_grad_case, torch_form_grads
from _guided_util import DEV
from _guided_util import grads as _grads
from _guided_util import sweep_case_grad as _sweep_case

pytestmark = pytest.mark.gpu
spy = functools.partial(util.spy, grad=True)
_report = functools.partial(util.report, what="grad")


@pytest.mark.parametrize("name", GRAD_CASES)
def test_goldens(name):
    from crf import guided

    z = load_grad_case(name)
    with spy() as calls:
        hip = torch_form_grads(guided, z, torch.float32, DEV, fused_grad=True)
    assert calls == {"hip": 1, "hip_grad": 1, "box_sum": 0}
    t32 = torch_form_grads(guided, z, torch.float32, DEV)
    for k, a, b in zip(("y", "x", "omega"), hip, t32):
        _report(f"{name} grad_{k}", a, b, torch.from_numpy(z["grad_" + k]).to(DEV))


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 4, 20, 100])
def test_sweep_radius_and_subsample(r, s):
    kind = "gf" if s == 1 else "bga"
    _sweep_case(kind, 3, 5, 3, 61, 75, r, s, 1e-2, seed=r + s)


@pytest.mark.parametrize("dr", [0, 1, 25])
def test_sweep_both_sides_of_the_tiled_radius(dr):
    import phl

    r = phl.load_library().phl_guided_filter_grad_max_r() + dr
    _sweep_case("gf", 1, 2, 3, 203, 171, r, 1, 1e-2, seed=dr)
    _sweep_case("bga", 2, 3, 1, 203, 171, 2 * r, 2, 1e-5, seed=dr + 1)


@pytest.mark.parametrize("cx", [1, 3, 16])
@pytest.mark.parametrize("cy", [1, 5, 64])
def test_sweep_channels(cy, cx):
    _sweep_case("fast", 3, cy, cx, 45, 83, 4, 2, 1e-2, seed=cy + cx)


def test_sweep_window_of_one_pixel():
    _sweep_case("fast", 1, 5, 3, 33, 70, 1, 2, 1e-2)                      # r // s == 0
    _sweep_case("bga", 2, 2, 1, 33, 70, 2, 3, 1e-2)


def test_sweep_noncontiguous():
    _sweep_case("bga", 3, 5, 3, 61, 75, 4, 2, 1e-2, noncontiguous=True)


def test_sweep_large_image():
    _sweep_case("bga", 1, 8, 1, 1110, 1390, 20, 2, 1e-5)


def _inputs(shape_y, cx, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.rand(shape_y, device=DEV, generator=gen)
    x = torch.rand((shape_y[0], cx) + tuple(shape_y[2:]), device=DEV, generator=gen)
    g = torch.rand(shape_y, device=DEV, generator=gen) * 2 - 1
    return y, x, g


def test_need_combinations():
    import phl

    y, x, g = _inputs((2, 5, 37, 52), 3, 8)
    eps = torch.tensor([1e-2, 2e-2, 3e-2], device=DEV)
    kw = dict(subsample=2, scale=40.5, subtract_is_y=True)
    full = phl.guided_filter_grad(y, x, g, 4, eps, need_y=True, need_x=True, need_eps=True, **kw)
    assert all(t is not None and torch.isfinite(t).all() for t in full)
    for ny in (False, True):
        for nx in (False, True):
            for ne in (False, True):
                got = phl.guided_filter_grad(y, x, g, 4, eps, need_y=ny, need_x=nx, need_eps=ne, **kw)
                for want, asked, have in zip(full, (ny, nx, ne), got):
                    assert (have is None) if not asked else torch.equal(have, want), (ny, nx, ne)
    assert tuple(t.shape for t in full) == (y.shape, x.shape, (3,))


def test_deterministic():
    import phl

    y, x, g = _inputs((2, 7, 131, 257), 16, 4)
    kw = dict(subsample=2, scale=840.5, subtract_is_y=True, need_y=True, need_x=True, need_eps=True)
    a = phl.guided_filter_grad(y, x, g, 20, 1e-5, **kw)
    b = phl.guided_filter_grad(y, x, g, 20, 1e-5, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_function_honours_needs_input_grad():
    """GuidedFilterFn asks guided_filter_grad only for the gradients autograd needs, in one call, and saves y, x, eps."""
    import phl

    y, x, g = _inputs((1, 3, 30, 44), 2, 9)
    eps = torch.tensor([1e-2, 1e-2], device=DEV)
    seen = []
    real = phl.guided_filter_grad

    def f(*a, **k):
        seen.append((k["need_y"], k["need_x"], k["need_eps"]))
        return real(*a, **k)

    phl.guided_filter_grad = f
    try:
        for ny, nx, ne in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
            yy, xx, ee = y.clone().requires_grad_(ny), x.clone().requires_grad_(nx), eps.clone().requires_grad_(ne)
            out = phl.GuidedFilterFn.apply(yy, xx, ee, 4, 2, 1.0, False)
            assert len(out.grad_fn.saved_tensors) == 3
            (out * g).sum().backward()
            assert seen[-1] == (ny, nx, ne)
            assert (yy.grad is not None) == ny and (xx.grad is not None) == nx and (ee.grad is not None) == ne
    finally:
        phl.guided_filter_grad = real
    assert len(seen) == 4


def test_crfasrnn_trains_on_the_kernels():
    """CRFasRNN(fused_grad=True) with its default W: niters forward and niters backward kernel calls, no torch box sum; the
    gradients of logits, guide, gamma, s and omega against the float64 run, held to a factor 2 (see the header)."""
    from crf.crf_module import CRFasRNN, charb

    niters, L, H, W = 3, 16, 96, 128
    gen = torch.Generator(device=DEV).manual_seed(10)
    logits0 = torch.randn((1, L, H, W), device=DEV, generator=gen) * 2
    guide0 = torch.rand((1, 1, H, W), device=DEV, generator=gen)
    up = torch.rand((1, L, H, W), device=DEV, generator=gen) * 2 - 1

    def run(net, dtype):
        logits, guide = logits0.clone().to(dtype).requires_grad_(True), guide0.clone().to(dtype).requires_grad_(True)
        net.zero_grad(set_to_none=True)
        (net(guide, logits, labels=torch.arange(L, dtype=dtype, device=DEV)) * up.to(dtype)).sum().backward()
        return {"logits": logits.grad, "guide": guide.grad, "gamma": net.Mu.gamma.grad.clone(), "s": net.Mu.s.grad.clone(),
                "omega": net.W.omega.grad.clone()}

    net = CRFasRNN(charb(3.0), niters=niters, fused_grad=True).to(DEV)
    assert net.W.fused_grad
    with spy() as calls:
        hip = run(net, torch.float32)
    assert calls == {"hip": niters, "hip_grad": niters, "box_sum": 0}
    net.W.fused_grad = False
    with spy() as calls:
        t32 = run(net, torch.float32)
    assert calls["hip"] == 0 and calls["hip_grad"] == 0 and calls["box_sum"] > 0
    want = run(net.double(), torch.float64)
    for k in hip:
        _report(f"crfasrnn grad_{k}", hip[k], t32[k], want[k], factor=2)


def test_shapes_the_kernels_do_not_take_run_the_torch_form():
    """fused_grad=True with 17 guide channels, a bilinear upsampling or a Gaussian window: the torch form and its gradients."""
    from crf import guided

    y, x17, g = _inputs((1, 2, 30, 40), 17, 11)
    x1 = x17[:, :1].contiguous()
    cases = [(lambda f: guided.BatchedGuidedAdjacency(17, 2, 1e-2, fused_grad=f), x17, 1),
             (lambda f: guided.FastGuidedFilter(1, 4, 1e-2, mode="bilinear", fused_grad=f), x1, 0),
             (lambda f: guided.GuidedFilter(1, 2, 1e-2, gaussian=True, fused_grad=f), x1, 0)]
    for make, x, attempts in cases:
        res = []
        for flag in (True, False):
            torch.manual_seed(0)
            m = make(flag).to(DEV)
            with spy() as calls:
                res.append(_grads(m, y, x, g, torch.float32))
            assert calls["hip_grad"] == 0 and calls["hip"] == (attempts if flag else 0)
        for a, b in zip(*res):
            assert torch.equal(a, b)
