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
from _guided_fixtures import GRAD_CASES, fixture_grads, load_grad_case
from _guided_util import DEV, NEAREST, kernel_route, route, spy, torch_route
from _guided_util import grads as _grads
from _guided_util import sweep_case_grad as _sweep_case

pytestmark = pytest.mark.gpu
_report = functools.partial(util.report, what="grad")


@pytest.mark.parametrize("name", GRAD_CASES)
def test_goldens(name):
    from crf import guided

    z = load_grad_case(name)
    with spy() as calls:
        hip = fixture_grads(guided, z, torch.float32, DEV, fused_grad=True)
    assert calls == kernel_route(NEAREST)
    t32 = fixture_grads(guided, z, torch.float32, DEV)
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
    util.check_need_combinations(NEAREST, *_inputs((2, 5, 37, 52), 3, 8), torch.tensor([1e-2, 2e-2, 3e-2], device=DEV))


def test_deterministic():
    util.check_deterministic(NEAREST, *_inputs((2, 7, 131, 257), 16, 4))


def test_function_honours_needs_input_grad():
    """GuidedFilterFn asks guided_filter_grad only for the gradients autograd needs, in one call, and saves y, x, eps."""
    util.check_function_honours_needs_input_grad(NEAREST, *_inputs((1, 3, 30, 44), 2, 9), torch.tensor([1e-2, 1e-2], device=DEV))


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
    assert calls == kernel_route(NEAREST, niters)
    net.W.fused_grad = False
    with spy() as calls:
        t32 = run(net, torch.float32)
    assert calls == torch_route(calls)
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
            assert calls == route(nearest=attempts if flag else 0, box_sum=calls["box_sum"])
        for a, b in zip(*res):
            assert torch.equal(a, b)
