"""The backward of the full-covariance guided filter on the HIP kernels (phl.guided_filter_full_grad,
phl.GuidedFilterFullFn, the ``full_cov_grad`` keyword of the classes).

Rule of every accuracy check, the one of tests/test_gpu_guided_grad.py applied to each gradient (y, x, omega): with g64 the
float64 torch form's autograd gradient on the device, e_hip = max|hip - g64| and e_torch = max|fp32 torch autograd - g64|
over ALL elements, and e_hip <= e_torch with no margin.  Both are printed, also in u = 2^-24 max|g64|; no precondition in u
is asserted (the device's fp32 sums are not those of the CPU the shapes were chosen on).  On the correlated guide, with
more than one channel and a window of more than one pixel, each gradient must also differ from the diagonal kernels'
(phl.guided_filter_grad on the same inputs) by at least 1000 e_hip: a backward without the off-diagonal terms cannot pass.
The end-to-end CRFasRNN case is held to e_hip <= 2 e_torch: the fp32 compatibility and softmax steps are common to both
paths."""
import functools

import pytest
import torch

import _guided_util as util
from _guided_fixtures import load_case
from _guided_util import DEV, GUIDES, NEAREST_FULL, grad_inputs, grads, kernel_route, module, omega_grad, route, rule, spy, torch_route

pytestmark = pytest.mark.gpu
_case = functools.partial(util.full_grad_case, units=(True, True, True))
ROUTE = kernel_route(NEAREST_FULL)


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 4, 20, 100])
def test_sweep_radius_and_subsample(r, s, guide):
    # (r // s == 0, a window of one pixel: grad_x and grad_omega are rounding residue, see test_sweep_window_of_one_pixel)
    _case("gf" if s == 1 else "bga", 3, 5, 3, 61, 75, r, s, 1e-2, guide, seed=r + s, units=(True, r >= s, r >= s))


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("dr", [0, 1, 25])
def test_sweep_both_sides_of_the_tiled_radius(dr, guide):
    import phl

    r = phl.load_library().phl_guided_filter_grad_max_r() + dr
    _case("gf", 1, 2, 3, 203, 171, r, 1, 1e-2, guide, seed=dr)
    _case("bga", 2, 3, 4, 203, 171, 2 * r, 2, 1e-5, guide, seed=dr + 1)


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("cx", [1, 2, 3, 4])
@pytest.mark.parametrize("cy", [1, 5, 64])
def test_sweep_channels(cy, cx, guide):
    _case("fast", 3, cy, cx, 45, 83, 4, 2, 1e-2, guide, seed=cy + cx)


@pytest.mark.parametrize("guide", GUIDES)
def test_sweep_noncontiguous(guide):
    _case("bga", 3, 5, 3, 61, 75, 4, 2, 1e-2, guide, noncontiguous=True)


@pytest.mark.parametrize("guide", GUIDES)
def test_sweep_large_image(guide):
    _case("bga", 1, 8, 3, 1110, 1390, 20, 2, 1e-2, guide)


@pytest.mark.parametrize("guide", GUIDES)
def test_sweep_window_of_one_pixel(guide):
    """r // s == 0: cov and Sig vanish identically, so the exact x- and omega-gradients are 0 and float64 autograd itself
    returns ~1e-11.  The rule is applied to the absolute errors as it stands; u means nothing for those two."""
    _case("fast", 1, 5, 3, 33, 70, 1, 2, 1e-2, guide, units=(True, False, False))


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
def test_natural_image(eps):
    z = load_case("gf_tsukuba")
    kind = {"GuidedFilter": "gf", "FastGuidedFilter": "fast"}.get(str(z["kind"]), "bga")
    y, x = torch.from_numpy(z["y"]).to(DEV), torch.from_numpy(z["x"]).to(DEV)
    g = torch.rand(y.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) * 2 - 1
    m = module(kind, int(z["cx"]), int(z["r"]), int(z["s"]), eps, full_cov=True, full_cov_grad=True).to(DEV)
    util.check_grad(NEAREST_FULL, f"full grad tsukuba eps{eps:g}", m, y, x, g, units=(True, True, True))


def test_need_combinations():
    util.check_need_combinations(NEAREST_FULL, *grad_inputs(2, 5, 3, 37, 52, "correlated", 8),
                                 torch.tensor([1e-2, 2e-2, 3e-2], device=DEV))


def test_deterministic():
    util.check_deterministic(NEAREST_FULL, *grad_inputs(2, 7, 4, 131, 257, "correlated", 4))


def test_function_honours_needs_input_grad():
    """GuidedFilterFullFn asks guided_filter_full_grad only for the gradients autograd needs, in one call, and saves y, x,
    eps."""
    util.check_function_honours_needs_input_grad(NEAREST_FULL, *grad_inputs(1, 3, 2, 30, 44, "correlated", 9),
                                                 torch.tensor([1e-2, 1e-2], device=DEV))


def test_chunks():
    """Two chunks with the boundary inside the second image: the labels around it have the bits of a call of their own, and
    what is summed over the labels of both chunks (grad_x, grad_eps) holds the rule."""
    import phl

    B, cx, H, W, r = 2, 3, 256, 192, 8
    chunk = phl.guided_filter_labels_per_chunk(B, 64, cx, H, W, full=True, full_cov=True, need_y=True, need_x=True, need_eps=True)
    cy = chunk - 4
    assert cy >= 8 and cy < chunk < 2 * cy and chunk + 4 <= 2 * cy, (chunk, cy)          # the precondition
    assert phl.guided_filter_labels_per_chunk(B, cy, cx, H, W, full=True, full_cov=True, need_y=True, need_x=True,
                                              need_eps=True) == chunk
    y, x, g = grad_inputs(B, cy, cx, H, W, "correlated", 12)
    m = module("gf", cx, r, 1, 1e-2, full_cov=True).to(DEV)
    gy, gx, ge = phl.guided_filter_full_grad(y, x, g, r, m.eps, need_y=True, need_x=True, need_eps=True)
    lo = chunk - 4 - cy                                              # labels chunk - 4 .. chunk + 3 of the call: image 1
    own = phl.guided_filter_full_grad(y[1:, lo:lo + 8].contiguous(), x[1:], g[1:, lo:lo + 8].contiguous(), r, m.eps, need_y=True)[0]
    assert torch.equal(gy[1:, lo:lo + 8], own)
    t32 = grads(m, y, x, g, torch.float32)
    want = grads(m.double(), y, x, g, torch.float64)
    m.float()
    rule("chunks grad_x", gx, t32[1], want[1])
    rule("chunks grad_omega", omega_grad(ge, m.omega.detach()), t32[2], want[2])
    rule("chunks grad_y", gy, t32[0], want[0])


def test_routing():
    from crf import guided

    y, x, g = grad_inputs(1, 3, 3, 40, 50, "correlated", 6)
    m = guided.BatchedGuidedAdjacency(3, 4, 1e-2, full_cov=True, full_cov_grad=True).to(DEV)
    with spy() as calls:
        grads(m, y, x, g, torch.float32)
    assert calls == ROUTE
    with spy() as calls:                       # omega alone asks for a gradient: the same route
        (m(y, x) * g).sum().backward()
    assert calls == ROUTE
    with torch.no_grad(), spy() as calls:      # nothing recorded: the forward alone, as without the keyword
        m(y, x)
    assert calls == route(nearest=1)
    # fused_grad=True does not switch the route on
    m2 = guided.BatchedGuidedAdjacency(3, 4, 1e-2, full_cov=True, fused_grad=True).to(DEV)
    with spy() as calls:
        grads(m2, y, x, g, torch.float32)
    assert calls == torch_route(calls)


def test_five_guide_channels_run_the_torch_form():
    from crf import guided

    y, x, g = grad_inputs(1, 2, 5, 30, 40, "correlated", 11)
    res = []
    for flag in (True, False):
        m = guided.BatchedGuidedAdjacency(5, 2, 1e-2, full_cov=True, full_cov_grad=flag).to(DEV)
        with spy() as calls:
            res.append(grads(m, y, x, g, torch.float32))
        # (with the keyword the forward is tried once: the attempt that PHL_ERR_UNSUPPORTED ends)
        assert calls == route(nearest=1 if flag else 0, box_sum=calls["box_sum"]) and calls["box_sum"] > 0, calls
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_crfasrnn_trains_on_the_kernels():
    """CRFasRNN(full_cov=True, full_cov_grad=True): niters forward and niters backward kernel calls, no torch box sum; the
    gradients of logits, Mu (gamma, s) and omega against the float64 loop, held to a factor 2 (see the header)."""
    from crf.crf_module import CRFasRNN, charb

    z = load_case("crfasrnn_guided")
    gen = torch.Generator(device=DEV).manual_seed(8)
    x1 = torch.from_numpy(z["x"]).to(DEV)
    refs = torch.cat([x1, x1 + 0.1 * torch.rand(x1.shape, device=DEV, generator=gen),
                      x1 + 0.1 * torch.rand(x1.shape, device=DEV, generator=gen)], 1)
    logits0, labels = torch.from_numpy(z["logits"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV)
    up = torch.rand(logits0.shape, device=DEV, generator=gen) * 2 - 1
    niters = 3

    def run(net, dtype):
        logits = logits0.clone().to(dtype).requires_grad_(True)
        net.zero_grad(set_to_none=True)
        (net(refs.to(dtype), logits, labels=labels.to(dtype)) * up.to(dtype)).sum().backward()
        return {"logits": logits.grad, "gamma": net.Mu.gamma.grad.clone(), "s": net.Mu.s.grad.clone(),
                "omega": net.W.omega.grad.clone()}

    net = CRFasRNN(charb(3.), niters=niters, gchannels=3, full_cov=True, full_cov_grad=True).to(DEV)
    assert net.W.full_cov_grad
    with spy() as calls:
        hip = run(net, torch.float32)
    assert calls == kernel_route(NEAREST_FULL, niters)
    net.W.full_cov_grad = False
    with spy() as calls:
        t32 = run(net, torch.float32)
    assert calls == torch_route(calls)
    want = run(net.double(), torch.float64)
    for k in hip:
        rule(f"crfasrnn full_cov grad_{k}", hip[k], t32[k], want[k], factor=2)
