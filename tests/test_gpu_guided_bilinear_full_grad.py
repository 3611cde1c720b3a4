"""The backward of FastGuidedFilter / BatchedGuidedAdjacency with ``mode='bilinear'`` and ``full_cov=True`` on the HIP
kernels (phl.guided_filter_bilinear_full_grad, phl.GuidedFilterBilinearFullFn, the ``bilinear_full_grad`` keyword of the
classes; phl_guided.hip: backward<ST, CX, true>, CX >= 1).

Rule of every accuracy check, the one of tests/test_gpu_guided_bilinear_grad.py and tests/test_gpu_guided_full_grad.py
applied to each gradient (y, x, omega) through _guided_util.report: with g64 the float64 torch autograd gradient of the
mode on the device, e_hip = max|hip - g64| and e_torch = max|fp32 torch autograd of the mode - g64| over all elements, and
e_hip <= e_torch with no margin.  Each case carries the precondition e_torch >= 8 u, u = 2^-24 max|g64| (MIN_U of the
forward's tests): where fp32 torch autograd does not err, the rule judges nothing.  At a window of one pixel the exact x-
and omega-gradients are 0: for those two the rule is applied to the absolute errors without the precondition, as
test_gpu_guided_full_grad.py::test_sweep_window_of_one_pixel does.  The end-to-end CRFasRNN case is held to e_hip <= 2
e_torch, as test_gpu_guided_bilinear_grad.py::test_crfasrnn_trains_on_the_kernels and for its reason: the fp32
compatibility and softmax steps are common to both paths.  Every figure is printed."""
import functools

import pytest
import torch

import _guided_util as util
from _guided_util import ALL, BILINEAR_FULL, DEV, GUIDES, MIN_U, grad_inputs, grads, report, route, spy

pytestmark = pytest.mark.gpu
module = functools.partial(util.module, variant=BILINEAR_FULL)

B, CY, EPS = 2, 3, 1e-2


def bilinear_full_grad_case(*args, **kw):
    res = util.full_grad_case(*args, variant=BILINEAR_FULL, min_torch_u=MIN_U, **kw)
    print(f"{res['name']}: largest e_hip = {res['u']:.2f} u")
    return res


def _max_r():
    import phl

    return phl.load_library().phl_guided_filter_grad_max_r()


#         kind    cx  H    W    r     s
SWEEP = [("fast", 3, 41, 67, 4, 2),          # ratios 2.05 and 2.03
         ("bga", 3, 70, 140, 9, 2),          # low resolution 35 x 70: U^T and D^T across all four tile edges
         ("bga", 1, 67, 131, 6, 3),          # cx = 1 is the diagonal model
         ("fast", 3, 45, 75, 7, 4),          # half the full-resolution rows are nobody's tap
         ("bga", 4, 66, 130, 9, 2),          # the largest cx: 10 pair planes
         ("bga", 3, 2, 131, 4, 2),           # low resolution 1 x 65
         ("bga", 2, 67, 3, 6, 3),            # 22 x 1
         ("bga", 3, 64, 128, 4, 2),          # exactly one tile
         ("bga", 3, 5, 7, 2, 2),             # both clamped-edge taps on each axis
         ("bga", 2, 4, 1500, None, 2),       # streamed: r = 2 (max_r + 1)
         ("bga", 2, 40, 50, 1, 2)]           # re = 0: a window of one pixel


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("case", SWEEP, ids=[f"{c[0]}-cx{c[1]}-{c[2]}x{c[3]}-s{c[5]}" for c in SWEEP])
def test_sweep(case, guide):
    kind, cx, H, W, r, s = case
    if r is None:
        r = 2 * (_max_r() + 1)
        assert min(r // s, max(H // s, W // s)) > _max_r()              # the streamed form of the window sums
    absolute = ("x", "omega") if r // s == 0 else ()
    bilinear_full_grad_case(kind, B, CY, cx, H, W, r, s, EPS, guide, seed=H * W + cx, absolute=absolute)


def test_noncontiguous_and_determinism():
    kind, cx, H, W, r, s = SWEEP[1]
    util.check_noncontiguous_and_determinism(
        BILINEAR_FULL, bilinear_full_grad_case(kind, B, CY, cx, H, W, r, s, EPS, "correlated", seed=5, noncontiguous=True))


def test_need_combinations():
    import phl

    y, x, g = grad_inputs(2, 5, 3, 37, 52, "correlated", 8)
    eps = torch.tensor([1e-2, 2e-2, 3e-2], device=DEV)
    util.check_need_combinations(BILINEAR_FULL, y, x, g, eps)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear_full_grad(y, x, g, 4, eps, subsample=1)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear_full_grad(y, x, g, 4, eps, subsample=40)            # 37 // 40 rows
    y5, x5, g5 = grad_inputs(1, 2, 5, 30, 40, "uniform", 9)
    with pytest.raises(phl.PhlError) as err:
        phl.guided_filter_bilinear_full_grad(y5, x5, g5, 4, 1e-2, subsample=2)
    assert err.value.status == phl.ERR_UNSUPPORTED == 7


def test_function_honours_needs_input_grad():
    """GuidedFilterBilinearFullFn asks guided_filter_bilinear_full_grad only for the gradients autograd needs, in one call,
    and saves y, x, eps; its forward is phl.guided_filter_bilinear(full_cov=True) bit for bit."""
    import phl

    y, x, g = grad_inputs(1, 3, 2, 30, 44, "correlated", 9)
    eps = torch.tensor([1e-2, 2e-2], device=DEV)
    util.check_function_honours_needs_input_grad(BILINEAR_FULL, y, x, g, eps)
    out = phl.GuidedFilterBilinearFullFn.apply(y.clone().requires_grad_(True), x, eps, 4, 2, 40.5, True)
    assert torch.equal(out, phl.guided_filter_bilinear(y, x, 4, eps, subsample=2, scale=40.5, subtract=y, full_cov=True))


# ---- chunks -------------------------------------------------------------------------------------------------------------
CHUNK_B, CHUNK_CX, CHUNK_HW, CHUNK_R, CHUNK_S = 2, 4, 512, 8, 2


def _chunk_layout():
    """(cy, labels per chunk) of the chunk case: cy from the library's query at the low resolution, so that the first chunk
    boundary falls inside the first image and the chunk behind it holds labels of both images."""
    import phl

    lo = CHUNK_HW // CHUNK_S
    per = phl.guided_filter_labels_per_chunk(CHUNK_B, 4096, CHUNK_CX, lo, lo, full_cov=True, **ALL)   # (cy enters only as a cap)
    cy = per + 2
    assert phl.guided_filter_labels_per_chunk(CHUNK_B, cy, CHUNK_CX, lo, lo, full_cov=True, **ALL) == per
    print(f"{per} labels per chunk of {CHUNK_B} x {cy}")
    assert 2 <= per < cy and cy % per != 0
    chunks = [(n0, min(CHUNK_B * cy, n0 + per)) for n0 in range(0, CHUNK_B * cy, per)]
    assert chunks[0][1] < cy                                                    # a boundary inside the first image
    assert any(n0 // cy != (n1 - 1) // cy for n0, n1 in chunks), chunks         # labels of two images in one launch
    assert any(n0 % cy != 0 for n0, _ in chunks), chunks                        # a chunk that starts inside an image
    return cy, per


@functools.lru_cache(maxsize=None)
def _chunk_case():
    cy, per = _chunk_layout()
    return bilinear_full_grad_case("bga", CHUNK_B, cy, CHUNK_CX, CHUNK_HW, CHUNK_HW, CHUNK_R, CHUNK_S, EPS, "correlated", seed=3), cy, per


def test_chunks():
    """The rule for all three gradients (grad_x and grad_omega are summed over the chunks)."""
    res, _, _ = _chunk_case()
    print(f"{res['name']}: largest e_hip = {res['u']:.2f} u")


def test_chunks_labels_alone_and_determinism():
    """grad_y of the labels on either side of a chunk boundary, bit for bit, in a call of their own (one chunk); grad_x and
    grad_eps the same bits in two runs."""
    import phl

    res, cy, per = _chunk_case()
    lo = CHUNK_HW // CHUNK_S
    kw = dict(subsample=CHUNK_S, scale=0.5 * (2 * CHUNK_R + 1) ** 2, subtract_is_y=True)
    e = res["m"].eps.detach()
    for l0, l1 in ((max(0, per - 3), per), (per, min(cy, per + 3)), (max(0, per - 2), min(cy, per + 2))):
        ys, gs = res["y"][:, l0:l1].contiguous(), res["g"][:, l0:l1].contiguous()
        assert phl.guided_filter_labels_per_chunk(CHUNK_B, l1 - l0, CHUNK_CX, lo, lo, need_y=True, full_cov=True) == CHUNK_B * (l1 - l0)
        gy, _, _ = phl.guided_filter_bilinear_full_grad(ys, res["x"], gs, CHUNK_R, e, **kw)
        assert torch.equal(gy, res["hip"][0][:, l0:l1]), (l0, l1)
    a = phl.guided_filter_bilinear_full_grad(res["y"], res["x"], res["g"], CHUNK_R, e, **ALL, **kw)
    b = phl.guided_filter_bilinear_full_grad(res["y"], res["x"], res["g"], CHUNK_R, e, **ALL, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0], res["hip"][0]) and torch.equal(a[1], res["hip"][1])


# ---- routing ------------------------------------------------------------------------------------------------------------
def test_five_guide_channels_take_the_torch_form():
    y, x, g = grad_inputs(1, 2, 5, 30, 40, "correlated", 11)
    res = []
    for flag in (True, False):
        m = module("bga", 5, 4, 2, EPS, bilinear_full_grad=flag).to(DEV)
        with spy() as calls:
            res.append(grads(m, y, x, g, torch.float32))
        # (with the keyword the forward is tried once and declined with PHL_ERR_UNSUPPORTED before any launch)
        assert calls == route(bilinear=1 if flag else 0, box_sum=calls["box_sum"]) and calls["box_sum"] > 0, calls
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_float64_on_the_device_takes_the_torch_form():
    y, x, g = grad_inputs(1, 2, 3, 30, 40, "correlated", 12)
    res = []
    for flag in (True, False):
        m = module("fast", 3, 4, 2, EPS, bilinear_full_grad=flag).to(DEV).double()
        with spy() as calls:
            res.append(grads(m, y, x, g, torch.float64))
        assert calls == route(box_sum=calls["box_sum"]) and calls["box_sum"] > 0, calls
    for a, b in zip(*res):
        assert a.dtype == torch.float64 and torch.equal(a, b)


def test_subsample_one_is_the_nearest_full_pair():
    """At subsample 1 both interpolations are the identity: phl.GuidedFilterFullFn, with the bits of the nearest
    ``full_cov_grad`` module."""
    from crf import guided

    y, x, g = grad_inputs(2, 3, 3, 41, 67, "correlated", 6)
    m = module("bga", 3, 4, 1, EPS, bilinear_full_grad=True).to(DEV)
    with spy() as calls:
        got = grads(m, y, x, g, torch.float32)
    assert calls == route(nearest=1, nearest_full_grad=1), calls
    want = grads(guided.BatchedGuidedAdjacency(3, 4, EPS, subsample_ratio=1, full_cov=True, full_cov_grad=True).to(DEV), y, x, g,
                 torch.float32)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_keyword_off_leaves_every_route_as_it_was():
    """Without ``bilinear_full_grad``: the recorded forward of the full-covariance bilinear module is the torch form
    (``full_cov_grad`` / ``fused_grad`` or not), its unrecorded forward phl.guided_filter_bilinear; the diagonal
    ``bilinear_grad`` module and the nearest ``full_cov_grad`` module keep their kernels.  With it, an unrecorded forward
    is unchanged."""
    from crf import guided

    y, x, g = grad_inputs(1, 2, 3, 30, 40, "correlated", 13)
    for extra in ({}, {"full_cov_grad": True}, {"full_cov_grad": True, "fused_grad": True}):
        m = module("bga", 3, 4, 2, EPS, **extra).to(DEV)
        with spy() as calls:
            grads(m, y, x, g, torch.float32)
        assert calls == route(box_sum=calls["box_sum"]) and calls["box_sum"] > 0, (extra, calls)
    outs = []
    for flag in (False, True):
        m = module("bga", 3, 4, 2, EPS, bilinear_full_grad=flag).to(DEV)
        with spy() as calls, torch.no_grad():
            outs.append(m(y, x))
        assert calls == route(bilinear=1), (flag, calls)
    assert torch.equal(*outs)
    m = guided.BatchedGuidedAdjacency(3, 4, EPS, subsample_ratio=2, mode="bilinear", fused_bilinear=True, bilinear_grad=True).to(DEV)
    with spy() as calls:
        grads(m, y, x, g, torch.float32)
    assert calls == route(bilinear=1, bilinear_grad=1), calls
    m = guided.BatchedGuidedAdjacency(3, 4, EPS, subsample_ratio=2, full_cov=True, full_cov_grad=True).to(DEV)
    with spy() as calls:
        grads(m, y, x, g, torch.float32)
    assert calls == route(nearest=1, nearest_full_grad=1), calls


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_step", [False, True], ids=["plain_step", "fused_step"])
def test_crfasrnn_trains_on_the_kernels(fused_step):
    """CRFasRNN(mode='bilinear', fused_bilinear=True, full_cov=True, bilinear_full_grad=True): niters forward and niters
    backward kernel calls, no torch box sum; the gradients of logits, guide, gamma, s and omega against the float64 run,
    held to a factor 2 (see the header).  Once more with ``fused_step=True``: the two opt-ins compose."""
    from crf.crf_module import CRFasRNN, charb

    niters, L, H, W = 3, 16, 96, 128
    gen = torch.Generator(device=DEV).manual_seed(10)
    logits0 = torch.randn((1, L, H, W), device=DEV, generator=gen) * 2
    guide0 = torch.rand((1, 3, H, W), device=DEV, generator=gen)
    up = torch.rand((1, L, H, W), device=DEV, generator=gen) * 2 - 1

    def run(net, dtype):
        logits, guide = logits0.clone().to(dtype).requires_grad_(True), guide0.clone().to(dtype).requires_grad_(True)
        net.zero_grad(set_to_none=True)
        (net(guide, logits, labels=torch.arange(L, dtype=dtype, device=DEV)) * up.to(dtype)).sum().backward()
        return {"logits": logits.grad, "guide": guide.grad, "gamma": net.Mu.gamma.grad.clone(), "s": net.Mu.s.grad.clone(),
                "omega": net.W.omega.grad.clone()}

    net = CRFasRNN(charb(.05), niters=niters, r=8, gchannels=3, mode="bilinear", fused_bilinear=True, full_cov=True,
                   bilinear_full_grad=True, fused_step=fused_step).to(DEV)
    assert net.W.bilinear_full_grad
    with spy() as calls:
        hip = run(net, torch.float32)
    assert calls == route(bilinear=niters, bilinear_full_grad=niters), calls
    net.W.bilinear_full_grad = False
    net.fused_step = False
    with spy() as calls:
        t32 = run(net, torch.float32)
    assert calls == route(box_sum=calls["box_sum"]) and calls["box_sum"] > 0, calls
    want = run(net.double(), torch.float64)
    for k in hip:
        report(f"crfasrnn bilinear full grad_{k}", hip[k], t32[k], want[k], factor=2, what="grad")
