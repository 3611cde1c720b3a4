"""The backward of FastGuidedFilter / BatchedGuidedAdjacency with ``mode='bilinear'`` on the HIP kernels
(phl.guided_filter_bilinear_grad, phl.GuidedFilterBilinearFn, the ``bilinear_grad`` keyword of the classes; phl_guided.hip:
backward<ST, 0, true>).

Rule of every accuracy check, the one of tests/test_gpu_guided_grad.py applied to each gradient (y, x, omega) through
_guided_util.report: with g64 the float64 gradient (the torch form in float64 on the device, or the reference's fixture),
e_hip = max|hip - g64| and e_torch = max|fp32 torch autograd of the mode - g64| over all elements, and e_hip <= e_torch
with no margin.  Each case carries the precondition e_torch >= 8 u, u = 2^-24 max|g64| (MIN_U of the forward's tests):
where fp32 torch autograd does not err, the rule judges nothing.  The end-to-end CRFasRNN case is held to e_hip <= 2
e_torch, as test_gpu_guided_grad.py::test_crfasrnn_trains_on_the_kernels and for its reason: the fp32 compatibility and
softmax steps are common to both paths.  Every figure is printed."""
import functools

import pytest
import torch

import _guided_util as util
from _guided_fixtures import BIL_CASES, fixture_grads, load_grad_case
from _guided_util import ALL, BILINEAR, DEV, MIN_U, NEAREST, grads, kernel_route, report, route, spy, torch_route

pytestmark = pytest.mark.gpu
module = functools.partial(util.module, variant=BILINEAR)
sweep_case_grad = functools.partial(util.sweep_case_grad, variant=BILINEAR, min_torch_u=MIN_U)
ROUTE = kernel_route(BILINEAR)

B, CY, EPS = 2, 3, 1e-2


def _max_r():
    import phl

    return phl.load_library().phl_guided_filter_grad_max_r()


#         kind    cx  H    W    r     s
SWEEP = [("fast", 3, 41, 67, 4, 2),          # ratios 2.05 and 2.03
         ("bga", 3, 70, 140, 9, 2),          # low resolution 35 x 70: U^T and D^T across all four tile edges
         ("bga", 1, 67, 131, 6, 3),
         ("fast", 3, 45, 75, 7, 4),          # half the full-resolution rows are nobody's tap
         ("bga", 16, 66, 130, 9, 2),         # 17 planes
         ("bga", 3, 40, 50, 1, 2),           # re = 0: a window of one pixel
         ("bga", 3, 2, 131, 4, 2),           # low resolution 1 x 65
         ("bga", 1, 67, 3, 6, 3),            # 22 x 1
         ("bga", 3, 64, 128, 4, 2),          # exactly one tile
         ("bga", 3, 5, 7, 2, 2),             # both clamped-edge taps on each axis
         ("bga", 1, 4, 1500, None, 2)]       # streamed: r = 2 (max_r + 1)


@pytest.mark.parametrize("case", SWEEP, ids=[f"{c[0]}-cx{c[1]}-{c[2]}x{c[3]}-s{c[5]}" for c in SWEEP])
def test_sweep(case):
    kind, cx, H, W, r, s = case
    if r is None:
        r = 2 * (_max_r() + 1)
        assert min(r // s, max(H // s, W // s)) > _max_r()              # the streamed form of the window sums
    res = sweep_case_grad(kind, B, CY, cx, H, W, r, s, EPS, seed=H * W + cx)
    print(f"{res['name']}: largest e_hip = {res['u']:.2f} u")


@pytest.mark.parametrize("name", BIL_CASES)
def test_goldens(name):
    """The reference's own float64 gradients as the yardstick."""
    from crf import guided

    z = load_grad_case(name)
    with spy() as calls:
        hip = fixture_grads(guided, z, torch.float32, DEV, "bilinear", fused_bilinear=True, bilinear_grad=True)
    assert calls == ROUTE
    with spy() as calls:
        t32 = fixture_grads(guided, z, torch.float32, DEV, "bilinear", fused_bilinear=True)
    assert calls == torch_route(calls)
    for k, a, b in zip(("y", "x", "omega"), hip, t32):
        report(f"{name} grad_{k}", a, b, torch.from_numpy(z["grad_" + k]).to(DEV), what="grad", min_torch_u=MIN_U)


def test_noncontiguous_and_determinism():
    kind, cx, H, W, r, s = SWEEP[1]
    util.check_noncontiguous_and_determinism(BILINEAR, sweep_case_grad(kind, B, CY, cx, H, W, r, s, EPS, seed=5, noncontiguous=True))


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
    util.check_need_combinations(BILINEAR, y, x, g, eps)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear_grad(y, x, g, 4, eps, subsample=1)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear_grad(y, x, g, 4, eps, subsample=40)            # 37 // 40 rows


def test_function_honours_needs_input_grad():
    """GuidedFilterBilinearFn asks guided_filter_bilinear_grad only for the gradients autograd needs, in one call, and
    saves y, x, eps."""
    util.check_function_honours_needs_input_grad(BILINEAR, *_inputs((1, 3, 30, 44), 2, 9), torch.tensor([1e-2, 1e-2], device=DEV))


# ---- chunks -------------------------------------------------------------------------------------------------------------
CHUNK_B, CHUNK_CX, CHUNK_HW, CHUNK_R, CHUNK_S = 2, 16, 256, 8, 2


def _chunk_layout():
    """(cy, labels per chunk) of the chunk case: cy from the library's query, so that the first chunk boundary falls inside
    the first image and the chunk behind it holds labels of both images."""
    import phl

    lo = CHUNK_HW // CHUNK_S
    per = phl.guided_filter_labels_per_chunk(CHUNK_B, 4096, CHUNK_CX, lo, lo, **ALL)      # (cy enters only as a cap)
    cy = per + 2
    assert phl.guided_filter_labels_per_chunk(CHUNK_B, cy, CHUNK_CX, lo, lo, **ALL) == per
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
    return sweep_case_grad("bga", CHUNK_B, cy, CHUNK_CX, CHUNK_HW, CHUNK_HW, CHUNK_R, CHUNK_S, EPS, seed=3), cy, per


def test_chunks():
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
        assert phl.guided_filter_labels_per_chunk(CHUNK_B, l1 - l0, CHUNK_CX, lo, lo, need_y=True) == CHUNK_B * (l1 - l0)
        gy, _, _ = phl.guided_filter_bilinear_grad(ys, res["x"], gs, CHUNK_R, e, **kw)
        assert torch.equal(gy, res["hip"][0][:, l0:l1]), (l0, l1)
    a = phl.guided_filter_bilinear_grad(res["y"], res["x"], res["g"], CHUNK_R, e, **ALL, **kw)
    b = phl.guided_filter_bilinear_grad(res["y"], res["x"], res["g"], CHUNK_R, e, **ALL, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0], res["hip"][0]) and torch.equal(a[1], res["hip"][1])


# ---- what the kernels do not take -------------------------------------------------------------------------------------
def test_seventeen_guide_channels_take_the_torch_form():
    y, x, g = _inputs((1, 2, 30, 40), 17, 11)
    res = []
    for flag in (True, False):
        m = module("bga", 17, 4, 2, EPS, fused_bilinear=True, bilinear_grad=flag).to(DEV)
        with spy() as calls:
            res.append(grads(m, y, x, g, torch.float32))
        assert calls == route(bilinear=1 if flag else 0, box_sum=calls["box_sum"]) and calls["box_sum"] > 0, calls
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_float64_on_the_device_takes_the_torch_form():
    y, x, g = _inputs((1, 2, 30, 40), 3, 12)
    res = []
    for flag in (True, False):
        m = module("fast", 3, 4, 2, EPS, fused_bilinear=True, bilinear_grad=flag).to(DEV).double()
        with spy() as calls:
            res.append(grads(m, y, x, g, torch.float64))
        assert calls == torch_route(calls), calls
    for a, b in zip(*res):
        assert a.dtype == torch.float64 and torch.equal(a, b)


def test_subsample_one_is_the_nearest_pair():
    """At subsample 1 both interpolations are the identity: phl.GuidedFilterFn, with the bits of the nearest
    ``fused_grad`` module."""
    from crf import guided

    y, x, g = _inputs((2, 3, 41, 67), 3, 6)
    m = module("bga", 3, 4, 1, EPS, fused_bilinear=True, bilinear_grad=True).to(DEV)
    with spy() as calls:
        got = grads(m, y, x, g, torch.float32)
    assert calls == kernel_route(NEAREST)
    want = grads(guided.BatchedGuidedAdjacency(3, 4, EPS, subsample_ratio=1, fused_grad=True).to(DEV), y, x, g, torch.float32)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_step", [False, True], ids=["plain_step", "fused_step"])
def test_crfasrnn_trains_on_the_kernels(fused_step):
    """CRFasRNN(mode='bilinear', fused_bilinear=True, bilinear_grad=True): niters forward and niters backward kernel calls,
    no torch box sum; the gradients of logits, guide, gamma, s and omega against the float64 run, held to a factor 2 (see
    the header).  Once more with ``fused_step=True``: the two opt-ins compose."""
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

    net = CRFasRNN(charb(.05), niters=niters, r=8, gchannels=3, mode="bilinear", fused_bilinear=True, bilinear_grad=True,
                   fused_step=fused_step).to(DEV)
    assert net.W.bilinear_grad
    with spy() as calls:
        hip = run(net, torch.float32)
    assert calls == kernel_route(BILINEAR, niters)
    net.W.bilinear_grad = False
    net.fused_step = False
    with spy() as calls:
        t32 = run(net, torch.float32)
    assert calls == torch_route(calls)
    want = run(net.double(), torch.float64)
    for k in hip:
        report(f"crfasrnn bilinear grad_{k}", hip[k], t32[k], want[k], factor=2, what="grad")
