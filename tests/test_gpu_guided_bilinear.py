"""FastGuidedFilter / BatchedGuidedAdjacency with ``mode='bilinear', fused_bilinear=True`` on the HIP kernels
(phl.guided_filter_bilinear, phl_guided.hip: four-tap tile fill, k_guide_mean, k_guide_up).

Rule of every accuracy check, the one of tests/test_gpu_guided.py unchanged (through _guided_util.report): with g the
float64 result (the torch form in float64 on the device, or the reference's fixture), e_hip = max|hip - g| and e_torch =
max|fp32 torch form - g| over all elements, and e_hip <= e_torch with no margin.  Each case carries the precondition
e_torch >= 8 u, u = 2^-24 max|g|: where the fp32 torch form does not err, the rule judges nothing.  Every figure is
printed.  The whole loop (CRFasRNN) is held to the project's rule for loops: no further from the float64 plain loop than
twice the plain fp32 loop."""
import functools

import pytest
import torch

import _guided_util as util
from _guided_fixtures import BIL_CASES, build_module, load_case
from _guided_util import BILINEAR, BILINEAR_FULL, DEV, MIN_U, correlated_guide, report, route, spy, torch_form, torch_route

pytestmark = pytest.mark.gpu
module = functools.partial(util.module, variant=BILINEAR)
check = functools.partial(util.check_forward, BILINEAR)
check_full = functools.partial(util.check_forward, BILINEAR_FULL)

B, CY, EPS = 2, 3, 1e-2


def _max_r():
    import phl

    return phl.load_library().phl_guided_filter_max_r()


#         kind    cx  H    W    r     s
SWEEP = [("fast", 3, 41, 67, 4, 2),          # scales 2.05 and 2.03
         ("bga", 3, 70, 140, 9, 2),          # low resolution 35 x 70: up-sampling across all four tile edges
         ("bga", 1, 67, 131, 6, 3),
         ("fast", 3, 45, 75, 7, 4),
         ("bga", 16, 66, 130, 9, 2),         # 17 planes, low resolution 33 x 65
         ("bga", 3, 40, 50, 1, 2),           # re = 0
         ("bga", 3, 2, 131, 4, 2),           # low resolution 1 x 65
         ("bga", 1, 67, 3, 6, 3),            # 22 x 1
         ("bga", 3, 64, 128, 4, 2),          # exactly one tile
         ("bga", 1, 4, 1500, None, 2)]       # streamed: r = 2 (max_r + 1)
FULL = [("bga", 3, 70, 140, 9, 2), ("fast", 4, 41, 67, 4, 2), ("bga", 2, 67, 131, 6, 3)]


def _inputs(cx, H, W, seed, cy=CY):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand((B, cy, H, W), device=DEV, generator=gen), torch.rand((B, cx, H, W), device=DEV, generator=gen)


def _name(kind, cx, H, W, r, s, extra=""):
    return f"bilinear {extra}{kind} B{B} cy{CY} cx{cx} {H}x{W} r{r} s{s}"


@pytest.mark.parametrize("case", SWEEP, ids=[f"{c[0]}-cx{c[1]}-{c[2]}x{c[3]}-s{c[5]}" for c in SWEEP])
def test_sweep(case):
    kind, cx, H, W, r, s = case
    if r is None:
        r = 2 * (_max_r() + 1)
        assert min(r // s, max(H // s, W // s)) > _max_r()              # the streamed form of the window sums
    y, x = _inputs(cx, H, W, seed=H * W + cx)
    check(_name(kind, cx, H, W, r, s), module(kind, cx, r, s, EPS).to(DEV), y, x)


@pytest.mark.parametrize("case", FULL, ids=[f"{c[0]}-cx{c[1]}" for c in FULL])
def test_full_covariance(case):
    kind, cx, H, W, r, s = case
    y, x = _inputs(cx, H, W, seed=7 * H + cx)
    check_full(_name(kind, cx, H, W, r, s, "full "), module(kind, cx, r, s, EPS, full_cov=True).to(DEV), y, x)


def test_full_covariance_off_diagonal_terms_are_live():
    """On the correlated guide: max|full - diagonal| >= 1000 e_hip, the diagonal model on its own kernels (the check of
    test_gpu_guided_full.py)."""
    kind, cx, H, W, r, s = FULL[0]
    gen = torch.Generator(device=DEV).manual_seed(11)
    y = torch.rand((B, CY, H, W), device=DEV, generator=gen)
    x = correlated_guide(B, cx, H, W, gen, DEV)
    m = module(kind, cx, r, s, EPS, full_cov=True).to(DEV)
    check_full(_name(kind, cx, H, W, r, s, "full, correlated guide, "), m, y, x, off_diagonal=True)


@pytest.mark.parametrize("name", BIL_CASES)
def test_goldens(name):
    """The reference's own float64 output as the yardstick."""
    from crf import guided

    z = load_case(name)
    m = build_module(guided, z, torch.float32, DEV, "bilinear", fused_bilinear=True)
    y, x = torch.from_numpy(z["y"]).to(DEV), torch.from_numpy(z["x"]).to(DEV)
    with torch.no_grad(), spy() as calls:
        hip = m(y, x)
    assert calls == route(bilinear=1)
    with torch.no_grad(), torch_form():
        t32 = m(y, x)
    report(name, hip, t32, torch.from_numpy(z["out"]).to(DEV), min_torch_u=MIN_U)


def test_noncontiguous_out_view_and_determinism():
    import phl

    kind, cx, H, W, r, s = SWEEP[1]
    gen = torch.Generator(device=DEV).manual_seed(5)
    y = torch.rand((B, H, W, CY), device=DEV, generator=gen).permute(0, 3, 1, 2)
    x = torch.rand((B, cx, H, 2 * W), device=DEV, generator=gen)[..., ::2]
    assert not y.is_contiguous() and not x.is_contiguous()
    m = module(kind, cx, r, s, EPS).to(DEV)
    hip, _ = check(_name(kind, cx, H, W, r, s, "strided "), m, y, x)
    with torch.no_grad():
        assert torch.equal(m(y, x), hip)                                         # the same bits on every call
        assert torch.equal(m(y.contiguous(), x.contiguous()), hip)
        # out= as a view at the front of a buffer: nothing behind it is touched
        n, sentinel = hip.numel(), -12345.0
        buf = torch.full((n + 4096,), sentinel, device=DEV)
        out = buf[:n].view(hip.shape)
        got = phl.guided_filter_bilinear(y, x, r, m.eps, subsample=s, scale=0.5 * (2 * r + 1) ** 2, subtract=y, out=out)
        assert got is out and torch.equal(out, hip)
        assert bool((buf[n:] == sentinel).all())
        for full_cov in (False, True):
            a = phl.guided_filter_bilinear(y, x, r, m.eps, subsample=s, full_cov=full_cov)
            assert torch.equal(a, phl.guided_filter_bilinear(y, x, r, m.eps, subsample=s, full_cov=full_cov))


def test_subsample_one_is_the_nearest_route():
    import phl

    y, x = _inputs(3, 41, 67, seed=6)
    for full_cov in (False, True):
        m = module("bga", 3, 4, 1, EPS, full_cov=full_cov).to(DEV)
        with torch.no_grad(), spy() as calls:
            got = m(y, x)
        assert calls == route(nearest=1)
        with torch.no_grad():
            assert torch.equal(got, phl.guided_filter(y, x, 4, m.eps, scale=0.5 * 81, subtract=y, full_cov=full_cov))


def test_binding_shape_checks():
    import phl

    y, x = _inputs(1, 3, 67, seed=8)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear(y, x, 4, EPS, subsample=1)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear(y, x, 4, EPS, subsample=4)                    # 3 // 4 rows
    with pytest.raises(phl.PhlError) as e:
        phl.guided_filter_bilinear(y, torch.rand((B, 5, 3, 67), device=DEV), 4, EPS, subsample=2, full_cov=True)
    assert e.value.status == phl.ERR_UNSUPPORTED
    empty = phl.guided_filter_bilinear(y[:0], x[:0], 4, EPS, subsample=2)
    assert tuple(empty.shape) == (0, CY, 3, 67)


# ---- routing ------------------------------------------------------------------------------------------------------------
def test_routing():
    kind, cx, H, W, r, s = SWEEP[0]
    y, x = _inputs(cx, H, W, seed=9)
    flagged = module(kind, cx, r, s, EPS, fused_grad=True).to(DEV)
    plain = module(kind, cx, r, s, EPS, fused_bilinear=False).to(DEV)
    with torch.no_grad(), spy() as calls:
        flagged(y, x)
    assert calls == route(bilinear=1)
    with torch.no_grad(), spy() as calls:                                        # without the keyword: the torch form
        want = plain(y, x)
    assert calls == torch_route(calls)
    # while recording, fused_grad or not: the torch form, with the bits of the flag off
    yy = y.clone().requires_grad_(True)
    with spy() as calls:
        got = flagged(yy, x)
    assert calls == torch_route(calls)
    assert got.requires_grad and torch.equal(got.detach(), want)
    # float64 on the device: the torch form
    with torch.no_grad(), spy() as calls:
        got64 = flagged.double()(y.double(), x.double())
        want64 = plain.double()(y.double(), x.double())
    assert calls == torch_route(calls) and torch.equal(got64, want64)


def test_seventeen_guide_channels_take_the_torch_form():
    y, x = _inputs(17, 20, 30, seed=10)
    with torch.no_grad():
        with spy() as calls:
            got = module("bga", 17, 4, 2, EPS).to(DEV)(y, x)
        assert calls == route(bilinear=1, box_sum=calls["box_sum"]) and calls["box_sum"] > 0     # asked, PHL_ERR_UNSUPPORTED, torch form
        assert torch.equal(got, module("bga", 17, 4, 2, EPS, fused_bilinear=False).to(DEV)(y, x))


def test_crfasrnn_loop():
    from _nchw_util import old_loop, report_loop
    from crf.crf_module import CRFasRNN, charb

    g = torch.Generator(device=DEV).manual_seed(12)
    net = CRFasRNN(charb(.05), niters=3, r=8, gchannels=3, mode="bilinear", fused_bilinear=True).to(DEV)
    refs = torch.rand((1, 3, 96, 128), device=DEV, generator=g)
    logits = torch.randn((1, 16, 96, 128), device=DEV, generator=g) * 2
    labels = torch.arange(16, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        with spy() as calls:
            new = net(refs, logits, labels=labels)
        assert calls == route(bilinear=3)
        with old_loop(), torch_form(), spy() as calls:
            old = net(refs, logits, labels=labels)
        assert calls == torch_route(calls)
        with old_loop():
            want = net.double()(refs.double(), logits.double(), labels=labels.double())
        net.float()
    report_loop("CRFasRNN bilinear, 3 iterations", new, old, want)
