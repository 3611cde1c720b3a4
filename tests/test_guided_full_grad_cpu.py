"""The backward of the full-covariance guided filter without a GPU: the closed form that the kernels implement
(_guided_util.closed_form_grads) against float64 autograd through the torch form, the argument checks of
phl_guided_filter_full_grad and its chunk query (host code, before the first HIP call), and the ``full_cov_grad`` keyword
on tensors the kernels do not take.

Bound of the closed form: 1e-12 of each gradient's largest magnitude.  Both sides are float64 evaluations of the same
function through differently ordered sums; the largest gap over the 36 gradients where this was written was 7.4e-15
relative (grad_omega of FastGuidedFilter, cx 2)."""
import ctypes

import pytest
import torch

from _guided_util import closed_form_grads, correlated_guide, omega_grad

BOUND = 1e-12
EPS = (1e-2, 2e-2, 5e-3, 3e-2)


def _module(kind, cx, r, **kw):
    from crf import guided

    if kind == "gf":
        m = guided.GuidedFilter(cx, r, 1e-2, **kw)
    elif kind == "fast":
        m = guided.FastGuidedFilter(cx, r, 1e-2, subsample_ratio=2, **kw)
    else:
        m = guided.BatchedGuidedAdjacency(cx, r, 1e-2, subsample_ratio=2, **kw)
    with torch.no_grad():
        m.omega.copy_(torch.log(torch.expm1(torch.tensor(EPS[:cx]))))       # a distinct eps per channel
    return m


@pytest.mark.parametrize("cx", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["gf", "fast", "bga"])
def test_closed_form_is_float64_autograd(kind, cx):
    gen = torch.Generator().manual_seed(10 * cx + len(kind))
    r = 2 if kind == "gf" else 5
    y = torch.rand((2, 3, 13, 17), generator=gen, dtype=torch.float64).requires_grad_(True)
    x = correlated_guide(2, cx, 13, 17, gen, dtype=torch.float64).requires_grad_(True)
    g = torch.rand((2, 3, 13, 17), generator=gen, dtype=torch.float64) * 2 - 1
    m = _module(kind, cx, r, full_cov=True).double()
    (m(y, x) * g).sum().backward()
    s = 1 if kind == "gf" else 2
    scale = 0.5 * (2 * r + 1) ** 2 if kind == "bga" else 1.0
    with torch.no_grad():
        gy, gx, ge = closed_form_grads(y, x, g, r, m.eps, s, scale, kind == "bga")
        got = (gy, gx, omega_grad(ge, m.omega))
    for k, mine, want in zip(("y", "x", "omega"), got, (y.grad, x.grad, m.omega.grad)):
        mag, err = float(want.abs().max()), float((mine - want).abs().max())
        print(f"{kind} cx{cx} grad_{k}: max |closed form - autograd| = {err:.3e}, scale {mag:.4g}")
        assert mine.shape == want.shape and mag > 1e-3
        assert err <= BOUND * mag, (kind, cx, k, err)


def test_argument_checks_are_those_of_the_diagonal_backward():
    """Every bad set of tests/test_guided_grad_cpu.py gives the same status, under this entry point's name."""
    import phl
    from test_guided_grad_cpu import ARG_CASES, OK

    lib = phl.load_library()
    for args, status in ARG_CASES:
        a = list(args)
        a[19] = ctypes.c_float(a[19])
        assert lib.phl_guided_filter_full_grad(*a, None) == status, args
        if status != OK:
            assert lib.phl_last_error().decode().startswith("phl_guided_filter_full_grad:"), lib.phl_last_error()


def test_more_than_four_guide_channels_is_unsupported():
    import phl
    from test_guided_grad_cpu import _args

    lib = phl.load_library()
    for cx, status in ((4, None), (5, 7), (16, 7)):
        a = list(_args(cx=cx))
        a[19] = ctypes.c_float(a[19])
        if status is not None:
            assert lib.phl_guided_filter_full_grad(*a, None) == status
            assert lib.phl_last_error().decode().startswith("phl_guided_filter_full_grad:"), lib.phl_last_error()
    # the channel bound comes after the zero-element return and before the aliasing check, as in phl_guided_filter_full
    a = list(_args(cx=5, B=0, y=None, x=None, g=None))
    a[19] = ctypes.c_float(a[19])
    assert lib.phl_guided_filter_full_grad(*a, None) == 0
    a = list(_args(cx=5, gy=0x1000))
    a[19] = ctypes.c_float(a[19])
    assert lib.phl_guided_filter_full_grad(*a, None) == 7


def test_labels_per_chunk_by_hand():
    """Plan::per_backward with the full covariance's grad_planes(): bytes a label = hw * (4 unless full + 8 (cx + 1) + 8 cx for
    grad_x + 8 (npairs + 2 cx) for grad_x or grad_eps), within 96 MiB, at least one label and at most B * cy."""
    import phl

    budget = 96 << 20
    for B, cy, cx, h, w in ((2, 64, 3, 256, 192), (1, 64, 4, 555, 695), (1, 5, 1, 30, 40), (3, 7, 2, 1110, 1390)):
        hw, npairs = h * w, cx * (cx + 1) // 2
        for full in (False, True):
            for ny in (False, True):
                for nx in (False, True):
                    for ne in (False, True):
                        per = hw * ((0 if full else 4) + 8 * (cx + 1) + (8 * cx if nx else 0) + (8 * (npairs + 2 * cx) if nx or ne else 0))
                        want = max(1, min(B * cy, budget // per))
                        kw = dict(full=full, need_y=ny, need_x=nx, need_eps=ne, full_cov=True)
                        if ny or nx or ne:
                            assert phl.guided_filter_labels_per_chunk(B, cy, cx, h, w, **kw) == want, (B, cy, cx, h, w, kw)
                        assert phl.guided_filter_labels_per_chunk(B, cy, cx, h, w, grad=True, **kw) == want
    lib = phl.load_library()
    assert lib.phl_guided_filter_full_grad_labels_per_chunk(2, 64, 3, 256, 192, 1, 7) == (96 << 20) // (256 * 192 * (32 + 24 + 96))
    # the full model keeps more fp64 planes a label than the diagonal one from three channels on
    assert phl.guided_filter_labels_per_chunk(2, 64, 4, 256, 192, need_eps=True, full_cov=True) < \
        phl.guided_filter_labels_per_chunk(2, 64, 4, 256, 192, need_eps=True)
    # the forward's chunks do not depend on the model; bad sizes, more than four channels and other masks give 0
    assert phl.guided_filter_labels_per_chunk(2, 64, 3, 256, 192, full_cov=True) == phl.guided_filter_labels_per_chunk(2, 64, 3, 256, 192)
    for bad in ((0, 1, 1, 4, 4, 0, 1), (1, 1, 5, 4, 4, 0, 1), (1, 1, 1, 4, 4, 0, 8), (1, 1, 1, 4, 4, 0, -1), (1, 1, 1, 0, 4, 0, 1)):
        assert lib.phl_guided_filter_full_grad_labels_per_chunk(*bad) == 0, bad


def test_keyword_needs_the_full_model():
    from crf import guided
    from crf.crf_module import CRFasRNN, charb

    for make in (lambda **k: guided.GuidedFilter(3, 2, 1e-2, **k), lambda **k: guided.FastGuidedFilter(3, 2, 1e-2, **k),
                 lambda **k: guided.BatchedGuidedAdjacency(3, 2, 1e-2, **k)):
        with pytest.raises(ValueError):
            make(full_cov_grad=True)
        with pytest.raises(ValueError):
            make(full_cov_grad=True, fused_grad=True)
        assert make(full_cov=True, full_cov_grad=True).full_cov_grad is True
        assert make(full_cov=True).full_cov_grad is False and make().full_cov_grad is False
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), gchannels=3, full_cov_grad=True)


def test_keyword_reaches_the_w_of_crfasrnn_and_the_heads():
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler

    assert CRFasRNN(charb(3.0), gchannels=3, full_cov=True).W.full_cov_grad is False
    net = CRFasRNN(charb(3.0), gchannels=3, full_cov=True, full_cov_grad=True)
    assert net.W.full_cov and net.W.full_cov_grad and not net.W.fused_grad
    assert CRFdepthRefiner(full_cov=True).CRF.W.full_cov_grad is False
    assert CRFdepthRefiner(full_cov=True, full_cov_grad=True).CRF.W.full_cov_grad is True
    assert CRFdepthUpsampler(full_cov=True, full_cov_grad=True).CRF.W.full_cov_grad is True
    # the keyword adds no parameter or buffer
    assert list(CRFasRNN(charb(3.0), gchannels=3, full_cov=True, full_cov_grad=True).state_dict()) == \
        list(CRFasRNN(charb(3.0), gchannels=3, full_cov=True).state_dict())


@pytest.mark.parametrize("kind", ["gf", "fast", "bga"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_keyword_on_cpu_tensors_is_the_torch_form(kind, dtype):
    """full_cov_grad=True changes nothing for tensors the kernels do not take: the same bits as without it."""
    gen = torch.Generator().manual_seed(3)
    y0 = torch.rand((2, 3, 20, 26), generator=gen, dtype=dtype)
    x0 = correlated_guide(2, 3, 20, 26, gen, dtype=dtype)
    res = []
    for flag in (False, True):
        m = _module(kind, 3, 3, full_cov=True, full_cov_grad=flag).to(dtype)
        y, x = y0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        out = m(y, x)
        out.square().sum().backward()
        res.append((out.detach(), y.grad, x.grad, m.omega.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_binding_rejects_other_tensors():
    import phl

    t = torch.zeros(1, 1, 4, 4)
    with pytest.raises(TypeError):
        phl.guided_filter_full_grad(t, t, t, 1, 1e-2)
    with pytest.raises(TypeError):
        phl.guided_filter_full_grad(t.double(), t.double(), t.double(), 1, 1e-2)
