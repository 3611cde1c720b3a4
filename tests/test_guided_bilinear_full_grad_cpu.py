"""The backward of the bilinear full-covariance guided filter without a GPU: the ``bilinear_full_grad`` keyword of the
classes, of CRFasRNN and of the heads; the closed form that the kernels implement
(_guided_util.closed_form_grads with ``mode='bilinear'``) against float64 autograd through the torch form of
``mode='bilinear', full_cov=True``; the argument checks of phl_guided_filter_bilinear_full_grad, which return before the
first HIP call; the ABI row; and the chunk query that answers for the call.

Bound of the closed form: BOUND of tests/test_guided_full_grad_cpu.py (1e-12 of each gradient's largest magnitude), which
holds the same comparison for the nearest form: both sides are float64 evaluations of one function through differently
ordered sums.  The largest gap over the 81 gradients where this was written was 2.4e-14 relative (grad_y at the one-pixel
window)."""
import ctypes

import pytest
import torch

from _guided_util import closed_form_grads, correlated_guide, omega_grad
from test_guided_full_grad_cpu import BOUND, EPS

KW = dict(mode="bilinear", fused_bilinear=True, full_cov=True)


# ---- the keyword ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["FastGuidedFilter", "BatchedGuidedAdjacency"])
def test_keyword_of_the_filter_classes(cls):
    from crf import guided

    make = getattr(guided, cls)
    assert make(3, 4, 1e-2).bilinear_full_grad is False
    assert make(3, 4, 1e-2, **KW).bilinear_full_grad is False
    m = make(3, 4, 1e-2, bilinear_full_grad=True, **KW)
    assert m.bilinear_full_grad is True and m.bilinear_grad is False and m.full_cov_grad is False and m.fused_grad is False
    with pytest.raises(ValueError):
        make(3, 4, 1e-2, mode="bilinear", fused_bilinear=True, bilinear_full_grad=True)              # no full_cov
    with pytest.raises(ValueError):
        make(3, 4, 1e-2, mode="bilinear", full_cov=True, bilinear_full_grad=True)                    # no fused_bilinear
    with pytest.raises(ValueError):
        make(3, 4, 1e-2, full_cov=True, full_cov_grad=True, fused_grad=True, bilinear_full_grad=True)   # ... are not enough
    with pytest.raises(ValueError):
        make(3, 4, 1e-2, bilinear_full_grad=True)
    with pytest.raises(NotImplementedError):                                                         # unchanged
        make(3, 4, 1e-2, bilinear_grad=True, **KW)
    with pytest.raises(NotImplementedError):
        make(3, 4, 1e-2, bilinear_grad=True, bilinear_full_grad=True, **KW)
    with pytest.raises(TypeError):
        make(3, 4, 1e-2, 2, "bilinear", True, False, True)      # keyword-only


def test_keyword_reaches_the_w_of_crfasrnn_and_the_heads():
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    kw = dict(bilinear_full_grad=True, **KW)
    assert CRFasRNN(charb(3.0)).W.bilinear_full_grad is False
    assert CRFasRNN(charb(3.0), gchannels=3, **KW).W.bilinear_full_grad is False
    net = CRFasRNN(charb(3.0), gchannels=3, **kw)
    assert net.W.bilinear_full_grad and net.W.full_cov and net.W.fused_bilinear and not net.W.full_cov_grad and not net.W.fused_grad
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), gchannels=3, mode="bilinear", fused_bilinear=True, bilinear_full_grad=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), gchannels=3, mode="bilinear", full_cov=True, bilinear_full_grad=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), gchannels=3, full_cov=True, full_cov_grad=True, bilinear_full_grad=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), lattice=True, bilinear_full_grad=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), lattice=True, **kw)
    with pytest.raises(NotImplementedError):
        CRFasRNN(charb(3.0), gchannels=3, bilinear_grad=True, **KW)
    with pytest.raises(TypeError):
        CRFasRNN(charb(3.0), 5, 20, 1e-5, False, False, 3, False, False, False, True, False, "bilinear", True, False, True)
    for head in (CRFdepthRefiner, CRFwUncertainty, CRFdepthUpsampler):
        assert head().CRF.W.bilinear_full_grad is False
        assert head(**KW).CRF.W.bilinear_full_grad is False
        assert head(**kw).CRF.W.bilinear_full_grad is True
        with pytest.raises(ValueError):
            head(mode="bilinear", fused_bilinear=True, bilinear_full_grad=True)
        with pytest.raises(ValueError):
            head(mode="bilinear", full_cov=True, bilinear_full_grad=True)
        with pytest.raises(NotImplementedError):
            head(bilinear_grad=True, **KW)
    # the keyword adds no parameter or buffer
    assert list(CRFasRNN(charb(3.0), gchannels=3, **kw).state_dict()) == list(CRFasRNN(charb(3.0), gchannels=3, **KW).state_dict())


@pytest.mark.parametrize("kind", ["fast", "bga"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_keyword_on_cpu_tensors_is_the_torch_form(kind, dtype):
    """bilinear_full_grad=True changes nothing for tensors the kernels do not take: the same bits as with the keyword off."""
    from crf import guided

    gen = torch.Generator().manual_seed(3)
    y0 = torch.rand((2, 3, 20, 26), generator=gen, dtype=dtype)
    x0 = correlated_guide(2, 3, 20, 26, gen, dtype=dtype)
    cls = guided.FastGuidedFilter if kind == "fast" else guided.BatchedGuidedAdjacency
    res = []
    for flag in (False, True):
        m = cls(3, 3, 1e-2, subsample_ratio=2, bilinear_full_grad=flag, **KW).to(dtype)
        y, x = y0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        out = m(y, x)
        out.square().sum().backward()
        res.append((out.detach(), y.grad, x.grad, m.omega.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- the closed form --------------------------------------------------------------------------------------------------
def _closed_form_case(kind, cx, H, W, r, s, seed):
    from crf import guided

    gen = torch.Generator().manual_seed(seed)
    y = torch.rand((2, 3, H, W), generator=gen, dtype=torch.float64).requires_grad_(True)
    x = correlated_guide(2, cx, H, W, gen, dtype=torch.float64).requires_grad_(True)
    g = torch.rand((2, 3, H, W), generator=gen, dtype=torch.float64) * 2 - 1
    cls = guided.FastGuidedFilter if kind == "fast" else guided.BatchedGuidedAdjacency
    m = cls(cx, r, 1e-2, subsample_ratio=s, mode="bilinear", full_cov=True)
    with torch.no_grad():
        m.omega.copy_(torch.log(torch.expm1(torch.tensor(EPS[:cx]))))       # a distinct eps per channel
    m = m.double()
    (m(y, x) * g).sum().backward()
    scale = 0.5 * (2 * r + 1) ** 2 if kind == "bga" else 1.0
    with torch.no_grad():
        gy, gx, ge = closed_form_grads(y, x, g, r, m.eps, s, scale, kind == "bga", "bilinear")
        got = (gy, gx, omega_grad(ge, m.omega))
    name = f"{kind} cx{cx} {H}x{W} r{r} s{s}"
    mag_y = float(y.grad.abs().max())
    for k, mine, want in zip(("y", "x", "omega"), got, (y.grad, x.grad, m.omega.grad)):
        mag, err = float(want.abs().max()), float((mine - want).abs().max())
        print(f"{name} grad_{k}: max |closed form - autograd| = {err:.3e}, scale {mag:.4g}")
        assert mine.shape == want.shape
        if r // s == 0 and k != "y":
            # a window of one pixel: cov and Sig vanish identically, so the exact x- and omega-gradients are 0 and both
            # sides hold what is left of cancelled terms of grad_y's size: the bound is taken of that size (the sum over
            # all pixels, for omega)
            assert mag <= BOUND * mag_y * y.numel(), (name, k, mag)
            mag = mag_y * (y.numel() if k == "omega" else 1)
        assert mag > 1e-3, (name, k, mag)
        assert err <= BOUND * mag, (name, k, err)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("cx", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["fast", "bga"])
def test_closed_form_is_float64_autograd(kind, cx, s):
    _closed_form_case(kind, cx, 13, 17, 3 * s, s, 10 * cx + s + len(kind))


@pytest.mark.parametrize("kind,cx,H,W,r,s", [("bga", 2, 12, 14, 1, 2),       # a window of one pixel
                                             ("bga", 3, 2, 17, 4, 2),        # a 2 x W image: low resolution 1 x 8
                                             ("fast", 2, 13, 3, 6, 3)],      # an H x 3 image: 4 x 1
                         ids=["one_pixel_window", "two_rows", "three_columns"])
def test_closed_form_at_the_edge_shapes(kind, cx, H, W, r, s):
    _closed_form_case(kind, cx, H, W, r, s, H * W + cx)


# ---- the C entry point ------------------------------------------------------------------------------------------------
OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
Y, X, G, GY, GX, GE, E = (0x1000 * k for k in range(1, 8))     # fake device addresses, never dereferenced
NAME = "phl_guided_filter_bilinear_full_grad"


def _args(y=Y, x=X, g=G, gy=GY, gx=GX, ge=GE, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, eps=E, scale=1.0, sub=1):
    return (y, x, g, gy, gx, ge, B, cy, cx, H, W, h, w, r, eps, scale, sub)


ARG_CASES = [
    (_args(y=None), INVALID), (_args(x=None), INVALID), (_args(g=None), INVALID), (_args(eps=None), INVALID),
    (_args(B=-1), INVALID), (_args(cy=-1), INVALID), (_args(cx=0), INVALID), (_args(H=-3), INVALID), (_args(h=0), INVALID),
    (_args(w=0), INVALID), (_args(r=-1), INVALID), (_args(h=49), INVALID), (_args(scale=float("nan")), INVALID),
    (_args(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE),
    (_args(cx=17), UNSUPPORTED), (_args(cx=5), UNSUPPORTED), (_args(cx=16), UNSUPPORTED),
    (_args(h=25), UNSUPPORTED), (_args(w=33), UNSUPPORTED), (_args(H=3, h=2), UNSUPPORTED),
    (_args(gy=Y), INVALID), (_args(gy=G), INVALID), (_args(gx=X), INVALID), (_args(ge=E), INVALID), (_args(gx=GY), INVALID),
    (_args(ge=GX), INVALID),
    (_args(B=0, y=None, x=None, g=None), OK), (_args(cy=0, y=None, g=None), OK), (_args(H=0, h=0, y=None, g=None), OK),
    (_args(B=0, cx=5, y=None, x=None, g=None), OK),                  # zero elements: before the channel bound
    (_args(gy=None, gx=None, ge=None), OK), (_args(gy=None, gx=None, ge=None, cx=5, h=25), OK),   # nothing asked for: nothing launched
    (_args(cx=5, h=25, gy=Y), UNSUPPORTED),                          # the order: channels, then sizes, then aliasing
    (_args(h=25, gy=Y), UNSUPPORTED), (_args(cx=5, gy=Y), UNSUPPORTED),
    (_args(g=None, cx=5), INVALID),                                  # the shared checks come first
]


@pytest.mark.parametrize("args,status", ARG_CASES, ids=[str(i) for i in range(len(ARG_CASES))])
def test_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    a = list(args)
    a[15] = ctypes.c_float(a[15])
    assert getattr(lib, NAME)(*a, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith(NAME + ":"), lib.phl_last_error()


def test_order_of_the_unsupported_checks():
    """cx = 5 with h = 25: the message is the channel bound's, not the size's."""
    import phl

    lib = phl.load_library()
    a = list(_args(cx=5, h=25, gy=Y))
    a[15] = ctypes.c_float(a[15])
    assert getattr(lib, NAME)(*a, None) == UNSUPPORTED
    assert "guide channels" in lib.phl_last_error().decode(), lib.phl_last_error()
    a = list(_args(h=25, gy=Y))
    a[15] = ctypes.c_float(a[15])
    assert getattr(lib, NAME)(*a, None) == UNSUPPORTED
    assert "more than half" in lib.phl_last_error().decode(), lib.phl_last_error()


def test_abi_row():
    import phl

    row = [r for r in phl._ABI if r[0] == NAME]
    assert row == [(NAME, "i", "PPPPPPiiiiiiiiPfiS")]
    names = [r[0] for r in phl._ABI]
    assert names.index(NAME) == names.index("phl_guided_filter_bilinear_grad") + 1


@pytest.mark.parametrize("needs", range(1, 8))
def test_chunk_query_is_the_nearest_full_backward_below_full_resolution(needs):
    """Labels per chunk of the call (phl.h: phl_guided_filter_full_grad_labels_per_chunk with full = 0), worked by hand: a
    label holds, at h x w, ys (4 bytes), Pd and Q (8 (cx + 1)), for grad_x A and mA (8 cx), for grad_x or grad_eps
    npairs + 2 cx fp64 planes; 96 MiB a chunk, at least one label, at most B cy."""
    import phl

    need_y, need_x, need_eps = bool(needs & 1), bool(needs & 2), bool(needs & 4)
    lib = phl.load_library()
    for B, cy, cx, h, w in ((2, 64, 3, 256, 192), (1, 64, 4, 555, 695), (2, 3, 2, 20, 33), (1, 70000, 1, 2, 2)):
        npairs = cx * (cx + 1) // 2
        per = h * w * (4 + 8 * (cx + 1) + (8 * cx if need_x else 0) + (8 * (npairs + 2 * cx) if need_x or need_eps else 0))
        want = max(1, min(B * cy, 65535, (96 << 20) // per))
        got = phl.guided_filter_labels_per_chunk(B, cy, cx, h, w, full_cov=True, need_y=need_y, need_x=need_x, need_eps=need_eps)
        assert got == want, (B, cy, cx, h, w, needs)
        assert lib.phl_guided_filter_full_grad_labels_per_chunk(B, cy, cx, h, w, 0, needs) == want


def test_header_states_the_chunk_query():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "phl.h")).read().replace("*", " ").split())
    decl = text.index("int phl_guided_filter_bilinear_full_grad(")
    assert text.index("int phl_guided_filter_bilinear_grad(") < decl
    comment = text[text.index("int phl_guided_filter_bilinear_grad("):decl]
    assert "phl_guided_filter_full_grad_labels_per_chunk(B, cy, cx, h, w, 0, needs) gives the labels per chunk of this call too" \
        in comment


def test_binding_rejects_other_arguments():
    import phl

    t = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear_full_grad(t, t, t, 1, 1e-2, subsample=1)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear_full_grad(t, t, t, 1, 1e-2, subsample=2)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear_full_grad(t.double(), t.double(), t.double(), 1, 1e-2, subsample=2)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear_full_grad(t, t, t, 1, 1e-2)              # subsample is required
    assert phl.GuidedFilterBilinearFullFn.__mro__[1] is torch.autograd.Function
