"""The backward of the box-window guided filter without a GPU: the float64 autograd gradients of the repository's torch
form (crf/guided.py) against the reference's (tests/golden/guided_grad_*.npz, written by
tests/golden/generate_guided_grad.py), the argument checks of phl_guided_filter_grad, which return before the first HIP
call, and the ``fused_grad`` keyword on tensors the kernels do not take.

Bound of the fixture check: 1e-12 of each gradient's largest magnitude, as tests/test_guided_cpu.py holds for the
forward.  Where the fixtures were written the largest gap was 8.2e-14 (grad_y of fast_r1_s2), 1.4e-14 elsewhere.  One
gradient has no magnitude of its own: fast_r1_s2 solves with r // s = 0, a window of one pixel, where cov = y x - y x and
var = x^2 - x^2 vanish identically, so A = 0 and the exact gradient with respect to x is 0.  Both float64 runs leave
rounding residue there (the reference's box sum and the repository's prefix sums round differently), so that gradient
is held, on both sides, to 1e-12 of the magnitude it would have without the cancellation, |g| |y| / eps."""
import ctypes

import numpy as np
import pytest
import torch

from _guided_fixtures import GRAD_CASES, fixture_grads, load_grad_case

BOUND = 1e-12


@pytest.mark.parametrize("name", GRAD_CASES)
def test_torch_form_gradients_match_reference_float64(name):
    from crf import guided

    z = load_grad_case(name)
    got = fixture_grads(guided, z, torch.float64, "cpu")
    for k, mine in zip(("y", "x", "omega"), got):
        want = z["grad_" + k]
        mag = float(np.abs(want).max())
        if name == "fast_r1_s2" and k == "x":           # exactly 0 in exact arithmetic: see the header
            mag = float(np.abs(z["g"]).max() * np.abs(z["y"]).max() / float(z["eps"]))
            assert np.abs(want).max() <= BOUND * mag
        err = float(np.abs(mine.numpy() - want).max())
        print(f"{name} grad_{k}: max |torch float64 - reference float64| = {err:.3e}, scale {mag:.4g}")
        assert mine.shape == want.shape
        assert err <= BOUND * mag, (name, k, err)


OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
Y, X, G, GY, GX, GE, M1, M2, M3, M4, E = (0x1000 * k for k in range(1, 12))     # fake device addresses, never dereferenced


def _args(y=Y, x=X, g=G, gy=GY, gx=GX, ge=GE, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, m1=M1, m2=M2, m3=M3, m4=M4, eps=E,
          scale=1.0, sub=1):
    return (y, x, g, gy, gx, ge, B, cy, cx, H, W, h, w, r, m1, m2, m3, m4, eps, scale, sub)


ARG_CASES = [
    (_args(B=-1), INVALID), (_args(cy=-1), INVALID), (_args(cx=0), INVALID), (_args(H=-3), INVALID), (_args(r=-1), INVALID),
    (_args(h=49), INVALID), (_args(w=65), INVALID), (_args(h=0), INVALID), (_args(scale=float("inf")), INVALID),
    (_args(y=None), INVALID), (_args(x=None), INVALID), (_args(g=None), INVALID), (_args(eps=None), INVALID),
    (_args(m1=None), INVALID), (_args(m4=None), INVALID), (_args(gy=Y), INVALID), (_args(gy=G), INVALID), (_args(gx=X), INVALID),
    (_args(ge=E), INVALID), (_args(gx=GY), INVALID),
    (_args(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE), (_args(B=1 << 20, cy=1 << 20), TOO_LARGE),
    (_args(H=(1 << 30) + 1, W=1, h=8, w=1), TOO_LARGE), (_args(cx=17), UNSUPPORTED),
    (_args(B=0, y=None, x=None, g=None), OK), (_args(cy=0, y=None, g=None), OK), (_args(H=0, h=0, y=None, g=None), OK),
    (_args(gy=None, gx=None, ge=None), OK),            # nothing asked for: nothing launched
]


@pytest.mark.parametrize("args,status", ARG_CASES, ids=[str(i) for i in range(len(ARG_CASES))])
def test_guided_filter_grad_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    a = list(args)
    a[19] = ctypes.c_float(a[19])
    assert lib.phl_guided_filter_grad(*a, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_guided_filter_grad"), lib.phl_last_error()


def test_tiled_backward_takes_the_default_radius():
    import phl

    assert phl.load_library().phl_guided_filter_grad_max_r() >= 20


@pytest.mark.parametrize("kind", ["gf", "fast", "bga"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fused_grad_on_cpu_tensors_is_the_torch_form(kind, dtype):
    """fused_grad=True changes nothing for tensors the kernels do not take: the same bits as fused_grad=False."""
    from crf import guided

    gen = torch.Generator().manual_seed(3)
    y0 = torch.rand((2, 3, 20, 26), generator=gen, dtype=dtype)
    x0 = torch.rand((2, 2, 20, 26), generator=gen, dtype=dtype)
    res = []
    for flag in (False, True):
        if kind == "gf":
            m = guided.GuidedFilter(2, 3, 1e-2, fused_grad=flag)
        elif kind == "fast":
            m = guided.FastGuidedFilter(2, 3, 1e-2, subsample_ratio=2, fused_grad=flag)
        else:
            m = guided.BatchedGuidedAdjacency(2, 3, 1e-2, subsample_ratio=2, fused_grad=flag)
        m = m.to(dtype)
        assert m.fused_grad is flag
        y, x = y0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        out = m(y, x)
        out.square().sum().backward()
        res.append((out.detach(), y.grad, x.grad, m.omega.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fused_grad_reaches_the_default_w_of_crfasrnn_and_the_heads():
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler

    assert CRFasRNN(charb(3.0)).W.fused_grad is False
    assert CRFasRNN(charb(3.0), fused_grad=True).W.fused_grad is True
    assert CRFdepthRefiner().CRF.W.fused_grad is False and CRFdepthRefiner(fused_grad=True).CRF.W.fused_grad is True
    assert CRFdepthUpsampler(fused_grad=True).CRF.W.fused_grad is True


def test_binding_rejects_other_tensors():
    import phl

    t = torch.zeros(1, 1, 4, 4)
    with pytest.raises(TypeError):
        phl.guided_filter_grad(t, t, t, 1, 1e-2)
    with pytest.raises(TypeError):
        phl.guided_filter_grad(t.double(), t.double(), t.double(), 1, 1e-2)
