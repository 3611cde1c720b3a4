"""The backward of the bilinear guided filter without a GPU: the float64 autograd gradients of the repository's torch form
(crf/guided.py, ``mode='bilinear'``) against the reference's (tests/golden/guided_bil_grad_*.npz, written by
tests/golden/generate_guided_bilinear_grad.py), the ``bilinear_grad`` keyword of the classes, the argument checks of
phl_guided_filter_bilinear_grad, which return before the first HIP call, and the chunk query.

Bound of the fixture check: BOUND of tests/test_guided_grad_cpu.py, 1e-12 of each gradient's largest magnitude.  Where the
fixtures were written the largest gap was 2.9e-15 (grad_y of bil_bga_cx1_s3)."""
import ctypes

import numpy as np
import pytest
import torch

from _guided_fixtures import BIL_CASES, fixture_grads, load_grad_case
from test_guided_grad_cpu import BOUND


@pytest.mark.parametrize("name", BIL_CASES)
def test_torch_form_gradients_match_reference_float64(name):
    from crf import guided

    z = load_grad_case(name)
    got = fixture_grads(guided, z, torch.float64, "cpu", "bilinear")
    for k, mine in zip(("y", "x", "omega"), got):
        want = z["grad_" + k]
        mag = float(np.abs(want).max())
        err = float(np.abs(mine.numpy() - want).max())
        print(f"{name} grad_{k}: max |torch float64 - reference float64| = {err:.3e}, scale {mag:.4g}")
        assert mine.shape == want.shape and mag > 0
        assert err <= BOUND * mag, (name, k, err)


# ---- the keyword ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["FastGuidedFilter", "BatchedGuidedAdjacency"])
def test_keyword_of_the_filter_classes(cls):
    from crf import guided

    make = getattr(guided, cls)
    assert make(3, 4, 1e-2, mode="bilinear", fused_bilinear=True).bilinear_grad is False
    assert make(3, 4, 1e-2).bilinear_grad is False
    assert make(3, 4, 1e-2, mode="bilinear", fused_bilinear=True, bilinear_grad=True).bilinear_grad is True
    with pytest.raises(ValueError):
        make(3, 4, 1e-2, mode="bilinear", bilinear_grad=True)
    with pytest.raises(ValueError):
        make(3, 4, 1e-2, bilinear_grad=True)
    with pytest.raises(NotImplementedError):
        make(3, 4, 1e-2, mode="bilinear", fused_bilinear=True, full_cov=True, bilinear_grad=True)
    with pytest.raises(TypeError):
        make(3, 4, 1e-2, 2, "bilinear", True, True)          # keyword-only


def test_keyword_reaches_the_w_of_crfasrnn_and_the_heads():
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    kw = dict(mode="bilinear", fused_bilinear=True, bilinear_grad=True)
    assert CRFasRNN(charb(3.0)).W.bilinear_grad is False
    assert CRFasRNN(charb(3.0), mode="bilinear", fused_bilinear=True).W.bilinear_grad is False
    assert CRFasRNN(charb(3.0), **kw).W.bilinear_grad is True
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), mode="bilinear", bilinear_grad=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), lattice=True, bilinear_grad=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), lattice=True, **kw)
    for head in (CRFdepthRefiner, CRFwUncertainty, CRFdepthUpsampler):
        assert head().CRF.W.bilinear_grad is False
        assert head(**kw).CRF.W.bilinear_grad is True
        with pytest.raises(ValueError):
            head(mode="bilinear", bilinear_grad=True)


@pytest.mark.parametrize("kind", ["fast", "bga"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_keyword_on_cpu_tensors_is_the_torch_form(kind, dtype):
    """bilinear_grad=True changes nothing for tensors the kernels do not take: the same bits as with the keyword off."""
    from crf import guided

    gen = torch.Generator().manual_seed(3)
    y0 = torch.rand((2, 3, 20, 26), generator=gen, dtype=dtype)
    x0 = torch.rand((2, 2, 20, 26), generator=gen, dtype=dtype)
    cls = guided.FastGuidedFilter if kind == "fast" else guided.BatchedGuidedAdjacency
    res = []
    for flag in (False, True):
        m = cls(2, 3, 1e-2, subsample_ratio=2, mode="bilinear", fused_bilinear=True, bilinear_grad=flag).to(dtype)
        y, x = y0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        out = m(y, x)
        out.square().sum().backward()
        res.append((out.detach(), y.grad, x.grad, m.omega.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- the C entry point ------------------------------------------------------------------------------------------------
OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
Y, X, G, GY, GX, GE, E = (0x1000 * k for k in range(1, 8))     # fake device addresses, never dereferenced


def _args(y=Y, x=X, g=G, gy=GY, gx=GX, ge=GE, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, eps=E, scale=1.0, sub=1, flags=0):
    return (y, x, g, gy, gx, ge, B, cy, cx, H, W, h, w, r, eps, scale, sub, flags)


ARG_CASES = [
    (_args(y=None), INVALID), (_args(x=None), INVALID), (_args(g=None), INVALID), (_args(eps=None), INVALID),
    (_args(B=-1), INVALID), (_args(cy=-1), INVALID), (_args(cx=0), INVALID), (_args(H=-3), INVALID), (_args(h=0), INVALID),
    (_args(w=0), INVALID), (_args(r=-1), INVALID), (_args(h=49), INVALID), (_args(scale=float("nan")), INVALID),
    (_args(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE),
    (_args(cx=17), UNSUPPORTED), (_args(flags=1), UNSUPPORTED), (_args(flags=2), UNSUPPORTED),
    (_args(h=25), UNSUPPORTED), (_args(w=33), UNSUPPORTED), (_args(H=3, h=2), UNSUPPORTED),
    (_args(gy=Y), INVALID), (_args(gy=G), INVALID), (_args(gx=X), INVALID), (_args(ge=E), INVALID), (_args(gx=GY), INVALID),
    (_args(B=0, y=None, x=None, g=None), OK), (_args(cy=0, y=None, g=None), OK), (_args(H=0, h=0, y=None, g=None), OK),
    (_args(gy=None, gx=None, ge=None), OK), (_args(gy=None, gx=None, ge=None, flags=1), OK),   # nothing asked for: nothing launched
    (_args(cx=17, flags=1, h=25, gy=Y), UNSUPPORTED),       # the order: channels, flags and sizes before the aliasing check
]


@pytest.mark.parametrize("args,status", ARG_CASES, ids=[str(i) for i in range(len(ARG_CASES))])
def test_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    a = list(args)
    a[15] = ctypes.c_float(a[15])
    assert lib.phl_guided_filter_bilinear_grad(*a, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_guided_filter_bilinear_grad"), lib.phl_last_error()


def test_abi_row():
    import phl

    row = [r for r in phl._ABI if r[0] == "phl_guided_filter_bilinear_grad"]
    assert row == [("phl_guided_filter_bilinear_grad", "i", "PPPPPPiiiiiiiiPfiIS")]
    names = [r[0] for r in phl._ABI]
    assert names.index("phl_guided_filter_bilinear_grad") == names.index("phl_guided_filter_bilinear_labels_per_chunk") + 1


@pytest.mark.parametrize("needs", range(1, 8))
def test_chunk_query_is_the_nearest_backward_below_full_resolution(needs):
    """Labels per chunk of the call (phl.h: phl_guided_filter_labels_per_chunk with full = 0), worked by hand: a label
    holds, at h x w, ys (4 bytes), P and Q (8 (cx + 1)), for grad_x A and mA (8 cx), for grad_x or grad_eps three fp64
    terms a channel (24 cx); 96 MiB a chunk, at least one label, at most B cy and 65535."""
    import phl

    need_y, need_x, need_eps = bool(needs & 1), bool(needs & 2), bool(needs & 4)
    for B, cy, cx, h, w in ((2, 11, 16, 128, 128), (1, 64, 3, 555, 695), (2, 3, 3, 20, 33), (1, 70000, 1, 2, 2)):
        per = h * w * (4 + 8 * (cx + 1) + (8 * cx if need_x else 0) + (24 * cx if need_x or need_eps else 0))
        want = max(1, min(B * cy, 65535, (96 << 20) // per))
        got = phl.guided_filter_labels_per_chunk(B, cy, cx, h, w, need_y=need_y, need_x=need_x, need_eps=need_eps)
        assert got == want, (B, cy, cx, h, w, needs)


def test_binding_rejects_other_arguments():
    import phl

    t = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear_grad(t, t, t, 1, 1e-2, subsample=1)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear_grad(t, t, t, 1, 1e-2, subsample=2)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear_grad(t.double(), t.double(), t.double(), 1, 1e-2, subsample=2)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear_grad(t, t, t, 1, 1e-2)                   # subsample is required
