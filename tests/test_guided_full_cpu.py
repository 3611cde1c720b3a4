"""The full-covariance guided filter (``full_cov=True``, crf/guided.py) without a GPU: its float64 torch form against
explicit loops, the single-channel case against the diagonal model, the affine reproduction that only the off-diagonal
terms give, the unchanged default, the argument checks of phl_guided_filter_full (which return before the first HIP call)
and the constructors.

Bounds.  Explicit loops: 1e-12 of max|out|, as tests/test_guided_cpu.py holds the diagonal form to its fixtures (both
sides are float64; they differ by the order of the window sums and by inverse-times-vector against a solve, at condition
numbers up to 1 / eps = 100).  cx = 1: 1e-13 of max|out| (the two forms differ by one rounding of 1 / (var + eps); 1.1e-15
measured).  Affine reproduction at eps = 1e-10: the full model within 1e-6 (2.3e-9 measured: the model's own eps bias), the
diagonal model off by at least 1e-2 (0.14 measured)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _guided_fixtures import build_module, load_case
from _guided_util import affine_inputs, brute_force, correlated_guide


def _random(shape_y, cx, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.rand(shape_y, generator=gen, dtype=torch.float64)
    x = correlated_guide(shape_y[0], cx, *shape_y[2:], gen, dtype=torch.float64)
    return y, x


@pytest.mark.parametrize("r", [1, 2])
def test_float64_torch_form_against_explicit_loops_plain(r):
    from crf import guided

    y, x = _random((1, 2, 7, 9), 3, r)
    m = guided.GuidedFilter(3, r, 1e-2, full_cov=True).double()
    with torch.no_grad():
        got = m(y, x).numpy()
    want = brute_force(y.numpy(), x.numpy(), r, m.eps.detach().numpy())
    err, mag = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"gf r{r}: |torch float64 - loops| = {err:.3e} of {mag:.4g}")
    assert got.shape == want.shape and err <= 1e-12 * mag


def test_float64_torch_form_against_explicit_loops_adjacency():
    from crf import guided

    y, x = _random((1, 2, 9, 11), 3, 7)
    m = guided.BatchedGuidedAdjacency(3, 2, 1e-2, subsample_ratio=2, full_cov=True).double()
    with torch.no_grad():
        got = m(y, x).numpy()
    want = brute_force(y.numpy(), x.numpy(), 2, m.eps.detach().numpy(), s=2, scale=0.5 * 5 ** 2, subtract=True)
    err, mag = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"bga r2 s2: |torch float64 - loops| = {err:.3e} of {mag:.4g}")
    assert got.shape == want.shape and err <= 1e-12 * mag


def test_one_channel_is_the_diagonal_model():
    from crf import guided

    gen = torch.Generator().manual_seed(2)
    y = torch.rand((2, 3, 30, 40), generator=gen, dtype=torch.float64)
    x = torch.rand((2, 1, 30, 40), generator=gen, dtype=torch.float64)
    full = guided.BatchedGuidedAdjacency(1, 4, 1e-2, subsample_ratio=2, full_cov=True).double()
    diag = guided.BatchedGuidedAdjacency(1, 4, 1e-2, subsample_ratio=2).double()
    with torch.no_grad():
        a, b = full(y, x), diag(y, x)
    err, mag = float((a - b).abs().max()), float(b.abs().max())
    print(f"cx = 1: |full - diagonal| = {err:.3e} of {mag:.4g}")
    assert err <= 1e-13 * mag


def test_affine_reproduction_needs_the_off_diagonal_terms():
    from crf import guided

    y, x = affine_inputs()
    with torch.no_grad():
        e_full = float((guided.GuidedFilter(3, 3, 1e-10, full_cov=True).double()(y, x) - y).abs().max())
        e_diag = float((guided.GuidedFilter(3, 3, 1e-10).double()(y, x) - y).abs().max())
    print(f"affine y: |full - y| = {e_full:.3e}  |diagonal - y| = {e_diag:.3e}")
    assert e_full <= 1e-6
    assert e_diag >= 1e-2


def test_full_form_is_differentiable_by_plain_autograd():
    from crf import guided

    y, x = _random((1, 2, 9, 11), 3, 5)
    y.requires_grad_(True), x.requires_grad_(True)
    m = guided.FastGuidedFilter(3, 2, 1e-2, subsample_ratio=2, full_cov=True, fused_grad=True).double()
    m(y, x).square().sum().backward()
    for g in (y.grad, x.grad, m.omega.grad):
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_default_is_unchanged():
    from crf import guided

    z = load_case("gf_r4")
    y, x = torch.from_numpy(z["y"]), torch.from_numpy(z["x"])
    plain = build_module(guided, z, torch.float32, "cpu")
    flagged = guided.GuidedFilter(int(z["cx"]), int(z["r"]), 1e-2, full_cov=False)
    flagged.load_state_dict(plain.state_dict())
    assert flagged.full_cov is False and plain.full_cov is False
    with torch.no_grad():
        assert torch.equal(plain(y, x), flagged(y, x))
    full = guided.GuidedFilter(int(z["cx"]), int(z["r"]), 1e-2, full_cov=True)
    assert list(full.state_dict()) == list(plain.state_dict()) == ["omega"]
    with torch.no_grad():
        assert not torch.equal(plain(y, x), full(y, x))            # (three guide channels: the flag does change the model)


OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
Y, X, SRC, OUT, M1, M2, M3, M4, E = (0x1000 * k for k in range(1, 10))       # fake device addresses, never dereferenced


def _args(y=Y, x=X, src=SRC, out=OUT, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, m1=M1, m2=M2, m3=M3, m4=M4, eps=E, scale=1.0):
    return (y, x, src, out, B, cy, cx, H, W, h, w, r, m1, m2, m3, m4, eps, scale)


# the argument sets of tests/test_guided_grad_cpu.py in the forward's list (out in the place of g and of the gradients)
ARG_CASES = [
    (_args(B=-1), INVALID), (_args(cy=-1), INVALID), (_args(cx=0), INVALID), (_args(H=-3), INVALID), (_args(r=-1), INVALID),
    (_args(h=49), INVALID), (_args(w=65), INVALID), (_args(h=0), INVALID), (_args(scale=float("inf")), INVALID),
    (_args(y=None), INVALID), (_args(x=None), INVALID), (_args(out=None), INVALID), (_args(eps=None), INVALID),
    (_args(m1=None), INVALID), (_args(m4=None), INVALID), (_args(out=Y), INVALID), (_args(out=X), INVALID), (_args(out=SRC), INVALID),
    (_args(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE), (_args(B=1 << 20, cy=1 << 20), TOO_LARGE),
    (_args(H=(1 << 30) + 1, W=1, h=8, w=1), TOO_LARGE), (_args(cx=17), UNSUPPORTED),
    (_args(B=0, y=None, x=None, out=None), OK), (_args(cy=0, y=None, out=None), OK), (_args(H=0, h=0, y=None, out=None), OK),
]


@pytest.mark.parametrize("args,status", ARG_CASES, ids=[str(i) for i in range(len(ARG_CASES))])
def test_guided_filter_full_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    a = list(args)
    a[17] = ctypes.c_float(a[17])
    assert lib.phl_guided_filter(*a, None) == status
    assert lib.phl_guided_filter_full(*a, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_guided_filter_full"), lib.phl_last_error()


def test_guided_filter_full_channel_bound():
    import phl

    lib = phl.load_library()
    assert phl.GUIDED_FULL_MAX_CX == 4
    a = list(_args(cx=5))
    a[17] = ctypes.c_float(a[17])
    assert lib.phl_guided_filter_full(*a, None) == UNSUPPORTED
    msg = lib.phl_last_error().decode()
    assert msg.startswith("phl_guided_filter_full") and "at most 4" in msg, msg
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phl.h")).read()
    assert "#define PHL_GUIDED_FULL_MAX_CX 4\n" in header


def test_constructors():
    from crf import guided
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    for cls in (guided.GuidedFilter, guided.FastGuidedFilter, guided.BatchedGuidedAdjacency):
        assert cls(3, 4, 1e-2).full_cov is False and cls(3, 4, 1e-2, full_cov=True).full_cov is True
        with pytest.raises(NotImplementedError):
            cls(3, 4, 1e-2, gaussian=True, full_cov=True)
        with pytest.raises(TypeError):
            cls(3, 4, 1e-2, False, False, True)                  # keyword-only
    guide = torch.rand(1, 3, 8, 9)
    assert guided.GuidedAdjacency(guide, 2, 1e-2).full_cov is False
    assert guided.GuidedAdjacency(guide, 2, 1e-2, full_cov=True).full_cov is True
    assert CRFasRNN(charb(3.0)).W.full_cov is False
    assert CRFasRNN(charb(3.0), gchannels=3, full_cov=True).W.full_cov is True
    with pytest.raises(ValueError):
        CRFasRNN(charb(3.0), lattice=True, full_cov=True)
    with pytest.raises(NotImplementedError):
        CRFasRNN(charb(3.0), gaussian=True, full_cov=True)
    for head in (CRFdepthRefiner, CRFwUncertainty, CRFdepthUpsampler):
        assert head().CRF.W.full_cov is False and head(full_cov=True).CRF.W.full_cov is True


def test_guided_adjacency_matmul_full_cov_on_cpu():
    """The flat ``W @ U`` form takes the flag through to the torch form: the same numbers as BatchedGuidedAdjacency."""
    from crf import guided

    gen = torch.Generator().manual_seed(9)
    guide = correlated_guide(1, 3, 12, 14, gen)
    U = torch.rand((12 * 14, 4), generator=gen)
    W = guided.GuidedAdjacency(guide, 2, 1e-2, full_cov=True)
    m = guided.BatchedGuidedAdjacency(3, 2, 1e-2, subsample_ratio=1, full_cov=True)
    with torch.no_grad():
        want = m(U.t().reshape(1, 4, 12, 14), guide)[0].reshape(4, -1).t()
    assert torch.equal(W @ U, want)
