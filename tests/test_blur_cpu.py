"""The separable Gaussian of the guided filter on the CPU (plain-torch path) against the reference's own float64 results
(tests/golden/generate_blur.py), the notebook-facing names, and the C-ABI argument checks of phl_box_blur /
phl_box_blur_grad (every case returns before the first HIP call: no GPU, fake pointers never dereferenced)."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cases():
    z = np.load(os.path.join(GOLDEN, "blur_cases.npz"))
    return z, [str(n) for n in z["names"]]


def test_notebook_imports():
    from crf.gaussian_matrix import GaussianBlur, box_filter, gaussian_blur  # TestGaussianBlur.ipynb cell 1

    ns = {}
    exec("from crf.gaussian_matrix import *", ns)                               # trainableDenseCRF.ipynb
    assert ns["GaussianBlur"] is GaussianBlur and ns["gaussian_blur"] is gaussian_blur and ns["box_filter"] is box_filter


def test_box_filter_ones_quirk():
    from crf.guided import box_filter

    h, r = 20, 3
    y = box_filter(torch.ones(h, dtype=torch.float64), r, 0)
    assert y[0] == 1.0                                           # window 0..r, divisor r + 1
    assert abs(float(y[h // 2]) - 2 * r / (2 * r + 1)) < 1e-15   # 2r samples over 2r + 1
    assert abs(float(y[-1]) - r / (r + 1)) < 1e-15


@pytest.mark.parametrize("r", [0, -2])
def test_box_filter_rejects_r(r):
    from crf.guided import box_filter

    with pytest.raises(ValueError):
        box_filter(torch.ones(5), r, 0)


def test_forward_and_gradients_match_reference():
    from crf.guided import GaussianBlur, box_filter

    z, names = _cases()
    assert len(names) == 30
    for n in names:
        v = torch.from_numpy(z[f"{n}/v"]).requires_grad_(True)
        g = torch.from_numpy(z[f"{n}/g"])
        dim = int(z[f"{n}/dim"])
        sigma = torch.tensor(float(z[f"{n}/sigma"]), dtype=torch.float64, requires_grad=True)
        y = GaussianBlur.apply(v, sigma, dim)
        (y * g).sum().backward()
        np.testing.assert_allclose(y.detach().numpy(), z[f"{n}/out"], rtol=0, atol=1e-12, err_msg=n)
        np.testing.assert_allclose(v.grad.numpy(), z[f"{n}/grad_x"], rtol=0, atol=1e-12, err_msg=n)
        gs = float(z[f"{n}/grad_sigma"])
        assert abs(float(sigma.grad) - gs) <= 1e-12 * max(1.0, abs(gs)), (n, float(sigma.grad), gs)
        np.testing.assert_allclose(box_filter(torch.from_numpy(z[f"{n}/v"]), 3, dim).numpy(), z[f"{n}/box"], rtol=0, atol=1e-12)


def test_number_sigma_and_no_sigma_grad():
    from crf.guided import gaussian_blur

    z, names = _cases()
    n = names[-1]
    v = torch.from_numpy(z[f"{n}/v"]).requires_grad_(True)
    y = gaussian_blur(v, 3, int(z[f"{n}/dim"]))          # a Python number, as the notebook passes
    np.testing.assert_allclose(y.detach().numpy(), z[f"{n}/out"], rtol=0, atol=1e-12)
    (y * torch.from_numpy(z[f"{n}/g"])).sum().backward()
    np.testing.assert_allclose(v.grad.numpy(), z[f"{n}/grad_x"], rtol=0, atol=1e-12)
    s = torch.tensor(3.0, dtype=torch.float64)            # a tensor without requires_grad gets none
    v2 = torch.from_numpy(z[f"{n}/v"]).requires_grad_(True)
    gaussian_blur(v2, s, int(z[f"{n}/dim"])).sum().backward()
    assert s.grad is None and v2.grad is not None


def test_sigma_to_r_table():
    from crf.guided import sigma_radius

    z = np.load(os.path.join(GOLDEN, "blur_sigma_r.npz"))
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        got = [sigma_radius(torch.tensor(s, dtype=dt)) for s in z[f"sigma_{name}"]]
        assert got == [int(r) for r in z[f"r_{name}"]], name


def test_guided_filter_gaussian_matches_reference():
    from crf.guided import GuidedFilter

    z = np.load(os.path.join(GOLDEN, "blur_guided.npz"))
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    y = torch.from_numpy(z["y"]).requires_grad_(True)
    gf = GuidedFilter(channels=3, r=2, eps=1e-2, gaussian=True)
    out = gf(y, x)
    (out * torch.from_numpy(z["g_out"])).sum().backward()
    np.testing.assert_allclose(out.detach().numpy(), z["out"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(x.grad.numpy(), z["grad_x"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(y.grad.numpy(), z["grad_y"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(gf.omega.grad.numpy(), z["grad_omega"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gf.omega2.grad.numpy(), z["grad_omega2"], rtol=1e-5, atol=1e-6)
    assert float(gf.r().detach()) == pytest.approx(2.0)


def test_guided_filter_gaussian_window_assert():
    from crf.guided import GuidedFilter

    gf = GuidedFilter(channels=1, r=5, eps=1e-2, gaussian=True)
    with pytest.raises(AssertionError):
        gf(torch.rand(1, 1, 10, 30), torch.rand(1, 1, 10, 30))     # h = 10 is not > 2 r + 1 = 11


def test_fast_guided_and_crfasrnn_gaussian_still_refuse():
    from crf.crf_module import CRFasRNN, charb
    from crf.guided import BatchedGuidedAdjacency, FastGuidedFilter

    with pytest.raises(NotImplementedError):
        FastGuidedFilter(1, 4, 1e-2, gaussian=True)
    with pytest.raises(NotImplementedError):
        BatchedGuidedAdjacency(1, 4, 1e-2, gaussian=True)
    with pytest.raises(NotImplementedError):
        CRFasRNN(charb(3.0), niters=1, gaussian=True)


OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
A, B, C, D = 0x1000, 0x2000, 0x3000, 0x4000
BIG = 1 << 40
ARG_CASES = [
    # phl_box_blur(src, dst, outer, h, inner, r, passes)
    ("phl_box_blur", (A, B, 2, 8, 3, 0, 3), INVALID),
    ("phl_box_blur", (A, B, 2, 8, 3, -1, 3), INVALID),
    ("phl_box_blur", (A, B, -1, 8, 3, 2, 3), INVALID),
    ("phl_box_blur", (A, B, 2, -8, 3, 2, 3), INVALID),
    ("phl_box_blur", (A, B, 2, 8, -3, 2, 3), INVALID),
    ("phl_box_blur", (A, B, 2, 8, 3, 2, 0), INVALID),
    ("phl_box_blur", (A, B, 2, 8, 3, 2, 9), INVALID),
    ("phl_box_blur", (None, B, 2, 8, 3, 2, 3), INVALID),
    ("phl_box_blur", (A, None, 2, 8, 3, 2, 3), INVALID),
    ("phl_box_blur", (A, A, 2, 8, 3, 2, 3), INVALID),
    ("phl_box_blur", (A, B, BIG, BIG, 3, 2, 3), TOO_LARGE),
    ("phl_box_blur", (A, B, 1 << 37, 4, 1, 2, 3), TOO_LARGE),          # 2^31 workgroups
    ("phl_box_blur", (None, None, 0, 8, 3, 2, 3), OK),
    ("phl_box_blur", (None, None, 4, 0, 3, 2, 8), OK),
    # phl_box_blur_grad(v, g, outer, h, inner, r, sigma, grad_x, grad_sigma)
    ("phl_box_blur_grad", (A, B, 2, 8, 3, 0, 3.0, C, D), INVALID),
    ("phl_box_blur_grad", (A, B, -2, 8, 3, 1, 3.0, C, D), INVALID),
    ("phl_box_blur_grad", (A, B, 2, 8, 3, 1, 0.0, C, D), INVALID),
    ("phl_box_blur_grad", (A, B, 2, 8, 3, 1, -1.0, C, D), INVALID),
    ("phl_box_blur_grad", (A, B, 2, 8, 3, 1, float("nan"), C, D), INVALID),
    ("phl_box_blur_grad", (A, B, 2, 8, 3, 1, 3.0, None, None), INVALID),
    ("phl_box_blur_grad", (None, B, 2, 8, 3, 1, 3.0, C, D), INVALID),
    ("phl_box_blur_grad", (A, None, 2, 8, 3, 1, 3.0, C, D), INVALID),
    ("phl_box_blur_grad", (A, B, 2, 8, 3, 1, 3.0, A, D), INVALID),
    ("phl_box_blur_grad", (A, B, BIG, BIG, 3, 1, 3.0, C, D), TOO_LARGE),
    ("phl_box_blur_grad", (A, B, 2, 1000, 3, 200, 3.0, C, D), UNSUPPORTED),
    ("phl_box_blur_grad", (A, B, 2, 1000, 1, 200, 3.0, None, D), UNSUPPORTED),
]


@pytest.mark.parametrize("name,args,status", ARG_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(ARG_CASES)])
def test_blur_entry_point_argument_checks(name, args, status):
    import ctypes

    import phl

    lib = phl.load_library()
    if name == "phl_box_blur_grad":
        args = args[:6] + (ctypes.c_double(args[6]),) + args[7:]
    assert getattr(lib, name)(*args, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith(name), lib.phl_last_error()


def test_fused_limits():
    import phl

    for rows in (False, True):
        assert phl.box_blur_fused_max_r(rows, 1) == 2 ** 31 - 1
        m3 = phl.box_blur_fused_max_r(rows, 3)
        assert 30 <= m3 < 200
        assert 30 <= phl.box_blur_fused_max_r(rows, 3, grad=True) < 200
        assert phl.box_blur_fused_max_r(rows, 8) < m3
