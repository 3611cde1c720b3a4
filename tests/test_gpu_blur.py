"""HIP separable Gaussian (phl_blur.hip) on the GPU: the fused box cascade against float64 on every axis, both sides of
the fused kernel's radius limit, the sigma-gradient against the reference's goldens and float64, determinism, and
GuidedFilter(gaussian=True) / the notebook's sigma fit on the device."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda", 0)


def _ref64(x, r, dim, passes=3):
    from crf.guided import _box_torch

    y = x.double()
    for _ in range(passes):
        y = _box_torch(y, r, dim)
    return y


def _check(x, r, dim, passes=3):
    import phl

    got = phl.box_blur(x, r, dim, passes=passes)
    want = _ref64(x, r, dim, passes)
    err = float((got.double() - want).abs().max()) if x.numel() else 0.0
    scale = float(x.abs().max()) if x.numel() else 1.0
    assert err <= 1e-6 * scale, (tuple(x.shape), r, dim, passes, err)


@pytest.mark.parametrize("shape", [(300, 3), (3, 300), (2, 257, 64), (5, 1, 700), (2, 3, 130, 70), (1, 70, 3, 1)])
@pytest.mark.parametrize("r", [1, 4, 11])
def test_forward_every_axis(shape, r):
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(shape, device=DEV, generator=g)
    for dim in range(len(shape)):
        _check(x, r, dim)


@pytest.mark.parametrize("h", [1, 2, 5, 64, 1000, 5000])
@pytest.mark.parametrize("inner", [1, 3, 65])
def test_forward_lengths(h, inner):
    g = torch.Generator(device=DEV).manual_seed(h + inner)
    x = torch.rand((3, h, inner), device=DEV, generator=g) - 0.3
    for r in (1, 7, 40):                        # h = 1, h < r, h crossing several chunks
        _check(x, r, 1)


@pytest.mark.parametrize("inner", [1, 64])
@pytest.mark.parametrize("passes", [1, 2, 3, 5, 8])
def test_fused_limit_both_sides(inner, passes):
    import phl

    lim = phl.box_blur_fused_max_r(inner == 1, passes)
    g = torch.Generator(device=DEV).manual_seed(passes)
    h = 2600
    x = torch.randn((2, h, inner), device=DEV, generator=g)
    for r in {min(lim, 300), min(lim + 1, 400), 3}:
        _check(x, r, 1, passes)


def test_noncontiguous_and_out():
    import phl

    g = torch.Generator(device=DEV).manual_seed(3)
    base = torch.randn((40, 90, 6), device=DEV, generator=g)
    x = base.permute(2, 0, 1)[:, ::2]           # [6, 20, 90], no unit stride
    for dim in range(3):
        _check(x, 5, dim)
    out = torch.empty(x.shape, device=DEV)
    assert phl.box_blur(x, 5, 2, out=out) is out


def test_accuracy_not_worse_than_fp32_torch():
    from crf.guided import _box_torch

    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand((64, 2048), device=DEV, generator=g) + 10.0      # large offset: prefix sums lose bits
    import phl

    want = _ref64(x, 30, 1)
    hip = float((phl.box_blur(x, 30, 1).double() - want).abs().max())
    y = x
    for _ in range(3):
        y = _box_torch(y, 30, 1)
    torch32 = float((y.double() - want).abs().max())
    assert hip <= torch32, (hip, torch32)


def test_gradients_match_goldens():
    from crf.guided import GaussianBlur

    z = np.load(os.path.join(GOLDEN, "blur_cases.npz"))
    for n in [str(s) for s in z["names"]]:
        v = torch.from_numpy(z[f"{n}/v"]).float().to(DEV).requires_grad_(True)
        g = torch.from_numpy(z[f"{n}/g"]).float().to(DEV)
        sigma = torch.tensor(float(z[f"{n}/sigma"]), device=DEV, requires_grad=True)
        y = GaussianBlur.apply(v, sigma, int(z[f"{n}/dim"]))
        (y * g).sum().backward()
        sc = max(1.0, float(np.abs(z[f"{n}/v"]).max()))
        assert np.abs(y.detach().cpu().double().numpy() - z[f"{n}/out"]).max() <= 1e-6 * sc, n
        assert np.abs(v.grad.cpu().double().numpy() - z[f"{n}/grad_x"]).max() <= 2e-6 * sc, n
        gs = float(z[f"{n}/grad_sigma"])
        assert abs(float(sigma.grad) - gs) <= 1e-5 * max(1.0, abs(gs)) + 1e-5 * np.abs(z[f"{n}/v"]).sum(), (n, float(sigma.grad), gs)


def _grad64(v, g, r, dim, sigma):
    """float64 reference formulas of the backward (torch path of crf.guided in float64)."""
    from crf.guided import GaussianBlur

    vv = v.double().cpu().requires_grad_(True)
    s = torch.tensor(float(sigma), dtype=torch.float64, requires_grad=True)
    (GaussianBlur.apply(vv, s, dim) * g.double().cpu()).sum().backward()
    return vv.grad, float(s.grad)


@pytest.mark.parametrize("dim", [0, 1])
@pytest.mark.parametrize("sigma", [5.0, 30.0])
def test_sigma_gradient_large(dim, sigma):
    import phl
    from crf.guided import sigma_radius

    gen = torch.Generator(device=DEV).manual_seed(11)
    v = torch.rand((1536, 2048), device=DEV, generator=gen)
    g = torch.randn((1536, 2048), device=DEV, generator=gen)
    r = sigma_radius(torch.tensor(sigma))
    gx, gs = phl.box_blur_grad(v, g, r, dim, sigma)
    gx64, gs64 = _grad64(v, g, r, dim, sigma)
    assert float((gx.double().cpu() - gx64).abs().max()) <= 1e-6 * float(g.abs().max())
    rel = abs(float(gs) - gs64) / abs(gs64)
    assert rel <= 1e-4, (float(gs), gs64, rel)
    _, gs2 = phl.box_blur_grad(v, g, r, dim, sigma)
    assert gs.cpu().numpy().tobytes() == gs2.cpu().numpy().tobytes()       # fixed-order reduction: same bits


def test_sigma_gradient_above_fused_limit():
    import phl

    gen = torch.Generator(device=DEV).manual_seed(2)
    v = torch.rand((3, 700, 1), device=DEV, generator=gen)
    g = torch.randn((3, 700, 1), device=DEV, generator=gen)
    r = phl.box_blur_fused_max_r(True, 3, grad=True) + 5
    sigma = 2.0 * r / np.sqrt(12 / 3)
    gx, gs = phl.box_blur_grad(v, g, r, 1, sigma)
    vv = v.double().cpu().requires_grad_(True)
    from crf.guided import GaussianBlur, sigma_radius

    s = torch.tensor(sigma, dtype=torch.float64, requires_grad=True)
    assert sigma_radius(s) == r
    (GaussianBlur.apply(vv, s, 1) * g.double().cpu()).sum().backward()
    assert float((gx.double().cpu() - vv.grad).abs().max()) <= 1e-6 * float(g.abs().max())
    assert abs(float(gs) - float(s.grad)) <= 1e-4 * abs(float(s.grad))


def test_no_sigma_work_without_sigma_grad(monkeypatch):
    import phl
    from crf.guided import gaussian_blur

    calls = []
    real = phl._launch
    monkeypatch.setattr(phl, "_launch", lambda dev, name, *a: (calls.append(name), real(dev, name, *a))[1])
    v = torch.rand((50, 60), device=DEV, requires_grad=True)
    gaussian_blur(v, torch.tensor(4.0, device=DEV), 0).sum().backward()
    assert "phl_box_blur_grad" not in calls and calls.count("phl_box_blur") == 2, calls
    calls.clear()
    s = torch.tensor(4.0, device=DEV, requires_grad=True)
    gaussian_blur(v, s, 0).sum().backward()
    assert "phl_box_blur_grad" in calls and s.grad is not None


def test_guided_filter_gaussian_gpu():
    from crf.guided import GuidedFilter

    z = np.load(os.path.join(GOLDEN, "blur_guided.npz"))
    x = torch.from_numpy(z["x"]).float().to(DEV).requires_grad_(True)
    y = torch.from_numpy(z["y"]).float().to(DEV).requires_grad_(True)
    gf = GuidedFilter(channels=3, r=2, eps=1e-2, gaussian=True).to(DEV)
    out = gf(y, x)
    (out * torch.from_numpy(z["g_out"]).float().to(DEV)).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), z["out"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), z["grad_x"], rtol=0, atol=1e-3 * np.abs(z["grad_x"]).max())
    np.testing.assert_allclose(y.grad.cpu().numpy(), z["grad_y"], rtol=0, atol=1e-3 * np.abs(z["grad_y"]).max())
    np.testing.assert_allclose(gf.omega.grad.cpu().numpy(), z["grad_omega"], rtol=2e-3, atol=1e-4)
    np.testing.assert_allclose(gf.omega2.grad.cpu().numpy(), z["grad_omega2"], rtol=2e-3, atol=1e-4)


def test_notebook_sigma_fit_tracks_float64():
    """TestGaussianBlur.ipynb cell 8: Adam on log sigma, fitting a two-axis blur of an impulse."""
    from crf.guided import GaussianBlur, gaussian_blur

    def run(device, dtype):
        h, w = 288, 384
        e0 = torch.zeros(h, w, dtype=dtype, device=device)
        e0[20, 100] = 1
        bxy = GaussianBlur.apply(GaussianBlur.apply(e0, 20, 0), 20, 1)
        alpha = torch.nn.Parameter(torch.log(torch.tensor(30.)).float())
        opt = torch.optim.Adam([alpha], lr=1e-1)
        traj = []
        for _ in range(5):
            opt.zero_grad()
            sigma = torch.exp(alpha)
            loss = ((gaussian_blur(gaussian_blur(e0, sigma, 0), sigma, 1) - bxy.detach()) ** 2).sum()
            loss.backward()
            traj.append((float(loss.detach()), float(torch.exp(alpha.detach())), float(alpha.grad)))
            opt.step()
        return np.array(traj)

    gpu, cpu = run(DEV, torch.float32), run("cpu", torch.float64)
    np.testing.assert_allclose(gpu[:, 1], cpu[:, 1], rtol=1e-4)
    np.testing.assert_allclose(gpu[:, 0], cpu[:, 0], rtol=1e-3, atol=1e-9)
    np.testing.assert_allclose(gpu[:, 2], cpu[:, 2], rtol=1e-3, atol=1e-7)
