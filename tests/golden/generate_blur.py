"""Golden vectors for the separable Gaussian of the guided filter: the reference's own box_filter / GaussianBlur /
GuidedFilter(gaussian=True) (crf/gaussian_matrix.py:86-232), run on the CPU in float64 through generate.py's import
shim (this script only imports its helpers; generate.py itself is not changed).

    python tests/golden/generate_blur.py      -> tests/golden/blur_cases.npz, blur_guided.npz, blur_sigma_r.npz

blur_cases.npz      for every axis of 1-D .. 4-D inputs and three axis lengths (h < r, h = 2r, h > 6r): the input v, a
                    fixed upstream gradient g, the forward, grad_x and grad_sigma (keys "<case>/<name>", plus "names")
blur_guided.npz     GuidedFilter(channels=3, r=2, eps=1e-2, gaussian=True) on y [1, 2, 12, 14] guided by x [1, 3, 12, 14]:
                    the output for a fixed upstream gradient and the gradients of omega, omega2, x and y
blur_sigma_r.npz    the sigma -> r table around the boundaries 4 sigma^2 + 1 = (2k)^2, in float32 and float64
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate as gen  # noqa: E402

SIGMA = 3.0            # r = 3


def blur_cases(gm):
    import torch

    rng = np.random.default_rng(11)
    out, names = {}, []
    r = 3
    for nd in (1, 2, 3, 4):
        for dim in range(nd):
            for h in (2, 2 * r, 7 * r + 2):
                shape = [3, 2, 4, 3][:nd]
                shape[dim] = h
                v = torch.from_numpy(rng.standard_normal(shape))
                g = torch.from_numpy(rng.standard_normal(shape))
                sigma = torch.tensor(SIGMA, dtype=torch.float64, requires_grad=True)
                vv = v.clone().requires_grad_(True)
                y = gm.GaussianBlur.apply(vv, sigma, dim)
                (y * g).sum().backward()
                name = f"nd{nd}_dim{dim}_h{h}"
                names.append(name)
                out.update({f"{name}/v": v.numpy(), f"{name}/g": g.numpy(), f"{name}/dim": np.int64(dim),
                            f"{name}/sigma": np.float64(SIGMA), f"{name}/out": y.detach().numpy(),
                            f"{name}/grad_x": vv.grad.numpy(), f"{name}/grad_sigma": sigma.grad.numpy()})
                box = gm.box_filter(v, r, dim)
                out[f"{name}/box"] = box.numpy()
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "blur_cases.npz"), **out)
    print("wrote blur_cases.npz", len(names), "cases")


def blur_guided(gm):
    import torch

    torch.manual_seed(3)
    h, w = 12, 14
    x = torch.rand(1, 3, h, w, dtype=torch.float64, requires_grad=True)
    y = torch.rand(1, 2, h, w, dtype=torch.float64, requires_grad=True)
    g_out = torch.randn(1, 2, h, w, dtype=torch.float64)
    gf = gm.GuidedFilter(channels=3, r=2, eps=1e-2, gaussian=True)
    out = gf(y, x)
    (out * g_out).sum().backward()
    np.savez_compressed(os.path.join(HERE, "blur_guided.npz"), x=x.detach().numpy(), y=y.detach().numpy(), g_out=g_out.numpy(),
                        out=out.detach().numpy(), grad_omega=gf.omega.grad.numpy(), grad_omega2=gf.omega2.grad.numpy(),
                        grad_x=x.grad.numpy(), grad_y=y.grad.numpy(), r=np.float64(2), eps=np.float64(1e-2))
    print("wrote blur_guided.npz", dict(omega2=float(gf.omega2.grad), omega=gf.omega.grad.numpy()))


def sigma_r_table():
    import torch

    k = np.arange(1, 61, dtype=np.float64)
    centre = np.sqrt((4 * k * k - 1) / 4)
    tables = {}
    for name, dt, npdt in (("f32", torch.float32, np.float32), ("f64", torch.float64, np.float64)):
        c = centre.astype(npdt)
        s = np.unique(np.concatenate([c, np.nextafter(c, npdt(0)), np.nextafter(c, npdt(np.inf)), np.array([0.5, 1, 2.5, 20, 30],
                                                                                                             dtype=npdt)]))
        # the reference's line (gaussian_matrix.py:118), niters = 3
        r = [int(np.floor(np.sqrt(12 * torch.tensor(si, dtype=dt) ** 2 / 3 + 1)) // 2) for si in s]
        tables[f"sigma_{name}"] = s
        tables[f"r_{name}"] = np.array(r, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "blur_sigma_r.npz"), **tables)
    print("wrote blur_sigma_r.npz", {k_: v.shape for k_, v in tables.items()})


if __name__ == "__main__":
    import torch

    torch.set_num_threads(1)
    _, gm = gen.import_reference_python()
    blur_cases(gm)
    blur_guided(gm)
    sigma_r_table()
