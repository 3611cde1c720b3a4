"""The fused compatibility + softmax step for 256 < L <= 512 labels (k_compat_wide, phl_compat_wide.hip, reached through
phl_compat_softmax_split / phl.compat_softmax): parity against float64, the route the binding takes, the mean-field
paths at the reference's 341 labels, reference-generated golden vectors, and repeatability."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("L", [260, 288, 300, 344, 352, 384, 444, 508, 512])
def test_wide_compat_softmax_parity(L):
    """Ragged n (1, less than one 64-pixel tile, several tiles plus every tail class mod 4 and mod 64, more tiles than
    resident workgroups), an asymmetric Mu, row-padded views of E0, X and out, softmax and logits epilogues -- against
    float64 (bound: twice the error of torch's fp32 GEMM + softmax on the same operands)."""
    import phl

    g = torch.Generator(device="cuda").manual_seed(L)
    Mu = torch.rand((L, L), device="cuda", generator=g) * 2
    Mu[: L // 2] *= 0.5                                      # not symmetric
    assert not torch.equal(Mu, Mu.t())
    sizes = (1, 37, 64 * 5 + 1, 64 * 6 + 2, 64 * 7 + 3, 64 * 9 + 63, 64 * 1100 + 17)
    for n in sizes:
        for logits in (False, True):
            pe, px, po = 4, 8, 12
            E0 = (torch.rand((n, L + pe), device="cuda", generator=g) * 25 - 5)[:, :L]
            X = (torch.rand((n, L + px), device="cuda", generator=g) - 0.2)[:, :L]
            out = torch.full((n, L + po), -7.0, device="cuda")
            got = phl.compat_softmax(E0, X, Mu, out=out[:, :L], logits=logits)
            E = E0 + X @ Mu
            E64 = E0.double() + X.double() @ Mu.double()
            want = -E64 if logits else torch.softmax(-E64, dim=1)
            e_torch = float(((-E if logits else torch.softmax(-E, dim=1)).double() - want).abs().max())
            err = float((got.double() - want).abs().max())
            tol = 1e-4 * float(E64.abs().max()) if logits else max(2e-6, 2 * e_torch)
            print(f"[measured] wide compat n={n} L={L} logits={logits}: max abs err vs fp64 {err:.2e} "
                  f"(torch fp32 {e_torch:.2e}, tol {tol:.2e})")
            assert bool(torch.isfinite(got).all())
            assert err <= tol, (n, L, logits, err, tol)
            if not logits:
                assert float((got.sum(1) - 1).abs().max()) <= 1e-5
            assert bool((out[:, L:] == -7.0).all()), "wrote into the row padding"


def test_wide_route_takes_the_split_kernel_and_no_matmul():
    """At L = 344 (the padded 341 of a 2048-column image) the default compat_softmax calls phl_compat_softmax_split and
    runs no torch matrix product; arith="f32" keeps the library route (GEMM + fused softmax)."""
    import phl
    from torch.overrides import TorchFunctionMode

    L, n = 344, 64 * 20 + 5
    g = torch.Generator(device="cuda").manual_seed(7)
    E0 = torch.rand((n, L), device="cuda", generator=g) * 10
    X = torch.rand((n, L), device="cuda", generator=g)
    Mu = torch.rand((L, L), device="cuda", generator=g)
    lib = phl.load_library()
    real = lib.phl_compat_softmax_split
    taken = []

    class _Spy:                                   # (ctypes function objects take no attributes: wrap the call)
        def __call__(self, *a):
            taken.append(a[9])
            return real(*a)

    class _Products(TorchFunctionMode):
        def __init__(self):
            super().__init__()
            self.seen = []

        def __torch_function__(self, func, types, args=(), kwargs=None):
            name = getattr(func, "__name__", "")
            if name in ("matmul", "mm", "__matmul__", "addmm", "bmm"):
                self.seen.append(name)
            return func(*args, **(kwargs or {}))

    lib_attr = lib.phl_compat_softmax_split
    lib.phl_compat_softmax_split = _Spy()
    try:
        phl.compat_softmax(E0, X, Mu)                          # warm-up: the Mu^T / planes caches
        taken.clear()
        with _Products() as mode:
            got = phl.compat_softmax(E0, X, Mu)
        assert taken == [L] and not mode.seen, (taken, mode.seen)
        taken.clear()
        with _Products() as mode:
            lib_route = phl.compat_softmax(E0, X, Mu, arith="f32")
        assert not taken and mode.seen, (taken, mode.seen)
    finally:
        lib.phl_compat_softmax_split = lib_attr
    want = torch.softmax(-(E0.double() + X.double() @ Mu.double()), dim=1)
    e_wide, e_lib = (float((r.double() - want).abs().max()) for r in (got, lib_route))
    print(f"[measured] L={L}: wide kernel {e_wide:.2e}, library route {e_lib:.2e} max abs err vs fp64")
    assert e_wide <= max(2e-6, 2 * e_lib)


def _mf_problem(L=341, h=24, w=40, seed=5 * 341):
    import crf.crf_module as cm

    g = torch.Generator(device="cpu").manual_seed(seed)
    n = h * w
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ref = torch.stack([yy / 6, xx / 6, torch.rand((h, w), generator=g) * 3], dim=-1).reshape(n, 3)
    E0 = torch.rand((n, L), generator=g) * 8
    labels = torch.arange(L, dtype=torch.float32)
    Mu = cm.compatibility_matrix(lambda a, b: cm.charbonneir(a, b, 2.0), labels) * 0.05
    return ref, E0, Mu


def test_mean_field_L341_paths_take_the_wide_kernel():
    """mean_field_infer on device tensors, on CPU tensors (the staged path) and CRFasRNN's fused NCHW path at L = 341
    (padded to 344 by crf_module._label_pad) reach k_compat_wide, and match the same iteration written with torch ops on
    the unpadded tensors."""
    import crf.crf_module as cm
    import phl
    from crf.gaussian_matrix import LatticeGaussian

    dev = torch.device("cuda")
    L, niters, h, w = 341, 3, 24, 40
    ref, E0, Mu = _mf_problem(L, h, w)
    W = LatticeGaussian(ref.to(dev))
    Q = torch.softmax(-E0.to(dev), dim=1)
    for _ in range(niters):                                  # crf_module.py:49-52 on the unpadded tensors
        Q = torch.softmax(-(E0.to(dev) + (W @ Q) @ Mu.to(dev)), dim=1)
    want = Q
    lib = phl.load_library()
    real = lib.phl_compat_softmax_split
    taken = []

    class _Spy:
        def __call__(self, *a):
            taken.append(a[9])
            return real(*a)

    lib.phl_compat_softmax_split = _Spy()
    try:
        got = cm.mean_field_infer(E0.to(dev), W, Mu.to(dev), niters)
        n_gpu = len(taken)
        got_cpu = cm.mean_field_infer(E0, LatticeGaussian(ref), Mu, niters)
        n_cpu = len(taken) - n_gpu
        # CRFasRNN over NCHW tensors with the lattice W: logits of the last iteration
        crf = cm.CRFasRNN(cm.charb(2.0), niters=2, lattice=True).to(dev)
        refs = ref.t().reshape(1, 3, h, w).to(dev)
        logits_in = -E0.t().reshape(1, L, h, w).to(dev)
        lab = torch.arange(L, dtype=torch.float32, device=dev)
        with torch.no_grad():
            out_fused = crf(refs, logits_in, labels=lab)
        n_nchw = len(taken) - n_gpu - n_cpu
    finally:
        lib.phl_compat_softmax_split = real
    assert n_gpu == niters and n_cpu == niters and n_nchw >= 2, (n_gpu, n_cpu, n_nchw)
    assert all(c == 344 for c in taken), taken
    for name, res in (("gpu tensors", got), ("cpu tensors", got_cpu.to(dev))):
        err = float((res - want).abs().max())
        print(f"[measured] mean field at L={L} ({name}): max abs diff to the unpadded torch iteration {err:.2e}")
        assert res.shape == (h * w, L) and err <= 4e-5
        assert float((res.sum(1) - 1).abs().max()) <= 1e-5
    # the NCHW path against CRFasRNN's own autograd modules (plain conv / lattice modules, no fused kernel)
    lg = logits_in.clone().requires_grad_(True)
    out_ag = crf(refs, lg, labels=lab)
    scale = float(out_ag.detach().abs().max())
    e_nchw = float((out_fused - out_ag.detach()).abs().max()) / scale
    print(f"[measured] CRFasRNN NCHW at L={L}: fused vs autograd path {e_nchw:.2e} (of the largest logit)")
    assert out_fused.shape == (1, L, h, w) and e_nchw <= 1e-5


def test_mean_field_L341_golden(golden_dir):
    """Reference-generated vectors (tests/golden/generate_wide.py: the reference's mean_field_infer over its own engine) at
    the reference's 341 labels on a 20 x 33 Tsukuba crop, 1, 5 and 10 iterations."""
    import phl
    from crf.crf_module import charbonneir, compatibility_matrix, mean_field_infer
    from crf.gaussian_matrix import LatticeGaussian

    g = np.load(os.path.join(golden_dir, "meanfield_tsukuba_L341.npz"))
    dev = torch.device("cuda")
    E0 = torch.from_numpy(g["E0_f16"].astype(np.float32)).to(dev)
    ref = torch.from_numpy(g["ref"]).to(dev)
    labels = torch.from_numpy(g["labels"]).to(dev)
    assert E0.shape == (int(g["h"]) * int(g["w"]), 341) and E0.shape[0] % 64 != 0
    Mu = compatibility_matrix(lambda a, b: charbonneir(a, b, float(g["gamma"])), labels)
    lib = phl.load_library()
    real = lib.phl_compat_softmax_split
    taken = []

    class _Spy:
        def __call__(self, *a):
            taken.append(a[9])
            return real(*a)

    lib.phl_compat_softmax_split = _Spy()
    try:
        W = LatticeGaussian(ref)
        for it in (1, 5, 10):
            Q = mean_field_infer(E0, W, Mu, it)
            eq = rel(Q.cpu().numpy(), g[f"Q{it}"])
            disp = (Q @ labels).cpu().numpy()
            ed = float((np.abs(disp - g[f"disp{it}"]) / np.maximum(np.abs(g[f"disp{it}"]), 1e-2)).max())
            print(f"[measured] mean field L=341, {it} iteration(s): Q rel {eq:.2e}, disparity rel per pixel {ed:.2e}")
            assert eq <= 5e-4 and ed <= 1e-4
    finally:
        lib.phl_compat_softmax_split = real
    assert len(taken) == 16 and all(c == 344 for c in taken), taken


def test_wide_compat_softmax_repeatable():
    """Bit-identical results across repeated launches at a size with many tiles per CU (no race in the LDS ring hand-off
    or the counted waits)."""
    import phl

    n, L = 64 * 4001 + 3, 344
    g = torch.Generator(device="cuda").manual_seed(1)
    E0 = torch.rand((n, L), device="cuda", generator=g) * 20
    X = torch.rand((n, L), device="cuda", generator=g)
    Mu = torch.rand((L, L), device="cuda", generator=g) * 2
    first = phl.compat_softmax(E0, X, Mu).clone()
    want = torch.softmax(-(E0.double() + X.double() @ Mu.double()), dim=1)
    assert float((first.double() - want).abs().max()) <= 2e-4
    out = torch.empty_like(first)
    for it in range(10):
        phl.compat_softmax(E0, X, Mu, out=out)
        assert torch.equal(out, first), f"launch {it} differs from the first"
