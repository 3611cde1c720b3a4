"""Pins tests/_filter_grad_util.py, the float64 reference of the fused filter backward, on the CPU: against the
reference's own autograd output (tests/golden/grad_*.npz), against the oracle's fp32 filter, and against the fp32
formulation of the reference whose distance from float64 is the noise the GPU tests allow a kernel."""
import os

import numpy as np
import pytest

from _filter_grad_util import Lattice64, filter64, grad64, image_features, scaled, slice_grad_mode, values, wide32


def _oracle(ref):
    from oracle import phl_oracle as po

    return po.Oracle(np.ascontiguousarray(ref, np.float32))


@pytest.mark.parametrize("name,src_key,g_key,bound_ref", [("grad_n80_d3_L2", "src", "gout", 2e-6), ("grad_n2000_d5_L4", "src", "gout", 2e-6),
                                                         ("grad_image_48x64_d5_L64", "src_f16", "gout_f16", 1e-4)])
def test_float64_gradient_reproduces_the_reference_autograd_goldens(golden_dir, name, src_key, g_key, bound_ref):
    """The image golden's grad_ref carries the reference's own fp32 noise at |f| ~ 55 (tests/test_gpu_crf_api.py holds
    the kernels to the same 1e-4 there); everything else is at fp32 rounding."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    ref, src, g = z["ref"], z[src_key].astype(np.float32), z[g_key].astype(np.float32)
    Wg, T = grad64(_oracle(ref), src, ref, g)
    es, er = scaled(z["grad_src"], Wg), scaled(z["grad_ref"], T)
    print(f"[measured] {name}: golden grad_src vs float64 {es:.2e}, grad_ref {er:.2e}")
    assert es <= 2e-6 and er <= bound_ref


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7])
def test_float64_forward_equals_the_oracle_filter(d):
    rng = np.random.default_rng(40 + d)
    f = image_features(40, d, rng)
    src, _ = values(f.shape[0], 8, rng)
    O = _oracle(f)
    e = scaled(O.filter(src), filter64(Lattice64(O), src))
    print(f"[measured] d={d}: Oracle.filter vs float64 {e:.2e}")
    assert e <= 1e-6


# (d, L, side, noise, offset of the first two features, the figure measured for the fp32 formulation against float64)
NOISE_CASES = [(1, 8, 40, 0.2, 0, 6.0e-6), (2, 36, 40, 0.2, 0, 2.7e-6), (3, 20, 48, 0.2, 0, 2.9e-6), (4, 64, 40, 0.2, 0, 1.7e-6),
               (5, 36, 48, 0.2, 0, 4.9e-6), (5, 36, 48, 3.0, 0, 2.4e-6), (5, 36, 48, 0.2, 300, 1.1e-4), (6, 8, 40, 0.2, 0, 2.1e-6),
               (7, 8, 48, 0.2, 0, 2.7e-6)]


@pytest.mark.parametrize("d,L,side,noise,offset,figure", NOISE_CASES)
def test_fp32_formulation_stays_within_twice_its_measured_distance_from_float64(d, L, side, noise, offset, figure):
    """The arithmetic noise of the reference's own fp32 chain: what the GPU tests scale their bound by.  With |f| ~ 300
    the 4L cancelling products lose two more digits -- the same effect as in the image golden."""
    rng = np.random.default_rng(1000 + 10 * d + L)
    f = image_features(side, d, rng, noise=noise)
    f[:, :2] += np.float32(offset)
    src, g = values(f.shape[0], L, rng)
    O = _oracle(f)
    Wg64, T64 = grad64(O, src, f, g)
    Wg32, T32 = wide32(O, src, f, g)
    es, er = scaled(Wg32, Wg64), scaled(T32, T64)
    print(f"[measured] d={d} L={L} n={f.shape[0]} noise={noise} offset={offset}: fp32 formulation vs float64 grad_src {es:.2e}, grad_ref {er:.2e}")
    assert es <= 1e-6
    assert er <= 2 * figure


def test_slice_mode_table():
    """k_slice_grad's choice restated (slice_grad_mode): the vertex counts at which a 256-pixel chunk changes path."""
    P = 256
    for d, last8, last4 in [(5, 88, 176), (2, 192, 381), (1, 295, 581)]:
        for nv_max in (last4 + 1, 700):            # (the budget binds: lds = 80 KiB whatever the worst chunk)
            assert slice_grad_mode(P, d, last8, nv_max) == 8 and slice_grad_mode(P, d, last8 + 1, nv_max) == 4
            assert slice_grad_mode(P, d, last4, nv_max) == 4 and slice_grad_mode(P, d, last4 + 1, nv_max) == 0
    # a chunk of 256 pixels has at most 256 (d + 1) vertices: DIRECT cannot be reached at d = 1
    assert slice_grad_mode(P, 1, 512, 512) == 4
    # the worst chunk of a light lattice sizes the launch for 32-channel slabs for every chunk
    for d in range(1, 8):
        for nv_max in (1, 17, 60):
            assert all(slice_grad_mode(P, d, nv, nv_max) == 8 for nv in range(1, nv_max + 1))
    # below the budget the launch is sized for exactly the worst chunk ...
    assert slice_grad_mode(P, 5, 88, 88) == 8 and slice_grad_mode(P, 2, 192, 192) == 8
    # ... and a smaller budget (PHL_TILE_LDS) moves the bands down
    assert slice_grad_mode(P, 5, 88, 200, budget=40 * 1024) == 0 and slice_grad_mode(P, 5, 30, 200, budget=40 * 1024) == 8
