"""TEST INFRASTRUCTURE ONLY -- an independent float64 evaluation of what phl_filter_grad (include/phl.h) computes.

"Gradient" means the reference's formulation (crf/gaussian_matrix.py:450-463, our ``_ref_gradient``) evaluated exactly,
not the true derivative: for d >= 2 the axis-by-axis blur is not self-adjoint and the reference ignores that.

Everything here runs on the CPU from the oracle's lattice (``oracle.phl_oracle.Oracle``: first-touch vertex ids, the
barycentric weights and the blur neighbours); nothing touches the GPU lattice.

* ``filter64``   splat / blur / slice in float64 numpy;
* ``grad64``     (W g, T) with T[:, k] = -2 sum_l (s f_k Wg - s W(g f_k) + g f_k Ws - g W(s f_k)), feature by feature;
* ``wide32``     the reference's own formulation in fp32: the 2L(1+d)-channel operand through ``Oracle.filter`` and the
                 fp32 contraction.  Its distance from ``grad64`` is the arithmetic noise a kernel is judged against;
* ``slice_grad_mode``  which of k_slice_grad's three code paths a chunk takes.
"""
import numpy as np


def scaled(a, b):
    """max |a - b| as a fraction of the largest component of b (the float64 side)."""
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


class Lattice64:
    """The oracle's lattice as float64 numpy arrays (read once per Oracle)."""

    def __init__(self, O):
        self.n, self.d, self.M = O.n, O.d, O.M
        vid, w = O.replay()
        self.vid = vid.astype(np.int64)
        self.w = w.astype(np.float64)
        self.nbr = O.neighbors().astype(np.int64)          # [d+1, M, 2], -1 = absent


def filter64(lat, X):
    """Splat, blur (axes 0..d in order, Jacobi, an absent neighbour counts as 0: phlo_blur) and slice of X [n, C]."""
    X = np.asarray(X, np.float64)
    V = np.zeros((lat.M, X.shape[1]), np.float64)
    for k in range(lat.d + 1):
        np.add.at(V, lat.vid[:, k], lat.w[:, k, None] * X)
    for axis in range(lat.d + 1):
        a, b = lat.nbr[axis, :, 0], lat.nbr[axis, :, 1]
        Va = np.where((a >= 0)[:, None], V[np.maximum(a, 0)], 0.0)
        Vb = np.where((b >= 0)[:, None], V[np.maximum(b, 0)], 0.0)
        V = 0.5 * Va + V + 0.5 * Vb
    out = np.zeros_like(X)
    for k in range(lat.d + 1):
        out += lat.w[:, k, None] * V[lat.vid[:, k]]
    return out / (1.0 + 2.0 ** -lat.d)


def grad64(O, src, ref, g):
    """(Wg [n, L], T [n, d]) in float64.  One feature at a time: memory stays at n * L doubles per array."""
    lat = O if isinstance(O, Lattice64) else Lattice64(O)
    s, f, gg = (np.asarray(x, np.float64) for x in (src, ref, g))
    Wg, Ws = filter64(lat, gg), filter64(lat, s)
    T = np.empty((lat.n, lat.d), np.float64)
    for k in range(lat.d):
        fk = f[:, k, None]
        T[:, k] = -2.0 * (s * fk * Wg - s * filter64(lat, gg * fk) + gg * fk * Ws - gg * filter64(lat, s * fk)).sum(1)
    return Wg, T


def wide32(O, src, ref, g):
    """(Wg, T) as the reference computes them, in fp32 on the CPU: the operand [g, g(x)ref, src, src(x)ref] of
    gaussian_matrix.py:450-455 through the oracle's filter, then the contraction of :456-463 (torch's fp32 sum)."""
    import torch
    from crf.gaussian_matrix import _ref_gradient, _wide_operand

    s, f, gg = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) for x in (src, ref, g))
    wall = torch.from_numpy(O.filter(_wide_operand(s, f, gg).numpy()))
    return wall[:, :s.shape[1]].numpy().copy(), _ref_gradient(s, f, gg, wall).numpy()


def slice_grad_mode(P, d, nv, nv_max, budget=80 * 1024):
    """Code path of k_slice_grad<d + 1> (csrc/phl_tiles.hip) for a chunk of ``nv`` local vertices in a lattice whose
    worst chunk has ``nv_max``: 8 (32-channel slabs, LG = 8), 4 (16-channel slabs, LG = 4) or 0 (DIRECT).

    phl_launch_slice_grad gives every workgroup  lds = min(fixed(nv_max) + nv_max * NS * 128, lds_budget())  bytes with
    NS = d + 1 and  fixed(nv) = (P * NS * 8 + P * 4 + nv * 4 + 15) & ~15  (entries, pixel ids, local vertex ids);
    k_slice_grad then takes  mode = fixed(nv) + nv * NS * 128 <= lds ? 8 : fixed(nv) + nv * NS * 64 <= lds ? 4 : 0.
    ``budget`` is lds_budget()'s default (PHL_TILE_LDS unset)."""
    NS = d + 1

    def fixed(v):
        return (P * NS * 8 + P * 4 + v * 4 + 15) & ~15

    lds = min(fixed(nv_max) + nv_max * NS * 128, budget)
    if fixed(nv) + nv * NS * 128 <= lds:
        return 8
    if fixed(nv) + nv * NS * 64 <= lds:
        return 4
    return 0


def image_features(side, d, rng, noise=0.2, scale=1.0):
    """Image-like features of a side x side picture: the pixel grid / 4 and sines with ``noise``; d = 1: a ramp."""
    n = side * side
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float32)
    if d == 1:
        return ((np.arange(n, dtype=np.float32) / (4 * side) + rng.random(n, dtype=np.float32) * noise) * scale).reshape(n, 1).astype(np.float32)
    cols = [xx.ravel() / 4, yy.ravel() / 4] + [np.sin(xx.ravel() / (7 + 3 * k)) * 2 + rng.random(n, dtype=np.float32) * noise
                                               for k in range(d - 2)]
    return (np.stack(cols[:d], 1) * scale).astype(np.float32)


def values(n, L, rng):
    """src uniform in [0, 1), g standard normal."""
    return rng.random((n, L), dtype=np.float32), rng.standard_normal((n, L)).astype(np.float32)
