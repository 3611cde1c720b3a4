"""TEST INFRASTRUCTURE ONLY -- the named inputs of the fused feature gradient at 8 <= d <= 16 and what the host test
and the GPU test (test_filter_grad_highd_host.py, test_gpu_filter_grad_highd.py) both need of them.

The rule and its constants are those of tests/test_gpu_filter_grad64.py, restated here:
    e_fused <= K * max(e_ref, FLOOR)   with K = 4, FLOOR = 1e-6, and never above CAP_REF = 2e-4 (features) /
    CAP_SRC = 1e-5 (source), every error a fraction of the largest float64 component;
``e_ref`` is the distance of the reference's own fp32 formulation (``wide32``, tests/_filter_grad_util.py) from
``grad64`` on the same inputs.  An input is only fit to be judged by K if its e_ref_T is at most CAP_REF / K = 5e-5:
above that the cap, not K, would judge.  That is a statement about the inputs alone; the host test holds it for every
input named here.

Two feature families, n = 48 x 48 pixels, seeds as in test_gpu_filter_grad64.py (7000 + 100 d + L):
  * "image":  image_features(48, d, rng, noise=0.0, scale=s) -- the pixel grid / 4 and sines.  s = 1 up to d = 13; at
              d = 14, 15 and 16 the staged splat declines s = 1 on the MI355X (M / n = 2.1 .. 2.5 and S_multi = 4842 ..
              5264 multi-chunk slots, above the 2 n = 4608 it takes: tile_stats says staged_splat == 0 and the call
              returns status 7), so those three run at s = 0.5 (M / n = 0.9 at d = 16, S_multi = 3620);
  * "smooth": cumsum(rand * 0.02, axis 0) minus its mean (centred: the uncentred form loses digits to |f| itself).
and, for the declined-or-taken case only, iid features (``iid_case``).
"""
import numpy as np

from _filter_grad_util import Lattice64, grad64, image_features, values, wide32

K = 4
FLOOR = 1e-6
CAP_REF, CAP_SRC = 2e-4, 1e-5          # the bounds of tests/test_gpu_filter_grad64.py (and of tests/test_gpu_grad.py)
E_REF_T_MAX = CAP_REF / K              # 5e-5: what every named input must meet on the CPU

SIDE = 48

# case 1: every d -- (d, L)
EVERY_D = [(d, L) for d in (8, 9, 14, 15, 16) for L in (4, 36, 64)] + [(d, 20) for d in (10, 11, 12, 13)]
# ... and d = 10 .. 13 at the one L whose wide rows ((cols + 1) * 64 = 320 .. 448 channels) take the three-axes blur route
EVERY_D += [(d, 64) for d in (10, 11, 12, 13)]
# case 2: smooth centred features
SMOOTH = [(8, 64), (16, 64)]
# case 6: the staged forms of the contracting slice at d >= 8.  (d, L, scale of the image features, form of the worst
# chunk, its local vertices as tile_stats reported them on an MI355X): the smaller the picture against a simplex, the
# more pixels share a vertex (the knob of SLICE_MODES in test_gpu_filter_grad64.py).
# At d = 16 the index data alone takes 36 KiB of the 80: the 7-block group of 6+5+5 gathers from memory where the two
# 6-block groups still stage.
STAGED_FORMS = [(9, 36, 0.12, (8, 8), 58), (9, 36, 0.25, (4, 4), 109), (16, 36, 0.12, (0, 4, 4), 151)]


def image_scale(d):
    """Scale of the image features of case 1 (module docstring)."""
    return 0.5 if d >= 14 else 1.0


_CASES = {}


def feature_groups(d, cap=7):
    """[(k0, columns)] as phl_filter_grad (csrc/phl_api.hip) cuts d features: ceil(d / cap) groups, as even as possible,
    the larger ones first."""
    ng = (d + cap - 1) // cap
    out, k0 = [], 0
    for i in range(ng):
        cols = d // ng + (1 if i < d % ng else 0)
        out.append((k0, cols))
        k0 += cols
    return out


def slice_grad_group_mode(P, d, cols, nv, nv_max, budget=80 * 1024):
    """Code path of k_slice_grad_group<cols + 1> (csrc/phl_tiles.hip) for a chunk of ``nv`` local vertices in a lattice
    whose worst chunk has ``nv_max``: 8 (32-channel slabs), 4 (16-channel slabs) or 0 (DIRECT).  Mirrors
    _filter_grad_util.slice_grad_mode with the two numbers it had as one: NV = d + 1 vertices per pixel size the index
    data, NB = cols + 1 blocks size a staged row.

    The launcher gives  lds = fixed(nv_max) + nv_max * NB * 128, or, where that exceeds lds_budget(), the budget -- but
    never less than fixed(nv_max);  fixed(nv) = (P * NV * 8 + P * 4 + nv * 4 + 15) & ~15."""
    NV, NB = d + 1, cols + 1

    def fixed(v):
        return (P * NV * 8 + P * 4 + v * 4 + 15) & ~15

    lds = fixed(nv_max) + nv_max * NB * 128
    if lds > budget:
        lds = max(budget, fixed(nv_max))
    if fixed(nv) + nv * NB * 128 <= lds:
        return 8
    if fixed(nv) + nv * NB * 64 <= lds:
        return 4
    return 0


class Case:
    """Inputs and the two CPU evaluations of one case (as Case of test_gpu_filter_grad64.py); computed once per key and
    shared, read-only."""

    def __init__(self, f, L, rng):
        from oracle import phl_oracle as po

        self.f = np.ascontiguousarray(f, np.float32)
        self.n, self.d = self.f.shape
        self.L = L
        self.src, self.g = values(self.n, L, rng)
        O = po.Oracle(self.f)
        self.M = O.M
        self.Wg64, self.T64 = grad64(Lattice64(O), self.src, self.f, self.g)
        self.Wg32, self.T32 = wide32(O, self.src, self.f, self.g)
        self.scale_T = float(np.abs(self.T64).max())
        self.scale_S = float(np.abs(self.Wg64).max())
        self.e_ref_T = float(np.abs(self.T32 - self.T64).max() / self.scale_T)
        self.e_ref_S = float(np.abs(self.Wg32 - self.Wg64).max() / self.scale_S)
        for a in (self.f, self.src, self.g, self.Wg64, self.T64, self.Wg32, self.T32):
            a.setflags(write=False)

    def cuda(self):
        import torch

        return tuple(torch.tensor(x, device="cuda") for x in (self.f, self.src, self.g))        # (copies: the arrays are read-only)


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _rng(d, L):
    return np.random.default_rng(7000 + 100 * d + L)


def image_case(d, L, scale=None):
    scale = image_scale(d) if scale is None else scale

    def make():
        rng = _rng(d, L)
        return Case(image_features(SIDE, d, rng, noise=0.0, scale=scale), L, rng)

    return _case(("image", d, L, scale), make)


def smooth_case(d, L):
    def make():
        rng = _rng(d, L)
        f = np.cumsum(rng.random((SIDE * SIDE, d), dtype=np.float32) * np.float32(0.02), axis=0)
        return Case((f - f.mean(0)).astype(np.float32), L, rng)

    return _case(("smooth", d, L), make)


def iid_features(d, L):
    """iid uniform features in [0, 6): next to no sharing between neighbouring pixels."""
    rng = _rng(d, L)
    return (rng.random((SIDE * SIDE, d), dtype=np.float32) * 6).astype(np.float32), rng


def named_cases():
    """(tag, constructor) of every input the GPU test judges by the rule."""
    out = [(f"image d={d} L={L}", (lambda d=d, L=L: image_case(d, L))) for d, L in EVERY_D]
    out += [(f"smooth d={d} L={L}", (lambda d=d, L=L: smooth_case(d, L))) for d, L in SMOOTH]
    out += [(f"image d={d} L={L} scale={s}", (lambda d=d, L=L, s=s: image_case(d, L, s))) for d, L, s, _, _ in STAGED_FORMS]
    out += [("image d=5 L=36", lambda: image_case(5, 36)), ("image d=9 L=136", lambda: image_case(9, 136))]
    return out
