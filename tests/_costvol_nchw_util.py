"""What the channel-major cost-volume tests and the winner-takes-all tests share (csrc/phl_costvol_nchw.hip).

The exactness argument is tests/_costvol_util.py's: on ``cu.int_images`` every raw cost and window sum is an integer, and
fp32 is exact in any order while every intermediate stays below 2^24.  The kernel's summation form keeps that file's bound:
its horizontal sums are running sums restarted every 8 columns, its vertical ones running sums down the 8 rows of a tile,
and both add the entering element before they subtract the leaving one -- at most ws + 1 raw costs in a horizontal
intermediate, ws + 1 rows of ws in a vertical one, ``cu.running_sum_bound``.  No wider prefix sum exists, so the pixels
are drawn from ``cu.PIXEL_RANGE`` unchanged (test_costvol_nchw_host.py asserts the bound for every case used here).

References are computed once per case (lru_cache) and shared by both GPU test files; callers do not write into them."""
import ctypes as C
import functools

import numpy as np

import _costvol_util as cu

B = 2                                                # items of the batched cases
EDGE_L = 33                                          # disparities of the tile / reflect sweep
BLOCK_CASE = (17, 40, 5, "SD", 3)                    # (h, w, window, criterion, channels) of the disparity-block sweep
TIE_CASE = (19, 37, 41)                              # (h, w, disparities): one channel, integer pixels in [-2, 2], AD
CONSUMER_CASE = (24, 40, 6, 5, "AD", 3)              # (h, w, disparities, window, criterion, channels)


def edge_heights(ty):
    return (1, 2, ty - 1, ty, ty + 1, 2 * ty + 1)


def edge_widths(tx):
    return (1, 2, 3, tx - 1, tx, tx + 1, 2 * tx + 1)


def block_counts(dc, volume=True):
    return (1, dc - 1, dc, dc + 1, 2 * dc + 1, 97) if volume else (1, dc, dc + 1, 2 * dc + 1)


@functools.lru_cache(maxsize=None)
def instance_case(ws, crit):
    """The 27-instance case: B items of cu.SHAPE with cu.channels_of channels (item 0 seed ws, item 1 seed ws + 1000) as
    float64 [B, h, w, c] arrays, and the oracle's float64 volume [B, h, w, L]."""
    from oracle import costvol_oracle as co

    (h, w), L, c = cu.SHAPE, cu.MAX_DISP, cu.channels_of(ws, crit)
    pairs = [cu.int_images(h, w, c, crit, seed=ws + 1000 * i) for i in range(B)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return a, b, np.stack([co.disparity_badness(a[i], b[i], ws, crit, max_disp=L) for i in range(B)])


@functools.lru_cache(maxsize=None)
def edge_case(ws, crit, c, h, w):
    """One shape of the tile / reflect sweep: a pair [h, w, c] and cu.reference_volume [h, w, EDGE_L]."""
    a, b = cu.int_images(h, w, c, crit, seed=100 * h + w)
    return a, b, cu.reference_volume(a, b, ws, crit, EDGE_L)


@functools.lru_cache(maxsize=None)
def block_case(L):
    """The disparity-block sweep: B items [B, h, w, c] (seeds L and L + 1000) and the oracle's volume [B, h, w, L]."""
    from oracle import costvol_oracle as co

    h, w, ws, crit, c = BLOCK_CASE
    pairs = [cu.int_images(h, w, c, crit, seed=L + 1000 * i) for i in range(B)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return a, b, np.stack([co.disparity_badness(a[i], b[i], ws, crit, max_disp=L) for i in range(B)])


def tie_images():
    h, w, _ = TIE_CASE
    rng = np.random.default_rng(3)
    return (rng.integers(-2, 3, size=(h, w, 1)).astype(np.float64), rng.integers(-2, 3, size=(h, w, 1)).astype(np.float64))


def tied_minimum(volume):
    """Pixels of a [..., L] volume whose minimum is attained more than once."""
    return (volume == volume.min(-1, keepdims=True)).sum(-1) > 1


def planar(a):
    """float64 [B, h, w, c] (or [h, w, c]) numpy -> contiguous [B, c, h, w] torch tensor on the CPU."""
    import torch

    a = a[None] if a.ndim == 3 else a
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def to_hwl(t):
    """[B, L, H, W] device tensor -> float64 numpy [B, H, W, L], the oracle's axis order."""
    return t.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)


def first_difference(got, want):
    """cu.first_difference over the items of two [B, h, w, L] arrays."""
    for i in range(want.shape[0]):
        diff = cu.first_difference(got[i], want[i])
        if diff:
            return f"item {i}: {diff}"
    return None


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def wta_into(disp, cost, a, b, L, ws, crit):
    """phl_disparity_wta through the C ABI into caller-owned (possibly strided) int32 ``disp`` / fp32 ``cost`` views
    [B, H, W]; a, b: contiguous fp32 CUDA [B, C, H, W]."""
    import phl
    import torch

    Bn, c, h, w = a.shape
    assert a.is_contiguous() and b.is_contiguous() and disp.stride(2) == 1 and disp.stride() == cost.stride()
    lib = phl.load_library()
    with torch.cuda.device(a.device):
        rc = lib.phl_disparity_wta(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), Bn, h, w, c, c * h * w, w, 1, h * w, L, ws,
                                   phl.CRITERIA[crit], C.c_void_p(disp.data_ptr()), C.c_void_p(cost.data_ptr()), disp.stride(0),
                                   disp.stride(1), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.phl_last_error().decode()
