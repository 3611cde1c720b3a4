"""What needs no GPU of the stereo sweep's three entry points (include/phl.h: phl_cost_volume, phl_cost_volume_nchw,
phl_disparity_wta): the argument checks of each with the status it returns and the order they run in -- every case
returns before the first HIP call, the fake addresses are never dereferenced --, what the binding refuses, the numpy
side of the reference's names, and the precondition of the exact GPU tests."""
import numpy as np
import pytest
import torch

import _costvol_nchw_util as nu
import _costvol_util as cu

OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
I1, I2, O, O2, MIS = 1 << 50, 1 << 51, 1 << 52, 1 << 53, (1 << 52) + 4       # fake device addresses, far apart; MIS off the 16-byte grid
I31 = (1 << 31) - 1
NEGATE = 1


def vol(i1=I1, i2=I2, B=2, h=4, w=8, C=3, st=None, L=5, ws=9, crit=0, flags=0, out=O, obs=None, ols=None, oys=None):
    """Arguments of phl_cost_volume_nchw; unnamed strides are those of dense planar images and a dense [B, L, h, w] volume."""
    st = (C * h * w, w, 1, h * w) if st is None else st
    oys = w if oys is None else oys
    ols = h * oys if ols is None else ols
    obs = L * ols if obs is None else obs
    return (i1, i2, B, h, w, C, *st, L, ws, crit, flags, out, obs, ols, oys)


def wta(i1=I1, i2=I2, B=2, h=4, w=8, C=3, st=None, L=5, ws=9, crit=0, disp=O, cost=O2, obs=None, oys=None):
    st = (C * h * w, w, 1, h * w) if st is None else st
    oys = w if oys is None else oys
    obs = h * oys if obs is None else obs
    return (i1, i2, B, h, w, C, *st, L, ws, crit, disp, cost, obs, oys)


def pix(i1=I1, i2=I2, h=4, w=8, C=3, L=5, ws=9, crit=0, out=O, ors=None):
    """Arguments of phl_cost_volume (pixel-major [h*w][L]); the unnamed row stride is the dense one."""
    return (i1, i2, h, w, C, L, ws, crit, out, L if ors is None else ors)


PIXEL_MAJOR = [
    # the supported set, before everything else: also with bad sizes, NULL pointers, a short row stride
    (pix(C=0), UNSUPPORTED), (pix(C=5), UNSUPPORTED), (pix(ws=0), UNSUPPORTED), (pix(ws=4), UNSUPPORTED),
    (pix(ws=19), UNSUPPORTED), (pix(ws=-3), UNSUPPORTED), (pix(crit=3), UNSUPPORTED), (pix(crit=-1), UNSUPPORTED),
    (pix(C=5, h=0), UNSUPPORTED), (pix(ws=2, i1=None, out=None), UNSUPPORTED), (pix(crit=7, L=-1), UNSUPPORTED),
    (pix(C=0, i1=None, i2=None), UNSUPPORTED), (pix(ws=19, ors=4), UNSUPPORTED), (pix(crit=3, L=0, w=0), UNSUPPORTED),
    # an image without pixels is PHL_ERR_INVALID here (not PHL_OK as in the channel-major entry points), also with max_disp = 0
    (pix(h=0), INVALID), (pix(w=0), INVALID), (pix(h=-4), INVALID), (pix(w=-8), INVALID),
    (pix(h=0, L=0), INVALID), (pix(w=0, L=0, out=None), INVALID),
    (pix(L=-1), INVALID), (pix(L=-1, ors=-1), INVALID),
    # max_disp = 0: PHL_OK with or without an output, after the image pointers and the row stride
    (pix(L=0), OK), (pix(L=0, out=None), OK), (pix(L=0, out=None, ors=7), OK),
    (pix(L=0, i1=None), INVALID), (pix(L=0, i2=None, out=None), INVALID), (pix(L=0, ors=-1), INVALID),
    # NULL with elements present
    (pix(i1=None), INVALID), (pix(i2=None), INVALID), (pix(out=None), INVALID),
    # rows that would overlap
    (pix(ors=4), INVALID), (pix(ors=0), INVALID), (pix(L=1, ors=0), INVALID),
]
VOLUME = [
    # the supported set, before everything else: also with negative sizes, NULL pointers, zero sizes, bad strides
    (vol(C=0), UNSUPPORTED), (vol(C=5), UNSUPPORTED), (vol(ws=0), UNSUPPORTED), (vol(ws=4), UNSUPPORTED),
    (vol(ws=19), UNSUPPORTED), (vol(ws=-3), UNSUPPORTED), (vol(crit=3), UNSUPPORTED), (vol(crit=-1), UNSUPPORTED),
    (vol(flags=2), UNSUPPORTED), (vol(flags=NEGATE | 4), UNSUPPORTED),
    (vol(C=5, h=-1), UNSUPPORTED), (vol(ws=2, i1=None, out=None), UNSUPPORTED), (vol(crit=7, B=0), UNSUPPORTED),
    (vol(flags=8, oys=1), UNSUPPORTED), (vol(C=0, i1=None, i2=None), UNSUPPORTED),
    # negative sizes, before the zero sizes
    (vol(B=-1), INVALID), (vol(h=-4), INVALID), (vol(w=-8), INVALID), (vol(L=-1), INVALID),
    (vol(B=0, h=-1), INVALID), (vol(L=0, w=-1), INVALID), (vol(h=0, L=-2, i1=None), INVALID),
    # zero sizes: PHL_OK, whatever the pointers and strides
    (vol(B=0), OK), (vol(h=0), OK), (vol(w=0), OK), (vol(L=0), OK),
    (vol(B=0, i1=None, i2=None, out=None), OK), (vol(L=0, out=None, flags=NEGATE), OK), (vol(w=0, out=I1, oys=0, ols=0, obs=0), OK),
    (vol(L=0, i1=MIS, i2=MIS, out=MIS, st=(0, 0, 0, 0), obs=-5), OK), (vol(B=0, h=I31, w=I31, L=I31), OK),
    # NULL with elements present
    (vol(i1=None), INVALID), (vol(i2=None), INVALID), (vol(out=None), INVALID),
    # overlapping rows: each stride against what it steps over
    (vol(oys=7), INVALID), (vol(oys=-8), INVALID), (vol(oys=12, ols=3 * 12 + 7), INVALID), (vol(ols=-32), INVALID),
    (vol(oys=12, ols=50, obs=4 * 50 + 3 * 12 + 7), INVALID), (vol(obs=0), INVALID),
    # ... before the sizes are looked at: a bad stride on a request that is also too large
    (vol(h=1 << 19, w=1 << 22, st=(0, 0, 0, 0), oys=5), INVALID),
    # the output inside an image
    (vol(out=I1), INVALID), (vol(out=I2 + 16), INVALID), (vol(out=I1 - 4 * 100), INVALID),
    # too large: the bytes leave int64, the workgroups leave the grid
    (vol(B=2, h=1, w=1, C=1, L=2, ols=1 << 61, obs=1 << 62), TOO_LARGE),
    (vol(B=1, h=1 << 19, w=1 << 22, C=1, st=(0, 0, 0, 0), L=1), TOO_LARGE),          # 2^16 x 2^16 tiles
    (vol(B=1 << 12, h=8 << 6, w=64 << 6, C=1, st=(0, 0, 0, 0), L=8 << 8), TOO_LARGE),   # 2^12 items x 2^12 tiles x 2^8 blocks
    (vol(B=2, h=2, w=2, C=1, st=(-(1 << 62), 2, 1, 0), L=1), TOO_LARGE),             # the second item's image bytes (below the base)
]
WTA = [
    (wta(C=0), UNSUPPORTED), (wta(C=5), UNSUPPORTED), (wta(ws=6), UNSUPPORTED), (wta(ws=19), UNSUPPORTED),
    (wta(crit=3), UNSUPPORTED), (wta(C=5, L=0), UNSUPPORTED), (wta(ws=2, B=-1, disp=None), UNSUPPORTED),
    (wta(B=-1), INVALID), (wta(h=-4), INVALID), (wta(w=-8), INVALID), (wta(L=-1), INVALID),
    # an argmin over nothing: PHL_ERR_INVALID, also where nothing would be launched
    (wta(L=0), INVALID), (wta(L=0, B=0), INVALID), (wta(L=0, h=0, i1=None, disp=None), INVALID),
    (wta(B=0), OK), (wta(h=0), OK), (wta(w=0), OK), (wta(B=0, i1=None, i2=None, disp=None, cost=None), OK),
    (wta(w=0, disp=I1, cost=I2, oys=0, obs=-1), OK), (wta(h=0, B=I31, w=I31, L=I31), OK),
    (wta(i1=None), INVALID), (wta(i2=None), INVALID), (wta(disp=None), INVALID),
    (wta(oys=7), INVALID), (wta(oys=12, obs=3 * 12 + 7), INVALID), (wta(obs=0), INVALID),
    (wta(h=1 << 19, w=1 << 22, st=(0, 0, 0, 0), oys=5), INVALID),
    # disp_dev or cost_dev inside an image, or inside each other
    (wta(disp=I1), INVALID), (wta(cost=I2), INVALID), (wta(disp=I2 + 4 * 191), INVALID), (wta(cost=I1 - 4), INVALID),
    (wta(cost=O), INVALID), (wta(cost=O + 4 * 63), INVALID),
    (wta(B=2, h=2, w=1, C=1, L=2, oys=1 << 61, obs=1 << 62, cost=None), TOO_LARGE),
    (wta(B=1, h=1 << 19, w=1 << 22, C=1, st=(0, 0, 0, 0), L=1, cost=None), TOO_LARGE),
    (wta(B=2, h=2, w=2, C=1, st=(-(1 << 62), 2, 1, 0), L=1, cost=None), TOO_LARGE),
]


def _check(name, args, status):
    import phl

    lib = phl.load_library()
    assert getattr(lib, name)(*args, None) == status
    if status != OK:
        text = lib.phl_last_error().decode()
        assert text.startswith(name + ":"), text


@pytest.mark.parametrize("args,status", PIXEL_MAJOR, ids=[f"{i}-{c[1]}" for i, c in enumerate(PIXEL_MAJOR)])
def test_cost_volume_argument_checks(args, status):
    _check("phl_cost_volume", args, status)


@pytest.mark.parametrize("args,status", VOLUME, ids=[f"{i}-{c[1]}" for i, c in enumerate(VOLUME)])
def test_cost_volume_nchw_argument_checks(args, status):
    _check("phl_cost_volume_nchw", args, status)


@pytest.mark.parametrize("args,status", WTA, ids=[f"{i}-{c[1]}" for i, c in enumerate(WTA)])
def test_disparity_wta_argument_checks(args, status):
    _check("phl_disparity_wta", args, status)


def test_binding_checks_need_no_gpu():
    """What the binding refuses before it reaches the device."""
    import phl

    a, b = np.zeros((6, 12, 3)), np.zeros((6, 12, 3))
    for fn in (phl.cost_volume_nchw, phl.disparity_wta):
        with pytest.raises(ValueError):
            fn(a, b[:, :-1])                                            # mismatched shapes
        with pytest.raises(ValueError):
            fn(a, b[..., :2])
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 3, 6, 12), torch.zeros(1, 3, 6, 12), channels_first=True)
        with pytest.raises(ValueError):
            fn(a, b, channels_first=True)                               # [H, W, C] is not [B, C, H, W]
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 3, 6, 12), torch.zeros(2, 3, 6, 12))      # ... and the other way round
    with pytest.raises(ValueError):
        phl.cost_volume_nchw(a, b, max_disp=2, out=torch.zeros(1, 2, 6, 11))            # wrong shape
    with pytest.raises(ValueError):
        phl.cost_volume_nchw(a, b, max_disp=2, out=torch.zeros(2, 6, 12))
    with pytest.raises(ValueError):
        phl.cost_volume_nchw(a, b, max_disp=2, out=torch.zeros(1, 2, 6, 24)[..., ::2])  # x stride 2
    with pytest.raises(ValueError):
        phl.cost_volume_nchw(a, b, max_disp=2, out=torch.zeros(1, 2, 6, 12, dtype=torch.float64))
    with pytest.raises(ValueError):
        phl.disparity_wta(a, b, max_disp=0)
    with pytest.raises(ValueError):
        phl.disparity_wta(a[:, :5], b[:, :5])                           # max_disp defaults to w // 6 = 0
    assert phl.COSTVOL_NCHW_TILE == (64, 8, 8) and phl.COSTVOL_NEGATE == NEGATE


def test_planar_sweep_algorithm_is_the_negated_window_one_badness(golden_dir):
    import os

    from crf import depth
    from oracle import costvol_oracle as co

    g = np.load(os.path.join(golden_dir, "costvol_tiny_ad9.npz"))
    a, b = g["img1"], g["img2"]
    got = depth.planar_sweep_algorithm()(a, b)
    want = -depth.disparity_badness(a, b, 1, depth.AD)
    assert got.shape == a.shape[:2] + (a.shape[1] // 6,) and got.dtype == np.float64
    assert np.array_equal(got, want) and np.array_equal(got, -co.disparity_badness(a, b, 1, "AD"))
    assert np.array_equal(depth.planar_sweep_algorithm(9, depth.AD)(a, b), -g["out"])
    assert np.array_equal(depth.planar_sweep_algorithm(3, depth.SD)(a, b), -depth.disparity_badness(a, b, 3, depth.SD))
    assert callable(depth.planar_sweep_algorithm(device=True)) and callable(depth.disparity_logits_device)
    assert callable(depth.disparity_estimate_device)


def test_integer_cases_keep_every_intermediate_exact_in_fp32():
    """The precondition of the exact GPU tests.  The kernel's horizontal sums are running sums restarted every 8 columns,
    its vertical sums running sums down the 8 rows of a tile; each adds the entering element before it subtracts the
    leaving one, so an intermediate holds at most ws + 1 raw costs (horizontal) or ws + 1 rows of ws (vertical): no more
    than ``cu.running_sum_bound``.  That is below 2^24 for every case the GPU tests use, and the expected volumes are
    integers that survive float32."""
    for crit in cu.CRITS:
        for ws in cu.WINDOWS:
            assert cu.running_sum_bound(ws, cu.channels_of(ws, crit), crit) < 2 ** 24
            a, b, want = nu.instance_case(ws, crit)
            assert a.shape == (nu.B,) + cu.SHAPE + (cu.channels_of(ws, crit),) and want.shape == (nu.B,) + cu.SHAPE + (cu.MAX_DISP,)
            assert not np.array_equal(a[0], a[1]) and np.abs(a).max() <= cu.PIXEL_RANGE[crit]
            assert np.array_equal(want, np.rint(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    for ws, crit, c in cu.EDGE_INSTANCES:
        assert cu.running_sum_bound(ws, c, crit) < 2 ** 24
    h, w, ws, crit, c = nu.BLOCK_CASE
    assert cu.running_sum_bound(ws, c, crit) < 2 ** 24
    h, w, L, ws, crit, c = nu.CONSUMER_CASE
    assert cu.running_sum_bound(ws, c, crit) < 2 ** 24
    a, b = nu.tie_images()                                              # |a - b| <= 4, windows 1 and 3
    assert np.abs(a).max() == 2 and np.abs(b).max() == 2 and (3 * 3 + 3 + 1) * 4 < 2 ** 24
    # the sweep's sizes sit on both sides of the tile, and the disparity counts on both sides of the block
    import phl

    tx, ty, dc = phl.COSTVOL_NCHW_TILE
    assert nu.edge_heights(ty) == (1, 2, 7, 8, 9, 17) and nu.edge_widths(tx) == (1, 2, 3, 63, 64, 65, 129)
    assert nu.block_counts(dc) == (1, 7, 8, 9, 17, 97)


def test_tie_counts_of_the_winner_takes_all_cases():
    """The lowest-index rule is under test only where minima are tied: the counts the GPU tests rely on."""
    from oracle import costvol_oracle as co

    tied = instances = pixels = 0
    for crit in cu.CRITS:
        for ws in cu.WINDOWS:
            t = int(nu.tied_minimum(nu.instance_case(ws, crit)[2][0]).sum())
            tied, instances, pixels = tied + t, instances + (t > 0), pixels + cu.SHAPE[0] * cu.SHAPE[1]
    assert (tied, pixels, instances) == (10073, 18981, 22)
    a, b = nu.tie_images()
    h, w, L = nu.TIE_CASE
    for ws, n_tied, n_not_zero in ((1, 612, 469), (3, 272, 253)):
        vol = co.disparity_badness(a, b, ws, "AD", max_disp=L)
        t = nu.tied_minimum(vol)
        assert (int(t.sum()), int((t & (vol.argmin(-1) != 0)).sum())) == (n_tied, n_not_zero)
