"""GPU: phl_cost_volume (csrc/phl_costvol.hip) against the reference's own outputs (goldens) and against
the float64 numpy oracle on shapes the goldens do not cover.  fp32 on the device vs float64 in the
reference: asserted at 2e-5 of the volume's largest value (north-star tolerance is 1e-4).  On small integer images fp32 is
exact, and every (window, criterion) instance, the tile, reflect and disparity-block edges and the strided output are
compared bit for bit (tests/_costvol_util.py)."""
import glob
import os

import numpy as np
import pytest
import torch

import _costvol_util as cu

pytestmark = pytest.mark.gpu
TOL = 2e-5


def scaled_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def test_goldens_from_the_reference(golden_dir):
    import phl

    files = sorted(glob.glob(os.path.join(golden_dir, "costvol_*.npz")))
    assert len(files) >= 5
    for f in files:
        g = np.load(f)
        h, w, L = g["out"].shape
        E = phl.cost_volume(g["img1"], g["img2"], window_size=int(g["window"]), criterion=str(g["criterion"]))
        assert E.shape == (h * w, L) and E.dtype == torch.float32 and E.is_cuda
        assert scaled_err(E.cpu().numpy().reshape(h, w, L).astype(np.float64), g["out"]) <= TOL, f


@pytest.mark.parametrize("h,w,c,ws,L,crit", [(37, 53, 3, 9, None, "AD"), (8, 16, 3, 1, 5, "SD"), (50, 200, 3, 9, 70, "AD"),
                                             (5, 7, 2, 7, 20, "AD"), (64, 48, 1, 11, 33, "nprod"), (1, 40, 3, 3, 6, "SD"),
                                             (40, 1, 3, 5, 2, "AD"), (24, 100, 4, 13, 64, "AD")])
def test_random_shapes_against_oracle(h, w, c, ws, L, crit):
    """ragged tiles, disparities beyond the image width, windows larger than the image, 1..4 channels,
    disparity counts off the 32-wide block."""
    import phl
    from oracle import costvol_oracle as co

    rng = np.random.default_rng(h * 1000 + w)
    a, b = rng.random((h, w, c)), rng.random((h, w, c))
    want = co.disparity_badness(a, b, ws, crit, max_disp=L)
    got = phl.cost_volume(torch.from_numpy(a), torch.from_numpy(b).cuda(), max_disp=L, window_size=ws, criterion=crit)
    assert got.shape == (h * w, want.shape[2])
    assert scaled_err(got.cpu().numpy().reshape(want.shape).astype(np.float64), want) <= TOL


def test_errors_and_device_entry_point():
    import phl
    from crf import depth

    rng = np.random.default_rng(1)
    a, b = rng.random((20, 60, 3)), rng.random((20, 60, 3))
    with pytest.raises(phl.PhlError) as e:
        phl.cost_volume(a, b, window_size=4)
    assert e.value.status == 7                      # PHL_ERR_UNSUPPORTED: even window
    with pytest.raises(phl.PhlError):
        phl.cost_volume(rng.random((4, 8, 5)), rng.random((4, 8, 5)))      # 5 channels
    with pytest.raises(ValueError):
        phl.cost_volume(a, b[:, :-1])
    assert phl.cost_volume(a, b, max_disp=0).shape == (1200, 0)
    E0 = depth.disparity_energy_device(a, b)        # window 9, AD, L = w // 6: the notebook's call
    want = depth.disparity_badness(a, b, 9, depth.AD)
    assert scaled_err(E0.cpu().numpy().reshape(want.shape).astype(np.float64), want) <= TOL
    # winner-takes-all disparity agrees wherever the float64 margin exceeds the fp32 error
    srt = np.sort(want, -1)
    clear = (srt[..., 1] - srt[..., 0]) > 1e-4 * want.max()
    assert np.array_equal(E0.argmin(1).cpu().numpy().reshape(20, 60)[clear], want.argmin(-1)[clear])
    # strided output: a column block of a wider E_0 buffer
    big = torch.zeros((1200, 32), device="cuda")
    phl.cost_volume(a, b, out=big[:, 8:18])
    assert torch.equal(big[:, 8:18], E0) and float(big[:, :8].abs().sum()) == 0.0 and float(big[:, 18:].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------
# Exact tests: on the integer images of tests/_costvol_util.py fp32 computes every sum without rounding
# (test_costvol_cpu.py checks that precondition), so the kernel equals the float64 oracle bit for bit.
def _volume(a, b, ws, crit, L, **kw):
    """phl.cost_volume of two float64 numpy images as a float64 [h, w, L] array."""
    import phl

    h, w = a.shape[:2]
    E = phl.cost_volume(torch.from_numpy(a), torch.from_numpy(b), max_disp=L, window_size=ws, criterion=crit, **kw)
    assert E.shape == (h * w, L) and E.dtype == torch.float32
    return E.cpu().numpy().reshape(h, w, L).astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("crit", cu.CRITS)
@pytest.mark.parametrize("ws", cu.WINDOWS)
def test_every_instance_exactly(ws, crit):
    """All 27 (window, criterion) kernels the host dispatch builds, 1..4 channels under each criterion, on a shape that is
    ragged in x, y and disparity, spans two disparity blocks and reads the zero padding left of the image."""
    from oracle import costvol_oracle as co

    (h, w), L = cu.SHAPE, cu.MAX_DISP
    a, b = cu.int_images(h, w, cu.channels_of(ws, crit), crit, seed=ws)
    diff = cu.first_difference(_volume(a, b, ws, crit, L), co.disparity_badness(a, b, ws, crit, max_disp=L))
    assert diff is None, diff


@pytest.mark.parametrize("ws,crit,c", cu.EDGE_INSTANCES)
def test_tile_and_reflect_edges_exactly(ws, crit, c):
    """h and w on both sides of the 16-pixel tile and down to 1: at window 17 the small sizes take the general (%) branch
    of reflect() through several folds on both axes.  The reference is the oracle, except at an axis of length 2 under
    window 17, where scipy's border is undefined and the rule is summed explicitly (cu.reference_volume)."""
    L, bad = 33, []
    for h in cu.EDGE_SIZES:
        for w in cu.EDGE_SIZES:
            a, b = cu.int_images(h, w, c, crit, seed=100 * h + w)
            diff = cu.first_difference(_volume(a, b, ws, crit, L), cu.reference_volume(a, b, ws, crit, L))
            if diff:
                bad.append(f"(h, w) = ({h}, {w}): {diff}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 65, 97])
def test_disparity_block_edges_and_strided_output(L):
    """Disparity counts around the 32-wide block, exactly; the same call again gives the same bytes; and written into a
    column block of a wider buffer it gives the same bytes and touches nothing else (a NaN sentinel around the block,
    which starts off the 32-disparity grid and ends in a partial block)."""
    import phl
    from oracle import costvol_oracle as co

    h, w, ws, crit = 17, 40, 5, "SD"
    a, b = cu.int_images(h, w, 3, crit, seed=L)
    diff = cu.first_difference(_volume(a, b, ws, crit, L), co.disparity_badness(a, b, ws, crit, max_disp=L))
    assert diff is None, diff
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    first = phl.cost_volume(ta, tb, max_disp=L, window_size=ws, criterion=crit)
    again = phl.cost_volume(ta, tb, max_disp=L, window_size=ws, criterion=crit)
    assert first.data_ptr() != again.data_ptr() and torch.equal(_bits(first), _bits(again))
    if L in (33, 65):
        buf = torch.full((h * w, 128), float("nan"), device="cuda")
        ret = phl.cost_volume(ta, tb, max_disp=L, window_size=ws, criterion=crit, out=buf[:, 8:8 + L])
        assert ret.data_ptr() == buf[:, 8:].data_ptr()
        assert torch.equal(_bits(buf[:, 8:8 + L]), _bits(first))
        assert bool(torch.isnan(buf[:, :8]).all()) and bool(torch.isnan(buf[:, 8 + L:]).all())


# ---------------------------------------------------------------------------------------------
# Real-valued signed inputs: what the callers pass (examples/stereo_crf.py normalises both images to zero mean).
@pytest.mark.parametrize("crit", cu.CRITS)
def test_normalized_signed_images_against_oracle(crit):
    from crf import depth
    from oracle import costvol_oracle as co

    rng = np.random.default_rng(cu.CRITS.index(crit))
    a, b = (depth.normalized(rng.standard_normal((37, 53, 3))) for _ in range(2))
    assert a.min() < 0 < a.max() and b.min() < 0 < b.max()
    want = co.disparity_badness(a, b, 9, crit, max_disp=20)
    if crit == "nprod":
        assert want.min() < 0 < want.max()          # the sign of the volume is part of what is compared
    assert scaled_err(_volume(a, b, 9, crit, 20), want) <= TOL


def test_high_dynamic_range_image():
    """Left half of both images 255 times brighter than the right half.  Asserted at the suite's tolerance (of the whole
    volume's maximum).  Printed, not asserted: the error inside the dark half relative to the dark half's own maximum --
    over the whole half, whose first columns have windows that reach into the bright half, and over the columns whose
    windows and disparities stay in the dark half (x >= 45: the tile x = 32..47 starts its running sums on bright columns
    and carries their rounding into x = 45..47, the tile x = 48..63 restarts on dark columns only).  Measured on an
    MI355X: whole volume 4.7e-7, dark half 4.2e-7, x = 45..47 2.4e-5, x = 48..63 4.5e-7."""
    from oracle import costvol_oracle as co

    h, w, ws, L = 32, 64, 9, 10
    rng = np.random.default_rng(5)
    a, b = rng.random((h, w, 3)), rng.random((h, w, 3))
    a[:, :w // 2] *= 255
    b[:, :w // 2] *= 255
    want = co.disparity_badness(a, b, ws, "AD", max_disp=L)
    got = _volume(a, b, ws, "AD", L)
    x_clear = w // 2 + ws // 2 + L - 1              # first column whose windows, at every disparity, lie in the dark half
    half = scaled_err(got[:, w // 2:], want[:, w // 2:])
    seam_tile = scaled_err(got[:, x_clear:48], want[:, x_clear:48])
    clean_tile = scaled_err(got[:, 48:], want[:, 48:])
    print(f"[measured] cost volume, left half x255: whole volume {scaled_err(got, want):.2e}; dark half vs its own maximum "
          f"{half:.2e}; dark-only windows x = {x_clear}..47 (tile shared with bright columns) {seam_tile:.2e}, "
          f"x = 48..63 (tile of dark columns only) {clean_tile:.2e}")
    assert scaled_err(got, want) <= TOL


# ---------------------------------------------------------------------------------------------
# The binding: phl.cost_volume's input forms and phl_cost_volume's rejections.
def test_input_forms_give_the_same_bits():
    import phl
    from crf import depth

    a, b = cu.int_images(19, 37, 3, "AD", seed=7)
    kw = dict(max_disp=12, window_size=5)
    ref = phl.cost_volume(a, b, **kw)
    # 2-D grayscale pair = the same data with a trailing axis of 1
    g1 = phl.cost_volume(a[..., 0], b[..., 0], **kw)
    assert g1.shape == (19 * 37, 12) and torch.equal(_bits(g1), _bits(phl.cost_volume(a[..., :1].copy(), b[..., :1].copy(), **kw)))
    # non-contiguous inputs = their contiguous copies: numpy views with a negative stride (a mirrored image, reversed
    # channels), a strided torch slice, a channel-first tensor permuted to [h, w, c]
    for fa, fb in ((a[:, ::-1], b[:, ::-1]), (a[..., ::-1], b[..., ::-1])):
        assert not fa.flags.c_contiguous
        assert torch.equal(_bits(phl.cost_volume(fa, fb, **kw)), _bits(phl.cost_volume(fa.copy(), fb.copy(), **kw)))
    assert torch.equal(_bits(phl.cost_volume(a[:, ::-1], b[:, ::-1], **kw)),
                       _bits(phl.cost_volume(torch.flip(torch.from_numpy(a), [1]), torch.flip(torch.from_numpy(b), [1]), **kw)))
    wa, wb = (torch.from_numpy(np.repeat(v, 2, axis=1)).cuda() for v in (a, b))
    sa, sb = wa[:, ::2], wb[:, ::2]
    assert not sa.is_contiguous() and torch.equal(_bits(phl.cost_volume(sa, sb, **kw)), _bits(ref))
    ca, cb = (torch.from_numpy(np.ascontiguousarray(v.transpose(2, 0, 1))).cuda().permute(1, 2, 0) for v in (a, b))
    assert not ca.is_contiguous() and torch.equal(_bits(phl.cost_volume(ca, cb, **kw)), _bits(ref))
    # a callable criterion (the reference's calling convention) = its name
    sd = phl.cost_volume(a, b, criterion="SD", **kw)
    assert torch.equal(_bits(phl.cost_volume(a, b, criterion=depth.SD, **kw)), _bits(sd))
    assert torch.equal(_bits(depth.disparity_energy_device(a, b, 5, depth.SD, 12)), _bits(sd))
    assert not torch.equal(sd, ref)


def test_rejections_launch_nothing():
    """phl_cost_volume turns each of these away in its argument tests, before any launch: windows outside 1..17 and
    channel counts outside 1..4 are PHL_ERR_UNSUPPORTED (7), and zero disparities return at once."""
    import phl

    a, b = cu.int_images(4, 8, 3, "AD", seed=1)
    for ws in (19, 0, -3):
        with pytest.raises(phl.PhlError) as e:
            phl.cost_volume(a, b, window_size=ws)
        assert e.value.status == 7, ws
    with pytest.raises(phl.PhlError) as e:
        phl.cost_volume(np.zeros((4, 8, 0)), np.zeros((4, 8, 0)))
    assert e.value.status == 7
    buf = torch.full((32, 128), float("nan"), device="cuda")
    ret = phl.cost_volume(a, b, max_disp=0, out=buf[:, 8:8])
    assert ret.shape == (32, 0) and bool(torch.isnan(buf).all())
    torch.cuda.synchronize()
