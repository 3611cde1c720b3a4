"""GPU: phl_disparity_wta (csrc/phl_costvol_nchw.hip), the winner-takes-all disparity of the window sweep without the
volume.  On integer images the costs are exact, so the disparity is np.argmin of the float64 oracle at every pixel, ties
included (the smallest disparity wins); on real-valued input it is the argmin of the library's own channel-major volume
bit for bit, and the oracle's wherever the oracle's margin exceeds the fp32 error of two costs."""
import numpy as np
import pytest
import torch

import _costvol_nchw_util as nu
import _costvol_util as cu

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _wta(a, b, ws, crit, L):
    """phl.disparity_wta with the cost, of float64 numpy pairs [B, h, w, c] (planar input) -> numpy int32 / float64 [B, h, w]."""
    import phl

    disp, cost = phl.disparity_wta(nu.planar(a), nu.planar(b), max_disp=L, window_size=ws, criterion=crit, return_cost=True,
                                   channels_first=True)
    shape = ((1,) + a.shape[:2]) if a.ndim == 3 else a.shape[:3]
    assert disp.shape == shape and disp.dtype == torch.int32 and disp.is_cuda
    assert cost.shape == shape and cost.dtype == torch.float32 and cost.is_cuda
    return disp.cpu().numpy(), cost.cpu().numpy().astype(np.float64)


def _mismatch(disp, cost, want):
    """None, or a message naming the first pixel of [B, h, w] results that is not the oracle's argmin / minimum."""
    bad = np.argwhere((disp != want.argmin(-1)) | (cost != want.min(-1)))
    if not len(bad):
        return None
    i, y, x = (int(v) for v in bad[0])
    return (f"{len(bad)} of {disp.size} pixels differ, first at (item, y, x) = ({i}, {y}, {x}): got disparity {disp[i, y, x]} at cost "
            f"{cost[i, y, x]!r}, want {want[i, y, x].argmin()} at {want[i, y, x].min()!r}")


@pytest.mark.parametrize("crit", cu.CRITS)
@pytest.mark.parametrize("ws", cu.WINDOWS)
def test_every_instance_exactly(ws, crit):
    """The inputs of test_gpu_costvol_nchw.py's 27-instance test: argmin and minimum of the oracle everywhere.  Over the
    27 instances more than half of the pixels have a tied minimum (test_costvol_nchw_host.py counts them)."""
    a, b, want = nu.instance_case(ws, crit)
    disp, cost = _wta(a, b, ws, crit, cu.MAX_DISP)
    diff = _mismatch(disp, cost, want)
    assert diff is None, diff


@pytest.mark.parametrize("ws", [1, 3])
def test_ties_go_to_the_smallest_disparity(ws):
    """Integer pixels in [-2, 2], 41 disparities: 612 (window 1) and 272 (window 3) of the 703 pixels have a tied minimum,
    and in 469 and 253 of them the winner is not disparity 0."""
    from oracle import costvol_oracle as co

    a, b = nu.tie_images()
    want = co.disparity_badness(a, b, ws, "AD", max_disp=nu.TIE_CASE[2])
    assert int(nu.tied_minimum(want).sum()) == {1: 612, 3: 272}[ws]
    disp, cost = _wta(a, b, ws, "AD", nu.TIE_CASE[2])
    diff = _mismatch(disp, cost, want[None])
    assert diff is None, diff
    import phl

    plain = phl.disparity_wta(a, b, max_disp=nu.TIE_CASE[2], window_size=ws)          # interleaved numpy, no cost
    assert plain.shape == (1,) + a.shape[:2] and np.array_equal(plain.cpu().numpy(), disp)


def test_tile_and_reflect_seams_exactly():
    """The (h, w) sweep of the volume's seam test at (window 9, AD, 3 channels), 33 disparities."""
    import phl

    ws, crit, c = cu.EDGE_INSTANCES[0]
    assert (ws, crit, c) == (9, "AD", 3)
    tx, ty, _ = phl.COSTVOL_NCHW_TILE
    bad = []
    for h in nu.edge_heights(ty):
        for w in nu.edge_widths(tx):
            a, b, want = nu.edge_case(ws, crit, c, h, w)
            diff = _mismatch(*_wta(a, b, ws, crit, nu.EDGE_L), want[None])
            if diff:
                bad.append(f"(h, w) = ({h}, {w}): {diff}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("L", nu.block_counts(8, volume=False))
def test_disparity_blocks_batch_and_strided_output(L):
    """Disparity counts around the block the kernel walks, two planar items; and through the C ABI into strided views of
    sentinel-filled buffers, one float off the 16-byte grid: the same values, nothing else touched."""
    import phl

    assert nu.block_counts(phl.COSTVOL_NCHW_TILE[2], volume=False) == nu.block_counts(8, volume=False)
    h, w, ws, crit, _ = nu.BLOCK_CASE
    a, b, want = nu.block_case(L)
    disp, cost = _wta(a, b, ws, crit, L)
    diff = _mismatch(disp, cost, want)
    assert diff is None, diff
    dbuf = torch.full((nu.B + 1, h + 3, w + 7), -7, dtype=torch.int32, device="cuda")
    cbuf = torch.full((nu.B + 1, h + 3, w + 7), float("nan"), device="cuda")
    dview, cview = dbuf[:nu.B, :h, 1:1 + w], cbuf[:nu.B, :h, 1:1 + w]
    assert dview.data_ptr() % 16 == 4 and dview.stride(0) > h * dview.stride(1) > h * w
    nu.wta_into(dview, cview, nu.planar(a).float().cuda(), nu.planar(b).float().cuda(), L, ws, crit)
    assert np.array_equal(dview.cpu().numpy(), disp) and np.array_equal(cview.cpu().numpy().astype(np.float64), cost)
    mask = torch.ones_like(dbuf, dtype=torch.bool)
    mask[:nu.B, :h, 1:1 + w] = False
    assert bool((dbuf[mask] == -7).all()) and bool(torch.isnan(cbuf[mask]).all())


def _real_pair():
    rng = np.random.default_rng(37 * 1000 + 53)
    return rng.random((37, 53, 3)), rng.random((37, 53, 3))


def test_real_valued_input_is_the_argmin_of_the_librarys_volume_and_of_the_oracle():
    """The uniform-random 37x53x3 pair of test_random_shapes_against_oracle, window 9, AD, 20 disparities.  Against the
    library's own channel-major volume: equal at every pixel, the cost bit for bit (the two kernels share their
    arithmetic).  Against the float64 oracle: equal wherever the oracle's margin between best and second best exceeds
    2 * TOL * max|volume| -- both candidates are within TOL * max of their float64 values, so their order cannot flip
    there; that condition may leave out at most 1 % of the pixels (the oracle alone leaves out 5 of 1,961)."""
    import phl
    from oracle import costvol_oracle as co

    a, b = _real_pair()
    ws, L = 9, 20
    ta, tb = torch.from_numpy(a).float().cuda(), torch.from_numpy(b).float().cuda()
    disp, cost = phl.disparity_wta(ta, tb, max_disp=L, window_size=ws, return_cost=True)
    vol = phl.cost_volume_nchw(ta, tb, max_disp=L, window_size=ws)
    assert np.array_equal(disp[0].cpu().numpy(), vol[0].cpu().numpy().argmin(0))
    assert torch.equal(nu.bits(cost), nu.bits(vol.min(1).values))
    want = co.disparity_badness(a, b, ws, "AD", max_disp=L)
    srt = np.sort(want, -1)
    clear = (srt[..., 1] - srt[..., 0]) > 2 * TOL * np.abs(want).max()
    left_out = int((~clear).sum())
    print(f"[measured] winner-takes-all vs the float64 oracle: {left_out} of {clear.size} pixels inside the margin; "
          f"{int((disp[0].cpu().numpy() != want.argmin(-1)).sum())} pixels differ in all")
    assert left_out <= 0.01 * clear.size
    assert np.array_equal(disp[0].cpu().numpy()[clear], want.argmin(-1)[clear])
    assert float(np.abs(cost[0].cpu().numpy() - want.min(-1)).max()) <= TOL * np.abs(want).max()


def test_a_known_shift_is_found():
    """right = left shifted by 7: every pixel of columns 11..91 gets disparity 7, as the oracle gives, and none of them
    is inside the margin."""
    import phl
    from oracle import costvol_oracle as co

    rng = np.random.default_rng(11)
    left = rng.random((40, 96, 3))
    right = np.zeros_like(left)
    right[:, :89] = left[:, 7:]
    ws, L = 9, 16
    want = co.disparity_badness(left, right, ws, "AD", max_disp=L)
    cols = slice(11, 92)
    assert bool((want.argmin(-1)[:, cols] == 7).all())
    srt = np.sort(want, -1)
    assert bool(((srt[..., 1] - srt[..., 0]) > 2 * TOL * np.abs(want).max())[:, cols].all())
    disp = phl.disparity_wta(left, right, max_disp=L, window_size=ws)
    assert bool((disp[0, :, cols] == 7).all())
    from crf import depth

    est = depth.disparity_estimate_device(left, right, ws, depth.AD, L)
    assert est.shape == (40, 96) and est.dtype == torch.int32 and torch.equal(est, disp[0])
