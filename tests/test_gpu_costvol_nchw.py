"""GPU: phl_cost_volume_nchw (csrc/phl_costvol_nchw.hip), the cost volume written channel-major [B, L, H, W].  On the small
integer images of tests/_costvol_util.py fp32 is exact (test_costvol_nchw_host.py holds the precondition), so every
(window, criterion) instance, the tile, reflect and disparity-block seams, the strided output and the image layouts are
compared by value or bit for bit; real-valued input is held to the suite's 2e-5 of the volume's largest magnitude."""
import glob
import os

import numpy as np
import pytest
import torch

import _costvol_nchw_util as nu
import _costvol_util as cu

pytestmark = pytest.mark.gpu
TOL = 2e-5


def scaled_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def _volume(a, b, ws, crit, L, **kw):
    """phl.cost_volume_nchw of float64 numpy pairs [B, h, w, c] (or one pair [h, w, c]) -> device tensor [B, L, h, w]."""
    import phl

    Bn, h, w = (1,) + a.shape[:2] if a.ndim == 3 else a.shape[:3]
    E = phl.cost_volume_nchw(nu.planar(a), nu.planar(b), max_disp=L, window_size=ws, criterion=crit, channels_first=True, **kw)
    assert E.shape == (Bn, L, h, w) and E.dtype == torch.float32 and E.is_cuda and E.is_contiguous()
    return E


@pytest.mark.parametrize("crit", cu.CRITS)
@pytest.mark.parametrize("ws", cu.WINDOWS)
def test_every_instance_exactly(ws, crit):
    """All 27 (window, criterion) kernels, 1..4 channels under each criterion, two items, on a shape ragged in x, y and
    disparity that reads the zero padding left of the image; odd radii negated.  The same call again: the same bytes."""
    a, b, want = nu.instance_case(ws, crit)
    negate = (ws // 2) % 2 == 1
    first = _volume(a, b, ws, crit, cu.MAX_DISP, negate=negate)
    diff = nu.first_difference(nu.to_hwl(first), -want if negate else want)
    assert diff is None, diff
    again = _volume(a, b, ws, crit, cu.MAX_DISP, negate=negate)
    assert first.data_ptr() != again.data_ptr() and torch.equal(nu.bits(first), nu.bits(again))


def test_negated_zero_cost_is_minus_zero():
    """The reference's logits are -1 * cost: a cost of exactly 0 becomes -0.0."""
    import phl

    a = np.ones((3, 5, 2))
    E = phl.cost_volume_nchw(a, a, max_disp=1, window_size=3, negate=True)
    assert torch.equal(nu.bits(E), torch.full((1, 1, 3, 5), -2 ** 31, dtype=torch.int32, device="cuda"))
    assert int(nu.bits(phl.cost_volume_nchw(a, a, max_disp=1, window_size=3)).abs().max()) == 0


@pytest.mark.parametrize("ws,crit,c", cu.EDGE_INSTANCES)
def test_tile_and_reflect_seams_exactly(ws, crit, c):
    """h and w on both sides of the tile and down to 1 (a window of 17 then folds many times on both axes); the odd widths
    put every second row off the 16-byte grid, the widths below 4 leave no room for a 16-byte store."""
    import phl

    tx, ty, _ = phl.COSTVOL_NCHW_TILE
    bad = []
    for h in nu.edge_heights(ty):
        for w in nu.edge_widths(tx):
            a, b, want = nu.edge_case(ws, crit, c, h, w)
            diff = cu.first_difference(nu.to_hwl(_volume(a, b, ws, crit, nu.EDGE_L))[0], want)
            if diff:
                bad.append(f"(h, w) = ({h}, {w}): {diff}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("L", nu.block_counts(8))
def test_disparity_blocks_and_strided_output(L):
    """Disparity counts around the block, two items, exactly; and written into a view of a NaN-filled buffer whose batch,
    label and row strides all exceed the extents and whose first element is one float off the 16-byte grid: the same
    bytes, and nothing else touched."""
    import phl

    dc = phl.COSTVOL_NCHW_TILE[2]
    assert nu.block_counts(dc) == nu.block_counts(8)
    h, w, ws, crit, _ = nu.BLOCK_CASE
    a, b, want = nu.block_case(L)
    first = _volume(a, b, ws, crit, L)
    diff = nu.first_difference(nu.to_hwl(first), want)
    assert diff is None, diff
    if L in (dc + 1, 2 * dc + 1):
        buf = torch.full((nu.B + 1, L + 2, h + 3, w + 7), float("nan"), device="cuda")
        view = buf[:nu.B, :L, :h, 1:1 + w]
        assert view.data_ptr() % 16 == 4 and view.stride(0) > L * view.stride(1) > L * h * view.stride(2) > L * h * w
        ret = phl.cost_volume_nchw(nu.planar(a), nu.planar(b), max_disp=L, window_size=ws, criterion=crit, channels_first=True,
                                   out=view)
        assert ret.data_ptr() == view.data_ptr() and torch.equal(nu.bits(view), nu.bits(first))
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:nu.B, :L, :h, 1:1 + w] = False
        assert bool(torch.isnan(buf[mask]).all()) and int(mask.sum()) == buf.numel() - first.numel()


def test_image_layouts_give_the_same_bytes_without_a_copy():
    """Interleaved [H, W, C], planar [B, C, H, W] and non-contiguous views of each: the same bytes.  fp32 CUDA inputs are
    read in place -- the library call gets the data pointers of the views it was handed, whose storage is larger than
    the view."""
    import phl

    a, b = cu.int_images(19, 37, 3, "AD", seed=7)
    kw = dict(max_disp=12, window_size=5)
    ta, tb = (torch.from_numpy(v).float().cuda() for v in (a, b))
    ref = phl.cost_volume_nchw(a, b, **kw)                                        # float64 numpy: converted
    assert ref.shape == (1, 12, 19, 37)
    from oracle import costvol_oracle as co

    assert cu.first_difference(nu.to_hwl(ref)[0], co.disparity_badness(a, b, 5, "AD", max_disp=12)) is None

    seen = []
    lib = phl.load_library()
    real = lib.phl_cost_volume_nchw

    def spy(*args):
        seen.append((args[0].value, args[1].value))
        return real(*args)

    def run(x, y, **more):
        seen.clear()
        lib.phl_cost_volume_nchw = spy
        try:
            out = phl.cost_volume_nchw(x, y, **kw, **more)
        finally:
            lib.phl_cost_volume_nchw = real
        assert seen == [(x.data_ptr(), y.data_ptr())], "an fp32 CUDA image was copied"
        return out

    # interleaved, contiguous
    assert torch.equal(nu.bits(run(ta, tb)), nu.bits(ref))
    # interleaved, a strided column slice of a wider image
    wa, wb = (torch.repeat_interleave(v, 2, dim=1) for v in (ta, tb))
    sa, sb = wa[:, ::2], wb[:, ::2]
    assert not sa.is_contiguous() and sa.untyped_storage().nbytes() > sa.numel() * 4
    assert torch.equal(nu.bits(run(sa, sb)), nu.bits(ref))
    # planar [B, C, H, W], contiguous
    pa, pb = (v.permute(2, 0, 1)[None].contiguous() for v in (ta, tb))
    assert torch.equal(nu.bits(run(pa, pb, channels_first=True)), nu.bits(ref))
    # planar as a permuted view of the interleaved tensor, and planes cut out of a taller, wider, deeper tensor
    va, vb = (v[None].permute(0, 3, 1, 2) for v in (ta, tb))
    assert not va.is_contiguous() and torch.equal(nu.bits(run(va, vb, channels_first=True)), nu.bits(ref))
    big_a, big_b = (torch.full((2, 5, 23, 41), float("nan"), device="cuda") for _ in range(2))
    big_a[1, 1:4, 2:21, 3:40], big_b[1, 1:4, 2:21, 3:40] = pa[0], pb[0]
    ca, cb = big_a[1:, 1:4, 2:21, 3:40], big_b[1:, 1:4, 2:21, 3:40]
    assert ca.untyped_storage().nbytes() > ca.numel() * 4
    assert torch.equal(nu.bits(run(ca, cb, channels_first=True)), nu.bits(ref))
    # a grayscale [H, W] pair = the same data with a trailing axis of 1
    g = phl.cost_volume_nchw(a[..., 0], b[..., 0], **kw)
    assert g.shape == (1, 12, 19, 37) and torch.equal(nu.bits(g), nu.bits(phl.cost_volume_nchw(a[..., :1], b[..., :1], **kw)))
    # differing strides: img2 is copied into img1's layout, the result is the same
    seen.clear()
    assert torch.equal(nu.bits(phl.cost_volume_nchw(sa, tb, **kw)), nu.bits(ref))
    assert torch.equal(nu.bits(phl.cost_volume_nchw(va, pb, channels_first=True, **kw)), nu.bits(ref))


def test_goldens_from_the_reference(golden_dir):
    import phl

    files = sorted(glob.glob(os.path.join(golden_dir, "costvol_*.npz")))
    assert len(files) >= 5
    for f in files:
        g = np.load(f)
        h, w, L = g["out"].shape
        E = phl.cost_volume_nchw(g["img1"], g["img2"], window_size=int(g["window"]), criterion=str(g["criterion"]))
        assert E.shape == (1, L, h, w)
        assert scaled_err(nu.to_hwl(E)[0], g["out"]) <= TOL, f
        logits = phl.cost_volume_nchw(g["img1"], g["img2"], window_size=int(g["window"]), criterion=str(g["criterion"]), negate=True)
        assert torch.equal(logits, -E)


@pytest.mark.parametrize("crit", cu.CRITS)
def test_normalized_signed_images_against_oracle(crit):
    from crf import depth
    from oracle import costvol_oracle as co

    rng = np.random.default_rng(cu.CRITS.index(crit))
    a, b = (depth.normalized(rng.standard_normal((37, 53, 3))) for _ in range(2))
    want = co.disparity_badness(a, b, 9, crit, max_disp=20)
    if crit == "nprod":
        assert want.min() < 0 < want.max()
    assert scaled_err(nu.to_hwl(_volume(a, b, 9, crit, 20))[0], want) <= TOL


def test_high_dynamic_range_image():
    """The case of test_gpu_costvol.py: left half of both images 255 times brighter than the right half, asserted at the
    suite's tolerance of the whole volume's maximum.  Printed, not asserted: the error inside the dark half relative to the
    dark half's own maximum, and over the columns whose windows and disparities stay in the dark half (x >= 45).  The
    horizontal running sums restart every 8 columns here, so only the segment x = 40..47 starts on bright columns; the
    segments from x = 48 on never see one.  Measured on an MI355X: whole volume 4.2e-7, dark half 4.2e-7, x = 45..47 1.3e-5,
    x = 48..63 3.0e-7."""
    from oracle import costvol_oracle as co

    h, w, ws, L = 32, 64, 9, 10
    rng = np.random.default_rng(5)
    a, b = rng.random((h, w, 3)), rng.random((h, w, 3))
    a[:, :w // 2] *= 255
    b[:, :w // 2] *= 255
    want = co.disparity_badness(a, b, ws, "AD", max_disp=L)
    got = nu.to_hwl(_volume(a, b, ws, "AD", L))[0]
    x_clear = w // 2 + ws // 2 + L - 1
    half = scaled_err(got[:, w // 2:], want[:, w // 2:])
    seam = scaled_err(got[:, x_clear:48], want[:, x_clear:48])
    clean = scaled_err(got[:, 48:], want[:, 48:])
    print(f"[measured] channel-major cost volume, left half x255: whole volume {scaled_err(got, want):.2e}; dark half vs its own "
          f"maximum {half:.2e}; dark-only windows x = {x_clear}..47 {seam:.2e}, x = 48..63 {clean:.2e}")
    assert scaled_err(got, want) <= TOL


def test_consumer_gets_the_same_logits_as_the_old_route():
    """CRFasRNN's default W on the new logits and on the same logits built from the pixel-major volume: equal bit for bit,
    as are the logits themselves."""
    import phl
    from crf import depth
    from crf.crf_module import CRFasRNN, charb

    h, w, L, ws, crit, c = nu.CONSUMER_CASE
    a, b = cu.int_images(h, w, c, crit, seed=6)
    ta, tb = (torch.from_numpy(v).float().cuda() for v in (a, b))
    new = depth.disparity_logits_device(ta, tb, ws, depth.AD, L)
    old = (-phl.cost_volume(ta, tb, max_disp=L, window_size=ws, criterion=crit)).reshape(h, w, L).permute(2, 0, 1)[None].contiguous()
    assert new.shape == (1, L, h, w) and torch.equal(nu.bits(new), nu.bits(old))
    assert L == w // 6 and torch.equal(nu.bits(depth.planar_sweep_algorithm(ws, depth.AD, device=True)(ta, tb)), nu.bits(new))
    net = CRFasRNN(charb(.05), niters=2, r=2, eps=1e-2, gchannels=3).cuda()
    img = (ta / 255).permute(2, 0, 1)[None].contiguous()
    with torch.no_grad():
        got, want = net.expected_depth(img, new), net.expected_depth(img, old)
    assert got.shape == (1, 1, h, w) and bool(torch.isfinite(got).all()) and torch.equal(nu.bits(got), nu.bits(want))
