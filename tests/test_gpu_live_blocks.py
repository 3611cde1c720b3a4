"""GPU: every device block a lattice, a build or a call takes from the block cache goes back to it
(phl_debug_live_blocks: blocks handed out and not yet given back) -- over the whole life of a lattice, after a
build that fails, and at the edge sizes."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def live_blocks():
    import phl

    gc.collect()
    return int(phl.load_library().phl_debug_live_blocks())


def test_whole_life_of_a_lattice_returns_every_block():
    """Reference-table build above the first doubling (replay, renaming, side stream), a plain and an exact filter (the
    pixel-sorted lists and the vertex order are made on first use), add_vertices with present and new keys (table and
    neighbours rebuilt), a row band cut out with its own vertices; everything closed.  Twice: the second round runs out
    of the block cache."""
    import bench
    import phl

    dev = torch.device("cuda")
    H, W = 192, 512
    feat = bench.synthetic_features(H, W, sigma_xy=3.0)
    ref = torch.from_numpy(feat.reshape(-1, 5)).to(dev)
    src = torch.from_numpy(np.random.default_rng(0).random((H * W, 3), dtype=np.float32)).to(dev)
    base = live_blocks()
    for _ in range(2):
        lat = phl.Lattice(ref, reference_table=True)
        assert lat.M > 16383                          # goes through the replay
        assert live_blocks() > base
        lat.filter(src)
        lat.filter(src, exact=True)
        r0, r1 = 64, 128
        own = np.nonzero(lat.vertices_of_pixels(r0 * W, r1 * W))[0].astype(np.int32)
        sub = lat.sub_lattice(r0 * W, r1 * W, own, len(own), torch.from_numpy(feat[r0:r1].reshape(-1, 5)).to(dev))
        assert sub.M == sub.M_local == len(own)
        sub.filter(src[r0 * W:r1 * W])
        keys = lat.keys()
        M0 = lat.M
        q = np.concatenate([keys[10:14], keys[:3] + np.int16(100), keys[50:52]])       # present, new, present
        ids = lat.add_vertices(q)
        assert lat.M == M0 + 3 and len(ids) == len(q)
        lat.filter(src)
        torch.cuda.synchronize()
        sub.close()
        lat.close()
        assert live_blocks() == base


def test_failed_build_returns_every_block():
    """Features scaled until a lattice coordinate leaves int16: an ordinary argument error (PHL_ERR_KEY_RANGE) half-way
    through the build.  Nothing stays out, and the next build is the one a build before the failure made."""
    import bench
    import phl

    dev = torch.device("cuda")
    feat = bench.synthetic_features(64, 64, sigma_xy=3.0).reshape(-1, 5)
    ref = torch.from_numpy(feat).to(dev)
    src = torch.from_numpy(np.random.default_rng(1).random((64 * 64, 4), dtype=np.float32)).to(dev)
    before = phl.Lattice(ref)
    want = before.filter(src).cpu().numpy()
    before.close()
    base = live_blocks()
    with pytest.raises(phl.PhlError) as ei:
        phl.Lattice(ref * 1e6)
    assert ei.value.status == 5                       # PHL_ERR_KEY_RANGE
    assert live_blocks() == base
    after = phl.Lattice(ref)
    got = after.filter(src).cpu().numpy()
    after.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert live_blocks() == base


@pytest.mark.parametrize("n", [0, 1, 40 * 56])
def test_edge_sizes_return_every_block(n):
    """No pixel, one pixel, and a clean-table lattice of 40x56 pixels at d = 5: build, filter 4 channels, close."""
    import phl

    dev = torch.device("cuda")
    rng = np.random.default_rng(2)
    if n == 40 * 56:
        yy, xx = np.mgrid[:40, :56].astype(np.float32)
        ref = np.stack([yy / 5, xx / 5] + [rng.random((40, 56), dtype=np.float32) * 2 for _ in range(3)], axis=-1).reshape(n, 5)
    else:
        ref = rng.random((n, 5), dtype=np.float32)
    src = torch.from_numpy(rng.random((n, 4), dtype=np.float32)).to(dev)
    base = live_blocks()
    lat = phl.Lattice(torch.from_numpy(ref).to(dev))
    out = lat.filter(src)
    assert out.shape == (n, 4) and bool(torch.isfinite(out).all())
    torch.cuda.synchronize()
    lat.close()
    assert live_blocks() == base
