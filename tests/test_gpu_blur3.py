"""Three lattice axes per blur pass (k_blur3: the third axis by walking lattice lines).

The arithmetic is axis-by-axis Jacobi with the same blur3 association as the single-axis kernel, so every check here is
bitwise: there are no tolerances.  Narrow rows (several vertices per wave) and d = 3 keep the pair route; they are in the
matrix all the same, so a change of the routing rule cannot leave a width untested.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 4 ... 512: the issue's widths (one lane group, one wave, two column blocks); 66 runs the scalar-lane kernel (rows off the
# 16-byte grid, still one wave per row) and 260 a second column block that only part of the wave works on
WIDTHS = (4, 64, 66, 128, 256, 260, 512)


@pytest.fixture(scope="module")
def phl():
    import phl as _phl

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _phl.load_library()
    return _phl


def _axis_direction(d, c):
    """A feature-space direction whose elevation is the lattice's axis-c direction (1, .., 1, -d at c, 1, .., 1): pixels
    on a ramp along it walk one lattice line of axis c."""
    from oracle import phl_oracle as po

    sf = po.scale_factors(d).astype(np.float64)
    E = np.zeros((d + 1, d))
    for k in range(d):                  # the elevation's column of feature k: +1 at 0..k, -(k+1) at k+1, times the scale
        E[: k + 1, k] = 1
        E[k + 1, k] = -(k + 1)
    E *= sf[None, :]
    a = np.ones(d + 1)
    a[c] = -d
    f = np.linalg.lstsq(E, a, rcond=None)[0]
    assert np.allclose(E @ f, a)
    return f


def _features(kind, d):
    rng = np.random.default_rng(1000 + d)
    if kind == "smooth":                # a 48 x 64 image: position over 4 px, smooth colours
        y, x = np.mgrid[0:48, 0:64].astype(np.float32)
        cols = [x / 4, y / 4] + [np.sin(x / (7 + 3 * k)) * np.cos(y / (5 + 2 * k)) * 2 + k for k in range(d - 2)]
        return np.stack(cols[:d], -1).reshape(-1, d).astype(np.float32)
    if kind == "iid":                   # almost every line has length 1
        return (rng.random((3000, d), dtype=np.float32) * 40).astype(np.float32)
    if kind == "constant":              # d + 1 vertices
        return np.full((500, d), 0.37, np.float32)
    if kind == "single_pixel":
        return np.full((1, d), 0.37, np.float32)
    if kind == "feature_ramp":          # 1 x 4096, one feature varies
        ref = np.full((4096, d), 0.37, np.float32)
        ref[:, d - 1] += np.arange(4096, dtype=np.float32) * np.float32(0.25)
        return ref
    if kind == "axis_ramp":             # 1 x 4096 along lattice axis 2: one line of ~1025 vertices per remainder
        t = np.arange(4096, dtype=np.float64) * 0.25
        return (t[:, None] * _axis_direction(d, 2)[None, :] + 0.37).astype(np.float32)
    raise AssertionError(kind)


def _axis_by_axis(lat, v0):
    a, b = v0.clone(), torch.empty_like(v0)
    for axis in range(lat.d + 1):
        lat.blur_axis(axis, a, b)
        a, b = b, a
    return a


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _lines_of(vertex, nbr_c):
    """Line id of every list entry: consecutive entries belong together iff they are mutual neighbours."""
    prev, cur = vertex[:-1], vertex[1:]
    joined = (nbr_c[prev, 1] == cur) & (nbr_c[cur, 0] == prev)
    return np.concatenate([[0], np.cumsum(~joined)]), joined


def _check_line_lists(lat):
    """Every vertex once; sliding only between consecutive mutual neighbours inside one work item; absent exactly where
    nbr[c] is -1; evaluate for everything else.  Returns the longest line over all groups."""
    info = lat.blur_lines()
    if info["groups"] == 0:
        assert info == {"groups": 0, "items": 0, "item_size": 0}
        return 0
    nbr = lat.neighbors()
    M, K = lat.M, info["item_size"]
    assert info["items"] == (M + K - 1) // K
    longest = 0
    for g in range(info["groups"]):
        c = 3 * g + 2
        vertex, minus, plus, start = lat.blur_lines(g)
        assert np.array_equal(np.sort(vertex), np.arange(M))
        assert start[0] == 0 and start[-1] == M and np.all(np.diff(start) >= 1) and np.all(np.diff(start) < 2 * K)
        is_start = np.zeros(M + 1, bool)
        is_start[start] = True
        line, joined = _lines_of(vertex, nbr[c])
        slide_minus = np.concatenate([[False], joined & ~is_start[1:M]])
        slide_plus = np.concatenate([joined & ~is_start[1:M], [False]])
        for flag, side, slide in ((minus, 0, slide_minus), (plus, 1, slide_plus)):
            absent = nbr[c][vertex, side] < 0
            assert np.array_equal(flag == 0, absent)
            assert np.array_equal(flag == 1, slide & ~absent)
            assert np.array_equal(flag == 2, ~absent & ~slide)
        # lines in the order of their first member: the starts' first-touch ids need not ascend (rows do), but every
        # line is whole and an item is cut inside a line only where that line fills the whole bucket of K entries (the
        # list's last bucket may be shorter)
        length = np.bincount(line)
        inside = 1 + np.nonzero(is_start[1:M] & joined)[0]
        assert np.all(inside % K == 0) and np.all(line[inside] == line[np.minimum(inside + K, M) - 1])
        longest = max(longest, int(length.max()))
    return longest


KINDS = ("smooth", "iid", "constant", "single_pixel", "feature_ramp", "axis_ramp")


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_blur_equals_axis_by_axis(phl, kind, d):
    lat = phl.Lattice(torch.from_numpy(_features(kind, d)).cuda())
    info = lat.blur_lines()
    assert info["groups"] == (0 if d == 3 else (d + 1) // 3 if (d + 1) % 3 != 1 else (d + 1) // 3 - 1)
    longest = _check_line_lists(lat)
    if kind == "constant":
        assert lat.M == d + 1
        assert not info["groups"] or lat.M % info["item_size"] != 0         # a ragged last item (3, 5, 6, 7 vertices)
    if kind == "axis_ramp" and info["groups"]:
        assert longest > 4 * info["item_size"]                              # items cut inside lines
    rng = np.random.default_rng(7)
    for vd in WIDTHS:
        v0 = torch.from_numpy(rng.standard_normal((lat.M, vd)).astype(np.float32)).cuda()
        want = _axis_by_axis(lat, v0)
        got = lat.blur(v0.clone())
        assert np.array_equal(_bits(got), _bits(want)), (kind, d, vd)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("d", [2, 4, 5, 6])
def test_filter_equals_stage_composition(phl, d, exact):
    """filter() end to end (its own workspace, the route blur_all picks) against splat -> single-axis blurs -> slice."""
    ref = _features("smooth", d)
    lat = phl.Lattice(torch.from_numpy(ref).cuda())
    rng = np.random.default_rng(11)
    for vd in (256, 512):
        src = torch.from_numpy(rng.random((ref.shape[0], vd), dtype=np.float32)).cuda()
        want = lat.slice(_axis_by_axis(lat, lat.splat(src, exact=exact)), exact=exact)
        got = lat.filter(src, exact=exact)
        assert np.array_equal(_bits(got), _bits(want)), (d, vd, exact)


@pytest.fixture(scope="module")
def reference_table_crop(phl):
    import bench

    feat = bench.synthetic_features(1536, 2048)[:512, :768]
    ref = np.ascontiguousarray(feat.reshape(-1, 5))
    return ref, phl.Lattice(torch.from_numpy(ref).cuda(), reference_table=True)


def test_non_mutual_links(phl, reference_table_crop):
    """The reference's table makes duplicate vertices above its first doubling, and with them links that are not
    mutual: a line must not run over one, and the neighbour is still read."""
    ref, lat = reference_table_crop
    assert lat.M == 38214
    nbr = lat.neighbors()
    one_sided = 0
    for c in (2, 5):
        for side in (0, 1):
            w = nbr[c][:, side]
            have = w >= 0
            one_sided += int((nbr[c][w[have], 1 - side] != np.nonzero(have)[0]).sum())
    assert one_sided >= 1
    _check_line_lists(lat)
    rng = np.random.default_rng(13)
    v0 = torch.from_numpy(rng.standard_normal((lat.M, 256)).astype(np.float32)).cuda()
    assert np.array_equal(_bits(lat.blur(v0.clone())), _bits(_axis_by_axis(lat, v0)))
    src = torch.from_numpy(rng.random((ref.shape[0], 256), dtype=np.float32)).cuda()
    for exact in (False, True):
        want = lat.slice(_axis_by_axis(lat, lat.splat(src, exact=exact)), exact=exact)
        assert np.array_equal(_bits(lat.filter(src, exact=exact)), _bits(want)), exact


def test_step_under_graph_capture(phl):
    ref = _features("smooth", 5)
    lat = phl.Lattice(torch.from_numpy(ref).cuda())
    assert lat.blur_lines()["groups"] == 2
    lat.reserve(256)
    x = torch.rand((ref.shape[0], 256), device="cuda")
    out = torch.empty_like(x)
    lat.filter(x, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lat.filter(x, out=out)
    x.copy_(torch.rand((ref.shape[0], 256), device="cuda"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(lat.filter(x)))
