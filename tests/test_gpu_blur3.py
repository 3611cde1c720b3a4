"""Three lattice axes per blur pass (k_blur3: the third axis by walking lattice lines), d = 2 ... 6.

The arithmetic is axis-by-axis Jacobi with the same blur3 association as the single-axis kernel, so every check here is
bitwise: there are no tolerances.  Narrow rows (several vertices per wave) and d = 3 keep the pair route; they are in the
matrix all the same, so a change of the routing rule cannot leave a width untested.

The feature families and the check of the line lists live in tests/_blur3_util.py, shared with
tests/test_gpu_blur3_every_d.py: every d up to 16 (all tail layouts of triples and pairs), long lines in the later groups,
the numpy model of the blur as a reference from outside the library (pinned to the CPU oracle by
tests/test_blur3_model_cpu.py), other item sizes and the lattices on which the route is declined.
"""
import numpy as np
import pytest
import torch

from _blur3_util import _axis_by_axis, _axis_direction, _bits, _check_line_lists, _features, _lines_of  # noqa: F401

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
