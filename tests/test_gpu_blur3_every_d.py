"""The three-axes-per-pass blur (k_blur3 and the line lists of phl_rebuild_table_and_neighbors) where test_gpu_blur3.py
does not reach: every d up to 16 (two to five triples, every tail layout of triples and pairs), long lines in the LAST
group, rows off the 16-byte grid and buffers off it, other item sizes (PHL_BLUR3_ITEM, read at build) and the switch
(PHL_BLUR_TRIPLES) in fresh processes, and the lattices on which the route must be declined (ghost vertices, restricted
blur rows).

Two references, both bitwise: Lattice.blur_axis axis by axis (the same library, another kernel) and blur_model_f32
(tests/_blur3_util.py), numpy float32 on Lattice.neighbors(), which tests/test_blur3_model_cpu.py pins to the CPU oracle's
blur.  The only tolerances are the default-path bounds of test_gpu_lattice_parity.test_filter_stages_match_oracle, copied
for the stage test at wide rows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _blur3_util import (INFO_FIELDS, RANDOM_SCALE, WIDTHS3, _axis_by_axis, _bits, _check_line_lists, _features, blur_model_f32,
                         check_item_starts, expected_groups, last_group_axis, longest_line, route_results)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def phl():
    import phl as _phl

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _phl.load_library()
    return _phl


def _make(kind, d):
    if kind == "last_axis_ramp":
        return _features("axis_ramp", d, c=last_group_axis(d), n=2048)
    if kind == "iid":
        return _features("iid", d, n=1500)
    return _features(kind, d)


def _check_blur(lat, widths, tag):
    """lat.blur at every width against the single-axis kernels and against the numpy model.  The blur treats every column
    alike, so one model run at the widest width serves them all."""
    rng = np.random.default_rng(7)
    wide = rng.standard_normal((lat.M, max(widths))).astype(np.float32)
    nbr = lat.neighbors()
    model = None
    for vd in widths:
        v0 = torch.from_numpy(np.ascontiguousarray(wide[:, :vd])).cuda()
        want = _axis_by_axis(lat, v0)
        if model is None:                   # (rows of `wide` are in buffer order: the model wants first-touch order)
            wide_ft = lat.to_first_touch(torch.from_numpy(wide).cuda()).cpu().numpy()
            model = lat.from_first_touch(torch.from_numpy(blur_model_f32(nbr, wide_ft)).cuda()).cpu().numpy()
        got = lat.blur(v0.clone())
        assert np.array_equal(_bits(got), _bits(want)), (tag, vd, "axis by axis")
        assert np.array_equal(_bits(got), np.ascontiguousarray(model[:, :vd]).view(np.uint32)), (tag, vd, "numpy model")


# ---- a. every d ------------------------------------------------------------------------------------------------------
CASES_A = [(kind, d) for d in range(7, 17) for kind in ("iid", "constant", "single_pixel", "axis_ramp", "last_axis_ramp")]
CASES_A += [("smooth", d) for d in (8, 11, 16)] + [("last_axis_ramp", 5), ("last_axis_ramp", 6)]
# iid features at this scale leave almost every vertex without a blur neighbour (the lists and tables are still those of the
# layout); "dense" is the same draw in the unit cube: every group has lines of 2 and 3 and a third of the neighbours exist
CASES_A += [("dense", d) for d in range(7, 17)]


@pytest.mark.parametrize("kind,d", CASES_A)
def test_every_d_against_axis_by_axis_and_the_model(phl, kind, d):
    """d = 7 ... 16: 2T+1P, 3T, 2T+2P, 3T+1P, 4T, 3T+2P, 4T+1P, 5T, 4T+2P, 5T+1P.  The ramp along the last group's axis
    puts one line of 513 vertices into the group whose lines the other inputs keep at 3 or fewer (d = 5: group 1)."""
    lat = phl.Lattice(torch.from_numpy(_make(kind, d)).cuda())
    info = lat.blur_lines()
    assert info["groups"] == expected_groups(d) >= 1
    longest = _check_line_lists(lat)
    check_item_starts(lat)
    if kind == "constant":
        assert lat.M == d + 1
    if kind == "dense":
        nbr = lat.neighbors()
        assert (nbr >= 0).mean() > 0.15 and all(longest_line(nbr[3 * g + 2]) >= 2 for g in range(info["groups"]))
    if kind == "last_axis_ramp":
        assert longest > 4 * info["item_size"]                              # items cut inside lines, in the last group
        assert longest_line(lat.neighbors()[last_group_axis(d)]) == longest   # (the long line is that group's)
    _check_blur(lat, WIDTHS3, (kind, d))


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6])
def test_low_d_against_the_model(phl, d):
    """test_gpu_blur3.py's range once against the reference from outside the library (d = 3: the pair route)."""
    lat = phl.Lattice(torch.from_numpy(_features("smooth", d)).cuda())
    assert lat.blur_lines()["groups"] == expected_groups(d)
    _check_blur(lat, (260,), ("smooth", d))


# ---- b. the stages against the oracle at rows that take the route --------------------------------------------------------
def _scaled_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


@pytest.mark.parametrize("d", [7, 8, 10, 12, 13, 16])
def test_stages_match_oracle_at_wide_rows(phl, d):
    """test_gpu_lattice_parity.test_filter_stages_match_oracle at vd = 256: its cases above d = 5 stop at 20 channels."""
    from oracle import phl_oracle as po

    n, vd = 1500, 256
    rng = np.random.default_rng(100 + n + d)
    ref = (rng.random((n, d), dtype=np.float32) * np.float32(RANDOM_SCALE[d])).astype(np.float32)
    src = rng.standard_normal((n, vd)).astype(np.float32)
    O = po.Oracle(ref)
    out_o, splat_o, blur_o = O.filter(src, stages=True)
    L = phl.Lattice(torch.from_numpy(ref).cuda())
    assert L.M == O.M and L.blur_lines()["groups"] == expected_groups(d)
    s = torch.from_numpy(src).cuda()
    ft = lambda v: L.to_first_touch(v).cpu().numpy()
    vs = L.splat(s, exact=True)
    assert np.array_equal(ft(vs).view(np.uint32), splat_o.view(np.uint32)), "splat bitwise"
    assert _scaled_err(ft(L.splat(s)), splat_o) <= 1e-5
    vb = L.blur(vs)
    assert np.array_equal(ft(vb).view(np.uint32), blur_o.view(np.uint32)), "blur bitwise"
    assert np.array_equal(L.filter(s, exact=True).cpu().numpy().view(np.uint32), out_o.view(np.uint32)), "filter bitwise"
    assert _scaled_err(L.slice(vb).cpu().numpy(), out_o) <= 1e-6        # default slice: one final multiply
    assert _scaled_err(L.filter(s).cpu().numpy(), out_o) <= 1e-5        # default (fast) path


# ---- c. rows and buffers off the 16-byte grid --------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 8])
def test_rows_off_the_grid(phl, d):
    """Odd widths one past 1, 2, 4 and 8 column blocks of the scalar-lane instantiation."""
    lat = phl.Lattice(torch.from_numpy(_features("smooth", d)).cuda())
    assert lat.blur_lines()["groups"] == expected_groups(d)
    rng = np.random.default_rng(23)
    for vd in (65, 129, 257, 513):
        v0 = torch.from_numpy(rng.standard_normal((lat.M, vd)).astype(np.float32)).cuda()
        assert np.array_equal(_bits(lat.blur(v0.clone())), _bits(_axis_by_axis(lat, v0))), (d, vd)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("d", [5, 8])
def test_buffers_off_the_grid(phl, d, which):
    """Contiguous buffers that start one float off the 16-byte grid: vd = 64 is the narrowest row the route accepts (a wave
    of scalar lanes), vd = 256 runs four column blocks of it.  which: the first ping-pong buffer, the second, both."""
    lat = phl.Lattice(torch.from_numpy(_features("smooth", d)).cuda())
    rng = np.random.default_rng(29)
    for vd in (64, 256):
        v0 = torch.from_numpy(rng.standard_normal((lat.M, vd)).astype(np.float32)).cuda()
        want = _axis_by_axis(lat, v0)
        bufs = []
        for k in range(2):
            if which == k or which == 2:
                base = torch.empty(lat.M * vd + 1, device="cuda")
                bufs.append(base[1:].view(lat.M, vd))
                assert bufs[k].data_ptr() % 16 == 4 and bufs[k].is_contiguous()
            else:
                bufs.append(torch.empty((lat.M, vd), device="cuda"))
                assert bufs[k].data_ptr() % 16 == 0
        bufs[0].copy_(v0)
        bufs[1].fill_(float("nan"))
        assert np.array_equal(_bits(lat.blur(bufs[0], scratch=bufs[1])), _bits(want)), (d, vd, which)


# ---- d. item sizes and the switch, each in a fresh process ---------------------------------------------------------------
@pytest.fixture(scope="module")
def default_route_results(phl):
    assert "PHL_BLUR3_ITEM" not in os.environ and os.environ.get("PHL_BLUR_TRIPLES", "1") != "0"
    return route_results(phl)


CHILD = (
    "import os, sys, numpy as np\n"
    "root, path = sys.argv[1], sys.argv[2]\n"
    "sys.path[:0] = [os.path.join(root, 'depth-estimation_amd'), root, os.path.join(root, 'tests')]\n"
    "import phl\n"
    "from _blur3_util import route_results\n"
    "np.savez(path, **route_results(phl))\n")


@pytest.mark.parametrize("env", [{"PHL_BLUR3_ITEM": "1"}, {"PHL_BLUR3_ITEM": "7"}, {"PHL_BLUR3_ITEM": "32"}, {"PHL_BLUR3_ITEM": "33"},
                                 {"PHL_BLUR_TRIPLES": "0"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_item_sizes_and_the_switch_in_a_fresh_process(default_route_results, tmp_path, env):
    """Both variables are read once per process.  The child checks its own line lists (_check_line_lists,
    check_item_starts) and computes what the parent computed with the default settings: every array has the same bits,
    whatever the item size and whichever route ran."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, root, path], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(path)
    want = default_route_results
    assert sorted(got.files) == sorted(want)
    for name in sorted(want):
        if not name.endswith("/info"):
            assert got[name].shape == want[name].shape and np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), (env, name)
            continue
        mine, theirs = ({k: int(x) for k, x in zip(INFO_FIELDS, z[name])} for z in (want, got))
        d = int(name[1])
        assert theirs["M"] == mine["M"] and mine["groups"] == expected_groups(d) and mine["item_size"] == 4
        item = env.get("PHL_BLUR3_ITEM")
        if item == "33":                                                    # outside 1 .. 32: no lists, the pair route
            assert (theirs["groups"], theirs["items"], theirs["item_size"]) == (0, 0, 0), (name, theirs)
            continue
        assert theirs["groups"] == mine["groups"] and theirs["longest_line"] == mine["longest_line"], (name, theirs)
        K = int(item) if item else 4
        assert theirs["item_size"] == K and theirs["items"] == (theirs["M"] + K - 1) // K
        assert 1 <= theirs["longest_item"] <= min(2 * K - 1, 64), (name, theirs)
        if item == "1":                                                     # every present neighbour is "evaluate"
            assert theirs["sliding"] == 0 and theirs["longest_item"] == 1, (name, theirs)
        if item in ("7", "32") and name == "d5_smooth/info":                # lines of mixed lengths: items longer than a bucket
            assert theirs["longest_item"] > K and theirs["sliding"] > 0, (name, theirs)
        if name == "d5_ramp/info":
            assert theirs["longest_line"] > 4 * 32


# ---- e. lattices on which the route must be declined ----------------------------------------------------------------------
def test_ghost_vertices_keep_the_pair_route(phl):
    """add_vertices with keys just outside the key range, each the axis neighbour of a vertex at the range's edge: the line
    lists are dropped (row bands keep the pair route), and the blur of the enlarged lattice, ghosts included, is the
    model's on the enlarged neighbour table."""
    d = 5
    lat = phl.Lattice(torch.from_numpy(_features("smooth", d)).cuda())
    assert lat.blur_lines()["groups"] == 2
    keys = lat.keys().astype(np.int32)
    M0 = lat.M
    edge = np.nonzero(keys[:, 0] == keys[:, 0].max())[0][:3]
    ghosts = []
    for v in edge:
        for axis in (1, 2, d):              # the minus-side neighbour along `axis`: every stored coordinate + 1, -d at `axis`
            k = keys[v] + 1
            if axis < d:
                k[axis] = keys[v][axis] - d
            ghosts.append(k)
    ghosts = np.unique(np.array(ghosts), axis=0)
    assert (ghosts[:, 0] > keys[:, 0].max()).all() and np.abs(ghosts).max() < 32767
    rows = lat.add_vertices(ghosts.astype(np.int16))
    assert lat.M == M0 + len(ghosts) and lat.M_local == M0 and sorted(rows) == list(range(M0, lat.M))
    assert lat.blur_lines() == {"groups": 0, "items": 0, "item_size": 0}
    nbr = lat.neighbors()
    assert nbr.shape == (d + 1, lat.M, 2)
    assert sum(int((nbr[axis][:M0] >= M0).sum()) for axis in (1, 2, d)) >= len(ghosts)      # local vertices read ghosts
    _check_blur(lat, WIDTHS3, "ghosts")


def test_restricted_blur_rows_keep_the_pair_route(phl):
    """set_blur_rows: the line lists stay, the route is declined while the ranges are in force (k_blur3 computes every
    row), the rows inside the ranges have the unrestricted bits, and set_blur_rows(None) brings the whole buffer back."""
    d, vd = 5, 256
    lat = phl.Lattice(torch.from_numpy(_features("smooth", d)).cuda())
    M = lat.M
    assert lat.blur_lines()["groups"] == 2 and M > 64
    v0 = torch.from_numpy(np.random.default_rng(31).standard_normal((M, vd)).astype(np.float32)).cuda()
    want = lat.blur(v0.clone())
    assert np.array_equal(_bits(want), _bits(_axis_by_axis(lat, v0)))
    ranges = np.zeros((d + 1, 3, 2), np.int64)
    ranges[:d] = [[0, M], [M, M], [M, M]]
    ranges[d] = [[M // 8, M // 4], [M // 2, M // 2], [5 * M // 8, M - 3]]
    inside = np.zeros(M, bool)
    for b, e in ranges[d]:
        inside[b:e] = True
    assert 0 < inside.sum() < M
    lat.set_blur_rows(ranges)
    assert lat.blur_lines()["groups"] == 2
    got = lat.blur(v0.clone())
    assert np.array_equal(_bits(got)[inside], _bits(want)[inside])
    # the last pass computed the listed rows only: the others still hold an earlier pass's values
    assert not np.array_equal(_bits(got)[~inside], _bits(want)[~inside])
    lat.set_blur_rows(None)
    assert np.array_equal(_bits(lat.blur(v0.clone())), _bits(want))


# ---- f. repeatability -------------------------------------------------------------------------------------------------------
def test_second_run_and_swapped_buffers_change_no_bit(phl):
    d, vd = 16, 260
    lat = phl.Lattice(torch.from_numpy(_make("last_axis_ramp", d)).cuda())
    assert lat.blur_lines()["groups"] == 5
    v0 = torch.from_numpy(np.random.default_rng(37).standard_normal((lat.M, vd)).astype(np.float32)).cuda()
    a, b = v0.clone(), torch.full_like(v0, float("nan"))
    first = lat.blur(a, scratch=b).clone()
    b.copy_(v0)                                                             # the roles of the two buffers swapped
    a.fill_(float("nan"))
    second = lat.blur(b, scratch=a).clone()
    third = lat.blur(v0.clone())
    assert np.array_equal(_bits(first), _bits(second)) and np.array_equal(_bits(first), _bits(third))
    assert np.array_equal(_bits(first), _bits(_axis_by_axis(lat, v0)))
