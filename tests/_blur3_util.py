"""TEST INFRASTRUCTURE ONLY -- what the tests of the three-axes-per-pass blur share (test_gpu_blur3.py,
test_gpu_blur3_every_d.py, test_blur3_model_cpu.py): the feature families, the check of the line lists, and a model of
the blur in plain numpy float32 that test_blur3_model_cpu.py pins to the CPU oracle bit for bit.

Every comparison built on these is bitwise: the blur is axis-by-axis Jacobi with one fixed association, and every
product in it is by a power of two."""
import numpy as np

WIDTHS3 = (66, 256, 260)    # scalar lanes (rows off the 16-byte grid), one float4 column block, a ragged second block

# feature scale of the random cases per d: those of test_gpu_lattice_parity.CASES (the first case of every d there; d = 10
# and 12 are not in CASES and take d = 11's)
RANDOM_SCALE = {1: 10.0, 2: 3.0, 3: 5.0, 4: 2.5, 5: 4.0, 6: 3.0, 7: 2.0, 8: 2.0, 10: 1.5, 11: 1.5, 12: 1.5, 13: 1.0, 16: 1.0}


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


def expected_groups(d):
    """Triples of the three-axes route: d+1 = 3q + r axes go as q triples (r = 0, 2) or q-1 triples and two pairs (r = 1);
    none where that leaves no triple (d + 1 < 3, d + 1 == 4)."""
    naxes = d + 1
    if naxes < 3 or naxes == 4:
        return 0
    return naxes // 3 - 1 if naxes % 3 == 1 else naxes // 3


def last_group_axis(d):
    """The walked axis of the last triple, 3 (n3 - 1) + 2."""
    n3 = expected_groups(d)
    assert n3 >= 1
    return 3 * (n3 - 1) + 2


def _features(kind, d, c=2, n=None):
    """n: pixels of the kinds that are lists of pixels (iid 3000, dense 1500, constant 500, the ramps 4096 where not given)."""
    rng = np.random.default_rng(1000 + d)
    if kind == "smooth":                # a 48 x 64 image: position over 4 px, smooth colours
        y, x = np.mgrid[0:48, 0:64].astype(np.float32)
        cols = [x / 4, y / 4] + [np.sin(x / (7 + 3 * k)) * np.cos(y / (5 + 2 * k)) * 2 + k for k in range(d - 2)]
        return np.stack(cols[:d], -1).reshape(-1, d).astype(np.float32)
    if kind == "iid":                   # almost every line has length 1
        return (rng.random((3000 if n is None else n, d), dtype=np.float32) * 40).astype(np.float32)
    if kind == "dense":                 # a third of all neighbours present at d = 7 ... 16, lines of up to 3 in every group
        return rng.random((1500 if n is None else n, d), dtype=np.float32)
    if kind == "constant":              # d + 1 vertices
        return np.full((500 if n is None else n, d), 0.37, np.float32)
    if kind == "single_pixel":
        return np.full((1, d), 0.37, np.float32)
    n = 4096 if n is None else n
    if kind == "feature_ramp":          # 1 x n, one feature varies
        ref = np.full((n, d), 0.37, np.float32)
        ref[:, d - 1] += np.arange(n, dtype=np.float32) * np.float32(0.25)
        return ref
    if kind == "axis_ramp":             # 1 x n along lattice axis c, step 0.25: one line of ~n/4 + 1 vertices per remainder
        t = np.arange(n, dtype=np.float64) * 0.25
        return (t[:, None] * _axis_direction(d, c)[None, :] + 0.37).astype(np.float32)
    raise AssertionError(kind)


def _axis_by_axis(lat, v0):
    import torch

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


def check_item_starts(lat):
    """The cut of every group's list into work items, restated from the list itself: one item per bucket of K entries; it
    starts at the first line start inside the bucket, or at the bucket's first entry where the bucket has none.  Returns
    (entries of the longest item, entries flagged sliding) over all groups."""
    info = lat.blur_lines()
    nbr = lat.neighbors()
    M, K = lat.M, info["item_size"]
    longest, sliding = 0, 0
    for g in range(info["groups"]):
        vertex, minus, plus, start = lat.blur_lines(g)
        _, joined = _lines_of(vertex, nbr[3 * g + 2])
        line_start = np.concatenate([[0], 1 + np.nonzero(~joined)[0]])
        want = np.arange(info["items"]) * K
        first = np.full(info["items"], M, np.int64)
        np.minimum.at(first, line_start // K, line_start)
        want = np.where(first < M, first, want)
        assert np.array_equal(start, np.concatenate([want, [M]])), g
        longest = max(longest, int(np.diff(start).max()))
        sliding += int((minus == 1).sum() + (plus == 1).sum())
    return longest, sliding


def longest_line(nbr_c):
    """Vertices of the longest line along one axis, from its [M, 2] neighbour table: lines run over mutual links only."""
    M = nbr_c.shape[0]
    nxt = nbr_c[:, 1]
    v = np.arange(M)
    mutual_next = (nxt >= 0) & (nbr_c[np.maximum(nxt, 0), 0] == v)
    prv = nbr_c[:, 0]
    has_prev = (prv >= 0) & (nbr_c[np.maximum(prv, 0), 1] == v)
    best = 0
    for s in np.nonzero(~has_prev)[0]:
        u, l = int(s), 1
        while mutual_next[u]:
            u, l = int(nxt[u]), l + 1
        best = max(best, l)
    return best


def blur_model_f32(nbr, v_ft):
    """The blur of all d + 1 axes in numpy float32 on rows in first-touch order, from a [d + 1, M, 2] neighbour table
    (Lattice.neighbors() / Oracle.neighbors()): per axis, in order, 2 * ((0.25 a + 0.5 s) + 0.25 b) with an absent
    neighbour's row as 0.  Every operand and every intermediate is float32; all products are by powers of two, so a
    fused multiply-add rounds no differently."""
    v = np.ascontiguousarray(v_ft, np.float32)
    q, h, two = np.float32(0.25), np.float32(0.5), np.float32(2.0)
    for axis in range(nbr.shape[0]):
        ia, ib = nbr[axis][:, 0], nbr[axis][:, 1]
        a = np.where((ia >= 0)[:, None], v[np.maximum(ia, 0)], np.float32(0.0))
        b = np.where((ib >= 0)[:, None], v[np.maximum(ib, 0)], np.float32(0.0))
        out = two * ((q * a + h * v) + q * b)
        assert out.dtype == np.float32
        v = out
    return v


# ---- everything the item sizes and the route switch must leave unchanged (test_gpu_blur3_every_d.py, in the parent and in
# fresh child processes) ----
ROUTE_LATTICES = (("d5_smooth", "smooth", 5, {}), ("d5_ramp", "axis_ramp", 5, {"c": 5, "n": 2048}),
                  ("d8_iid", "iid", 8, {"n": 1500}), ("d6_constant", "constant", 6, {}))


def route_results(phl):
    """{name: array}: the blur at the three widths on the four lattices, the filter (exact and default) at 256 channels at
    d = 5 and d = 8, the fused backward at L = 64 at d = 5 (a 384-channel blur); and per lattice what blur_lines says.
    The line lists of every lattice are checked on the way."""
    import torch

    out = {}
    for name, kind, d, kw in ROUTE_LATTICES:
        ref = _features(kind, d, **kw)
        lat = phl.Lattice(torch.from_numpy(ref).cuda())
        info = lat.blur_lines()
        line = _check_line_lists(lat)
        item, sliding = check_item_starts(lat)
        out[name + "/info"] = np.array([info["groups"], info["items"], info["item_size"], line, item, sliding, lat.M], np.int64)
        rng = np.random.default_rng(17 + d)
        for vd in WIDTHS3:
            v0 = torch.from_numpy(rng.standard_normal((lat.M, vd)).astype(np.float32)).cuda()
            out[f"{name}/blur{vd}"] = lat.blur(v0).cpu().numpy()
        if name in ("d5_smooth", "d8_iid"):
            src = torch.from_numpy(rng.random((ref.shape[0], 256), dtype=np.float32)).cuda()
            for exact in (True, False):
                out[f"{name}/filter256_exact{int(exact)}"] = lat.filter(src, exact=exact).cpu().numpy()
        if name == "d5_smooth":
            src = torch.from_numpy(rng.random((ref.shape[0], 64), dtype=np.float32)).cuda()
            g = torch.from_numpy(rng.standard_normal((ref.shape[0], 64)).astype(np.float32)).cuda()
            gs, gr = lat.filter_grad(src, g, torch.from_numpy(ref).cuda())
            out[name + "/grad_src"], out[name + "/grad_ref"] = gs.cpu().numpy(), gr.cpu().numpy()
    torch.cuda.synchronize()
    return out


INFO_FIELDS = ("groups", "items", "item_size", "longest_line", "longest_item", "sliding", "M")
