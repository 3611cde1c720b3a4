"""The fused backward of the lattice filter (phl_filter_grad: wide splat, blur, contracting slice) against an
independent float64 evaluation on the CPU (tests/_filter_grad_util.py, from the oracle's lattice -- never the GPU's).

The rule, per case and for both gradients, each error a fraction of the largest component of the float64 result:
    e_fused <= K * max(e_ref, 1e-6),   and never above the older bounds 2e-4 (features) / 1e-5 (source),
where e_ref is the distance of the reference's own fp32 formulation (``wide32``: the 2L(1+d)-channel operand through the
oracle's fp32 filter, torch's fp32 contraction) from float64 on the same inputs.  K covers what legitimately differs
between two correct fp32 evaluations: the kernel sums the L products of a pixel as four-channel dots, then slabs, then
a shuffle tree, and the splat sums per chunk first; the reference uses torch's sum.  K = 4 is the next power of two above
the largest ratio measured over every case of this file on an MI355X, 2.34 (d = 5, L = 20: e_ref 2.1e-6, fused 5.0e-6);
the source gradient never went above 0.37 of its floor.  DESIGN.md, f-2, holds the table."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from _filter_grad_util import Lattice64, grad64, image_features, scaled, slice_grad_mode, values, wide32

pytestmark = pytest.mark.gpu

K = 4
FLOOR = 1e-6
CAP_REF, CAP_SRC = 2e-4, 1e-5          # the bounds of tests/test_gpu_grad.py: never exceeded whatever e_ref is

_REFERENCES = {}


class Case:
    """Inputs and the two CPU evaluations of one case; computed once per key and shared (read-only) between tests."""

    def __init__(self, f, L, rng):
        from oracle import phl_oracle as po

        self.f = np.ascontiguousarray(f, np.float32)
        self.n, self.d = self.f.shape
        self.L = L
        self.src, self.g = values(self.n, L, rng)
        O = po.Oracle(self.f)
        self.Wg64, self.T64 = grad64(Lattice64(O), self.src, self.f, self.g)
        Wg32, T32 = wide32(O, self.src, self.f, self.g)
        # n = 1: W(g f) = f Wg, the gradient is zero and T64 is float64 rounding; the terms that cancel give the scale
        terms = 2 * (np.abs(self.src.astype(np.float64) * self.Wg64).sum(1)[:, None] * np.abs(self.f.astype(np.float64))).max()
        self.scale_T = float(np.abs(self.T64).max())
        if self.scale_T < 1e-6 * terms:
            self.scale_T = float(terms)
        self.scale_S = float(np.abs(self.Wg64).max())
        self.e_ref_T = float(np.abs(T32 - self.T64).max() / self.scale_T)
        self.e_ref_S = float(np.abs(Wg32 - self.Wg64).max() / self.scale_S)
        for a in (self.f, self.src, self.g, self.Wg64, self.T64):
            a.setflags(write=False)

    def cuda(self):
        return tuple(torch.tensor(x, device="cuda") for x in (self.f, self.src, self.g))        # (copies: the arrays are read-only)


def _case(key, make):
    if key not in _REFERENCES:
        _REFERENCES[key] = make()
    return _REFERENCES[key]


def _image_case(d, L, side=48, noise=0.2, scale=1.0, offset=0.0):
    def make():
        rng = np.random.default_rng(7000 + 100 * d + L)
        f = image_features(side, d, rng, noise=noise, scale=scale)
        f[:, :2] += np.float32(offset)
        return Case(f, L, rng)

    return _case(("image", d, L, side, noise, scale, offset), make)


def _judge(tag, case, got_src, got_ref):
    """Prints both errors of both gradients, then holds the rule of the module docstring."""
    e_T = float(np.abs(got_ref.cpu().numpy() - case.T64).max() / case.scale_T)
    line = f"[measured] {tag}: grad_ref e_ref {case.e_ref_T:.2e} e_fused {e_T:.2e} ratio {e_T / max(case.e_ref_T, FLOOR):.2f}"
    e_S = None
    if got_src is not None:
        e_S = float(np.abs(got_src.cpu().numpy() - case.Wg64).max() / case.scale_S)
        line += f"; grad_src e_ref {case.e_ref_S:.2e} e_fused {e_S:.2e} ratio {e_S / max(case.e_ref_S, FLOOR):.2f}"
    print(line)
    assert np.isfinite(e_T) and e_T <= K * max(case.e_ref_T, FLOOR) and e_T <= CAP_REF, line
    if e_S is not None:
        assert np.isfinite(e_S) and e_S <= K * max(case.e_ref_S, FLOOR) and e_S <= CAP_SRC, line


def _lattice(ref):
    """The clean-table lattice (what Oracle(ref) builds) and the code path k_slice_grad takes for its worst chunk."""
    import phl

    lat = phl.Lattice(ref)
    st = lat.tile_stats(4)
    return lat, st, slice_grad_mode(st["pixels_per_chunk"], lat.d, st["max_local_vertices"], st["max_local_vertices"])


def _equal_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. every instance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 20, 36, 64])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7])
def test_every_instance_against_float64(d, L, monkeypatch):
    """k_slice_grad<d + 1>, k_splat_wide<d + 1> and k_splat_tiled with nsets = d + 1 for every d the fused path takes.
    L = 4: one quarter-filled slab; 20 and 36: slabs with a tail; n = 48 * 48 = 9 chunks.  k_splat_wide takes the
    chunk classes of 16 lanes per slab row: L = 64, and L = 36 as well (nine four-channel pieces round up to 16 lanes:
    the kernel's only run with dead lanes in its one slab).  At both widths the one-phase and the multi-phase form
    (PHL_WIDE_ONE_PHASE=0, k_splat_tiled) are held to float64 and to each other bit for bit (same products, same
    order).  test_which_widths_take_the_one_phase_wide_splat proves which kernel ran."""
    case = _image_case(d, L)
    ref, src, g = case.cuda()
    lat, st, mode = _lattice(ref)
    assert st["staged_splat"] == 1, st
    monkeypatch.setenv("PHL_WIDE_ONE_PHASE", "1")
    got_src, got_ref = lat.filter_grad(src, g, ref)
    _judge(f"instance d={d} L={L} nv_max={st['max_local_vertices']} mode={mode}", case, got_src, got_ref)
    if L in (36, 64):
        monkeypatch.setenv("PHL_WIDE_ONE_PHASE", "0")
        b_src, b_ref = lat.filter_grad(src, g, ref)
        _judge(f"instance d={d} L={L} multi-phase splat", case, b_src, b_ref)
        assert _equal_bits(got_src, b_src) and _equal_bits(got_ref, b_ref)


# ---- 2. slice modes ---------------------------------------------------------------------------------------------------
# The knob is the scale of all features: the smaller the picture against a simplex, the more pixels share a vertex.
# (d, scale, noise of the sine features, path of the worst chunk, nv_max that tile_stats reported on the MI355X);
# 64 x 64 pixels = 16 chunks, and S_multi stays below 1500 of the 8192 that would decline the call.
# Bands (slice_grad_mode, P = 256): d = 5: 32-channel slabs up to 88 vertices, 16-channel slabs up to 176, DIRECT
# above; d = 2: 192 / 381; d = 3: 140 / 279; d = 4: 109 / 218; d = 6: 73 / 147; d = 7: 62 / 125.  d = 1 (295 / 581)
# stays on 32-channel slabs: 296 vertices in 256 pixels of one feature need |f| in the thousands, where the fp32
# noise of ANY evaluation (e_ref) is above the 2e-4 cap.
SLICE_MODES = [(5, 0.25, 0.2, 8, 49), (5, 0.5, 0.2, 4, 113), (5, 1.0, 0.2, 0, 251),
               (2, 1.0, 0.2, 8, 60), (2, 3.5, 0.2, 4, 291), (2, 5.0, 0.2, 0, 504),
               (1, 1.0, 0.2, 8, 4),
               (3, 0.5, 0.2, 8, 50), (3, 1.75, 0.2, 4, 215), (3, 3.0, 0.2, 0, 432),
               (4, 0.5, 0.2, 8, 79), (4, 1.0, 0.2, 4, 171), (4, 2.0, 0.2, 0, 400),
               (6, 0.15, 0.2, 8, 58), (6, 0.35, 0.2, 4, 122), (6, 0.7, 0.2, 0, 232),
               (7, 0.06, 0.0, 8, 35), (7, 0.15, 0.2, 4, 101), (7, 0.4, 0.2, 0, 233)]


@pytest.mark.parametrize("d,scale,noise,mode,nv_seen", SLICE_MODES)
def test_slice_modes_against_float64(d, scale, noise, mode, nv_seen):
    """The worst chunk of each lattice is proven to take the named path of k_slice_grad (asserted from tile_stats
    before anything is compared); L = 36 = 32 + 4 = 2 * 16 + 4 gives both slab widths a tail with dead lanes (the
    clamped ld4 and `chok`).  Scales, and the vertex counts they gave: the table above this test.  d = 5 and d = 2 are
    the two the work asked for; the others give every instance of the kernel every path it can reach."""
    case = _image_case(d, 36, side=64, noise=noise, scale=scale)
    ref, src, g = case.cuda()
    lat, st, got_mode = _lattice(ref)
    assert st["pixels_per_chunk"] == 256 and st["staged_splat"] == 1, st
    assert got_mode == mode, (st, got_mode)
    got_src, got_ref = lat.filter_grad(src, g, ref)
    _judge(f"slice mode {mode} d={d} scale={scale} nv_max={st['max_local_vertices']} (table: {nv_seen}) S_multi={st['multi_chunk_slots']}",
           case, got_src, got_ref)


# ---- 3. chunk geometry ------------------------------------------------------------------------------------------------
def _strip_case(n, d, L):
    def make():
        rng = np.random.default_rng(300 + n)
        p = np.arange(n)
        xx, yy = (p % 128).astype(np.float32), (p // 128).astype(np.float32)
        cols = [xx / 4, yy / 4] + [np.sin(xx / (7 + 3 * k)) * 2 + rng.random(n, dtype=np.float32) * 0.2 for k in range(d - 2)]
        return Case(np.stack(cols[:d], 1).astype(np.float32), L, rng)

    return _case(("strip", n, d, L), make)


@pytest.mark.parametrize("need_src", [True, False])
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 16400])
def test_chunk_geometry_against_float64(n, need_src):
    """n < P, n = P, a short last chunk (`kclamp`), and 65 chunks: the XCD order over a grid of 72 workgroups of which 7
    are idle, with a last chunk of 16 pixels."""
    d, L = 3, 8
    case = _strip_case(n, d, L)
    ref, src, g = case.cuda()
    lat, st, mode = _lattice(ref)
    P = st["pixels_per_chunk"]
    assert P == 256 and st["chunks"] == (n + P - 1) // P and st["staged_splat"] == 1, st
    if n == 16400:
        assert st["chunks"] == 65 and n - 64 * P == 16
    got_src, got_ref = lat.filter_grad(src, g, ref, need_src=need_src)
    assert (got_src is not None) == need_src
    _judge(f"geometry n={n} need_src={need_src} chunks={st['chunks']} mode={mode}", case, got_src, got_ref)


# ---- 4. strides, through the C ABI ------------------------------------------------------------------------------------
def _abi(lat, src, g, L, ref, grad_ref, grad_src):
    """phl_filter_grad itself: every stride is the tensor's own (views of wider buffers); returns the status."""
    import phl

    vp = C.c_void_p
    with torch.cuda.device(lat.device):
        rc = phl.load_library().phl_filter_grad(lat._h, vp(src.data_ptr()), src.stride(0), vp(g.data_ptr()), g.stride(0), L,
                                                vp(ref.data_ptr()), ref.stride(0), ref.stride(1), vp(grad_ref.data_ptr()),
                                                vp(grad_src.data_ptr()) if grad_src is not None else None,
                                                grad_src.stride(0) if grad_src is not None else 0, phl._stream(lat.device))
    torch.cuda.synchronize()
    return rc


def _in_columns(t, width, c0, fill=0.0):
    """``t`` [n, L] as columns c0 .. c0 + L of a fresh [n, width] buffer."""
    buf = torch.full((t.shape[0], width), fill, dtype=torch.float32, device=t.device)
    buf[:, c0:c0 + t.shape[1]] = t
    return buf, buf[:, c0:c0 + t.shape[1]]


@pytest.mark.parametrize("ref_layout", ["dense", "transposed", "rows_of_8"])
def test_row_strides_through_the_c_abi(ref_layout):
    """src_rs = g_rs = 72 and grad_src_rs = 48 (columns 4..40 of wider tensors, 16-byte aligned), ref as the [n, d] view
    of a [d, n] tensor (ref_rs = 1, ref_cs = n: what the NCHW batched path passes) and as rows of an [n, 8] tensor."""
    d, L = 5, 36
    case = _image_case(d, L)
    ref, src, g = case.cuda()
    n = case.n
    lat, st, mode = _lattice(ref)
    _, src_v = _in_columns(src, 72, 4)
    _, g_v = _in_columns(g, 72, 4)
    out_buf = torch.full((n, 48), float("nan"), device="cuda")
    out_v = out_buf[:, 4:40]
    if ref_layout == "transposed":
        ref_v = ref.t().contiguous().t()
        assert ref_v.stride() == (1, n)
    elif ref_layout == "rows_of_8":
        ref_v = torch.full((n, 8), float("nan"), device="cuda")
        ref_v[:, :d] = ref
        ref_v = ref_v[:, :d]
        assert ref_v.stride() == (8, 1)
    else:
        ref_v = ref
    assert src_v.stride(0) == 72 and src_v.data_ptr() % 16 == 0 and out_v.stride(0) == 48 and out_v.data_ptr() % 16 == 0
    grad_ref = torch.full((n, d), float("nan"), device="cuda")
    assert _abi(lat, src_v, g_v, L, ref_v, grad_ref, out_v) == 0
    _judge(f"strides 72/72/48 ref {ref_layout} mode={mode}", case, out_v, grad_ref)
    outside = torch.ones((n, 48), dtype=torch.bool, device="cuda")
    outside[:, 4:40] = False
    assert torch.isnan(out_buf[outside]).all(), "grad_src was written outside its columns"
    # the same bits as the contiguous call: strides change addresses, not arithmetic
    c_src, c_ref = lat.filter_grad(src, g, ref)
    assert _equal_bits(out_v.contiguous(), c_src) and _equal_bits(grad_ref, c_ref)


@pytest.mark.parametrize("what", ["src_base", "g_base", "grad_src_base", "src_rs", "g_rs", "grad_src_rs"])
def test_rows_off_the_16_byte_grid_are_refused_untouched(what):
    """A base one float off the grid, or a row stride of 38 floats: status 7 (unsupported) before anything is written."""
    import phl

    d, L = 5, 36
    case = _image_case(d, L)
    ref, src, g = case.cuda()
    n = case.n
    lat, _, _ = _lattice(ref)
    nan = float("nan")
    src_v = _in_columns(src, 72, 1)[1] if what == "src_base" else _in_columns(src, 38, 0)[1] if what == "src_rs" else src
    g_v = _in_columns(g, 72, 1)[1] if what == "g_base" else _in_columns(g, 38, 0)[1] if what == "g_rs" else g
    out_buf = torch.full((n, 38 if what == "grad_src_rs" else 72), nan, device="cuda")
    out_v = out_buf[:, 1:37] if what == "grad_src_base" else out_buf[:, 0:36]
    grad_ref = torch.full((n, d), nan, device="cuda")
    assert _abi(lat, src_v, g_v, L, ref, grad_ref, out_v) == phl.ERR_UNSUPPORTED
    assert torch.isnan(grad_ref).all() and torch.isnan(out_buf).all()


# ---- 5. output semantics ----------------------------------------------------------------------------------------------
def test_first_pass_overwrites_and_need_src_changes_no_bit():
    d, L = 5, 36
    case = _image_case(d, L)
    ref, src, g = case.cuda()
    n = case.n
    lat, _, _ = _lattice(ref)
    fresh_src, fresh_ref = lat.filter_grad(src, g, ref)
    grad_ref = torch.full((n, d), float("nan"), device="cuda")
    grad_src = torch.full((n, L), float("nan"), device="cuda")
    assert _abi(lat, src, g, L, ref, grad_ref, grad_src) == 0
    assert torch.isfinite(grad_ref).all() and torch.isfinite(grad_src).all()
    assert _equal_bits(grad_ref, fresh_ref) and _equal_bits(grad_src, fresh_src)
    none, only_ref = lat.filter_grad(src, g, ref, need_src=False)
    assert none is None and _equal_bits(only_ref, fresh_ref)
    grad_ref.fill_(float("nan"))
    assert _abi(lat, src, g, L, ref, grad_ref, None) == 0 and _equal_bits(grad_ref, fresh_ref)
    _judge("output semantics d=5 L=36", case, fresh_src, fresh_ref)


def test_no_channels_give_a_zero_feature_gradient():
    """L = 0: the sum over channels is empty.  Through the C ABI (views of one-channel tensors: a real address, no
    channel read) and through the binding, whose empty tensors have no address at all."""
    case = _image_case(5, 36)
    ref, src, g = case.cuda()
    lat, _, _ = _lattice(ref)
    grad_ref = torch.full((case.n, 5), float("nan"), device="cuda")
    assert _abi(lat, src[:, :0], g[:, :0], 0, ref, grad_ref, None) == 0
    assert (grad_ref == 0).all()
    empty = torch.empty((case.n, 0), device="cuda")
    got_src, got_ref = lat.filter_grad(empty, empty, ref)
    assert got_src.shape == (case.n, 0) and (got_ref == 0).all()


@pytest.mark.parametrize("group", ["under 64", "64"])
def test_channel_groups_against_float64(group, monkeypatch):
    """PHL_GRAD_WS_MB cuts the call into channel groups; every group after the first accumulates into grad_ref
    (c0 > 0).  1 MiB gives groups of fewer than 64 channels (asserted from the lattice's row counts with the formula of
    phl_filter_grad), i.e. well over three accumulating groups at L = 192; the second budget gives 64-channel groups."""
    d, L = 5, 192
    case = _image_case(d, L)
    ref, src, g = case.cuda()
    lat, st, mode = _lattice(ref)
    per_ch = (2 * lat.M + st["multi_chunk_slots"]) * (d + 1) * 4          # bytes of workspace per channel

    def group_of(mb):
        fit = (mb << 20) // per_ch
        return min(L, fit // 64 * 64 if fit >= 64 else fit // 4 * 4)

    if group == "under 64":
        mb = 1
        assert 4 <= group_of(mb) < 64, (per_ch, group_of(mb))
    else:
        mb = next(m for m in range(1, 4096) if group_of(m) >= 64)
        assert group_of(mb) == 64, (per_ch, mb, group_of(mb))
    monkeypatch.setenv("PHL_GRAD_WS_MB", str(mb))
    got_src, got_ref = lat.filter_grad(src, g, ref)
    _judge(f"channel groups of {group_of(mb)} (PHL_GRAD_WS_MB={mb}) d={d} L={L} mode={mode}", case, got_src, got_ref)


# ---- 6. cancellation --------------------------------------------------------------------------------------------------
def test_cancellation_at_large_features():
    """The first two features offset by +300: f (Wg) - W(g f) loses two more digits in ANY fp32 evaluation, the
    reference's included (e_ref ~ 1e-4), and the bound moves with e_ref, up to the cap of 2e-4."""
    case = _image_case(5, 36, offset=300.0)
    ref, src, g = case.cuda()
    lat, st, mode = _lattice(ref)
    got_src, got_ref = lat.filter_grad(src, g, ref)
    _judge(f"cancellation |f| ~ 300 d=5 L=36 mode={mode}", case, got_src, got_ref)


# ---- which splat kernel ran ---------------------------------------------------------------------------------------------
def test_which_widths_take_the_one_phase_wide_splat():
    """k_splat_wide is taken by the chunk classes of 16 lanes per slab row (phl_launch_splat_tiled).  PHL_DEBUG is
    read once per process, so a fresh one prints its plan lines ("[phl] splat vd=... class i/n: ... N lanes") for the
    lattices and widths of the instance test: every d must show a 16-lane class at L = 64 and at L = 36 (33..64
    channels round up to 16 lanes), none at L = 4 and 20, and none at L = 256 (these nine-chunk lattices take 32
    lanes there)."""
    code = (
        "import os, sys, numpy as np, torch\n"
        "root = sys.argv[1]\n"
        "sys.path[:0] = [os.path.join(root, 'depth-estimation_amd'), root, os.path.join(root, 'tests')]\n"
        "import phl\n"
        "from _filter_grad_util import image_features, values\n"
        "for d in range(1, 8):\n"
        "    rng = np.random.default_rng(d)\n"
        "    ref = torch.from_numpy(image_features(48, d, rng)).cuda()\n"
        "    lat = phl.Lattice(ref)\n"
        "    for L in (4, 20, 36, 64, 256):\n"
        "        src, g = (torch.from_numpy(x).cuda() for x in values(ref.shape[0], L, rng))\n"
        "        torch.cuda.synchronize()\n"
        "        print(f'CASE d={d} L={L}', file=sys.stderr, flush=True)\n"
        "        lat.filter_grad(src, g, ref, need_src=False)\n"
        "        torch.cuda.synchronize()\n"
        "print('DONE', file=sys.stderr, flush=True)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, root], env=dict(os.environ, PHL_DEBUG="1", PHL_WIDE_ONE_PHASE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stderr, r.stderr[-2000:]
    lanes, current = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"CASE d=(\d+) L=(\d+)", line)
        if m:
            current = (int(m.group(1)), int(m.group(2)))
            lanes[current] = set()
            continue
        m = re.match(r"\[phl\] splat vd=(\d+) class \d+/\d+: .* (\d+) lanes", line)
        if m and current is not None:
            assert int(m.group(1)) == current[1], (line, current)
            lanes[current].add(int(m.group(2)))
    assert len(lanes) == 35 and all(lanes.values()), lanes
    for (d, L), seen in sorted(lanes.items()):
        assert (16 in seen) == (L in (36, 64)), (d, L, seen)
