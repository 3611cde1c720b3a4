"""phl -- Python binding of the MI355X permutohedral-lattice filter (C ABI in include/phl.h).

Thin plumbing only: torch supplies device memory and the current HIP stream, ctypes calls
``lib/libphl.so``.  There is NO CPU implementation behind this module: if the shared library or
a HIP device is missing, calls raise ``RuntimeError``.  CPU tensors are accepted the way the
reference accepts them (its extension is CPU-only, crf/lattice/lite/permutohedral.h:214) but
are computed on the GPU and copied back.

Public surface
    Lattice(ref)                 build once per feature tensor  (init-once / filter-many)
    Lattice.filter(src, ...)     == reference ``lattice.filter(src, ref)`` for that ref
    filter(src, ref)             drop-in for ``latticefilter`` (crf/gaussian_matrix.py:15-16);
                                 lattices are cached per ``ref`` tensor, invisibly
"""
import ctypes as C
import os
import threading
from collections import OrderedDict

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PHL_LIB: another build of the same library (A/B timing of two source states on one box); never a fallback
LIB_PATH = os.environ.get("PHL_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libphl.so")

SUBTRACT_INPUT = 1
EXACT = 4
NO_TILES = 8
ERR_UNSUPPORTED = 7          # PHL_ERR_UNSUPPORTED: the kernels do not take this shape, the caller keeps its own path
FILTER_GRAD_MAX_D = 16       # PHL_FILTER_GRAD_MAX_D: most feature dimensions phl_filter_grad takes (tests hold it to the header)
GUIDED_FULL_MAX_CX = 4       # PHL_GUIDED_FULL_MAX_CX: most guide channels phl_guided_filter_full takes
GUIDED_BILINEAR_FULL_COV = 1 # PHL_GUIDED_BILINEAR_FULL_COV: flag of phl_guided_filter_bilinear
BUILD_REFERENCE_TABLE = 1

_lib = None
_lib_lock = threading.Lock()


class PhlError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"phl error {status}: {message}")
        self.status = status


# The C ABI: one line per prototype of include/phl.h, in the header's order (name, return kind, argument kinds), kept
# equal to the header by tests/test_abi_table_host.py.  Argument kinds: P pointer (arrays and phl_lattice ** included),
# S phl_stream, i int, q int64_t, I unsigned, Q uint64_t, f float, d double; return kinds: i int, q int64_t, N size_t,
# z const char *.
_KINDS = {"P": C.c_void_p, "S": C.c_void_p, "i": C.c_int, "q": C.c_int64, "I": C.c_uint, "Q": C.c_uint64, "f": C.c_float,
          "d": C.c_double, "N": C.c_size_t, "z": C.c_char_p}
_ABI = (
    ("phl_version", "i", ""),
    ("phl_last_error", "z", ""),
    ("phl_status_string", "z", "i"),
    ("phl_device_count", "i", ""),
    ("phl_build", "i", "PPqiqqiS"),
    ("phl_build_ex", "i", "PPqiqqiSI"),
    ("phl_destroy", "i", "P"),
    ("phl_num_pixels", "q", "P"),
    ("phl_num_vertices", "q", "P"),
    ("phl_num_dims", "i", "P"),
    ("phl_device", "i", "P"),
    ("phl_device_bytes", "q", "P"),
    ("phl_trim_scratch", "i", ""),
    ("phl_add_vertices", "i", "PPqPS"),
    ("phl_num_local_vertices", "q", "P"),
    ("phl_vertices_of_pixels", "i", "PqqPS"),
    ("phl_sub_lattice", "i", "PPqqPqqPqqS"),
    ("phl_reserve", "i", "Pi"),
    ("phl_reserve_ex", "i", "PiI"),
    ("phl_filter", "i", "PPiqqPqqIS"),
    ("phl_filter_once", "i", "PiqqPiqqqPqqIiS"),
    ("phl_filter_grad", "i", "PPqPqiPqqPPqS"),
    ("phl_splat", "i", "PPiqPIS"),
    ("phl_blur_axis", "i", "PiPPiS"),
    ("phl_blur", "i", "PPPiPS"),
    ("phl_gather_rows", "i", "PiPqPqS"),
    ("phl_scatter_add_rows", "i", "PiPqPqS"),
    ("phl_num_chunks", "q", "P"),
    ("phl_partial_rows", "q", "P"),
    ("phl_chunks_touching", "i", "PPqPS"),
    ("phl_splat_part", "i", "PPiqPPPqPqS"),
    ("phl_splat_part_pack", "i", "PPiqPPPqPqPPqS"),
    ("phl_set_blur_rows", "i", "PPi"),
    ("phl_slice", "i", "PPiPqPqIS"),
    ("phl_softmax_neg_add", "i", "PqPqPqqiS"),
    ("phl_compat_softmax", "i", "PqPqPPqqiIS"),
    ("phl_compat_planes_bytes", "N", "i"),
    ("phl_compat_prepare", "i", "PiPS"),
    ("phl_compat_softmax_split", "i", "PqPqPPPqqiIS"),
    ("phl_uniform_compat_softmax", "i", "PqPqffPqqiIS"),
    ("phl_nchw_softmax_compat", "i", "PPPffPiiqiS"),
    ("phl_nchw_softmax_compat_wide", "i", "PPPPiiqS"),
    ("phl_nchw_step_train", "i", "PPPPiiqS"),
    ("phl_nchw_step_train_grad", "i", "PPPPPPiiqS"),
    ("phl_nchw_step_train_partials", "i", "iiq"),
    ("phl_nchw_expected_value", "i", "PPPPiiqiS"),
    ("phl_nchw_expected_value_grad", "i", "PPPPPiiqiS"),
    ("phl_nchw_scalar_unaries", "i", "PPPPPiiiiiiddS"),
    ("phl_nchw_scalar_unaries_grad", "i", "PPPPPPiiiiiiddS"),
    ("phl_nchw_confidence_unaries", "i", "PPPiiqS"),
    ("phl_nchw_confidence_unaries_grad", "i", "PPPPPiiqS"),
    ("phl_softmax_neg_grad", "i", "PqPqPqqiS"),
    ("phl_uniform_compat_grad", "i", "PqPqffPqPqqiS"),
    ("phl_compat_grad_x", "i", "PqPfPqqiS"),
    ("phl_compat_mu_grad_workspace_bytes", "N", "qi"),
    ("phl_compat_mu_grad", "i", "PqPqfqiPPiS"),
    ("phl_expected_value", "i", "PqPPqiS"),
    ("phl_cost_volume", "i", "PPiiiiiiPqS"),
    ("phl_cost_volume_nchw", "i", "PPiiiiqqqqiiiIPqqqS"),
    ("phl_disparity_wta", "i", "PPiiiiqqqqiiiPPqqS"),
    ("phl_box_blur", "i", "PPqqqiiS"),
    ("phl_box_blur_grad", "i", "PPqqqidPPS"),
    ("phl_box_blur_fused_max_r", "i", "iii"),
    ("phl_guided_filter", "i", "PPPPiiiiiiiiPPPPPfS"),
    ("phl_guided_filter_full", "i", "PPPPiiiiiiiiPPPPPfS"),
    ("phl_guided_filter_max_r", "i", ""),
    ("phl_guided_filter_labels_per_chunk", "i", "iiiiiii"),
    ("phl_guided_filter_grad", "i", "PPPPPPiiiiiiiiPPPPPfiS"),
    ("phl_guided_filter_grad_max_r", "i", ""),
    ("phl_guided_filter_full_grad", "i", "PPPPPPiiiiiiiiPPPPPfiS"),
    ("phl_guided_filter_full_grad_labels_per_chunk", "i", "iiiiiii"),
    ("phl_guided_filter_bilinear", "i", "PPPPiiiiiiiiPfIS"),
    ("phl_guided_filter_bilinear_labels_per_chunk", "i", "iiiii"),
    ("phl_guided_filter_bilinear_grad", "i", "PPPPPPiiiiiiiiPfiIS"),
    ("phl_guided_filter_bilinear_full_grad", "i", "PPPPPPiiiiiiiiPfiS"),
    ("phl_stream_copy", "i", "PPqS"),
    ("phl_copy2d", "i", "PqqPqqqiS"),
    ("phl_tile_stats", "i", "PiP"),
    ("phl_get_vertex_order", "i", "PP"),
    ("phl_get_pixel_order", "i", "PP"),
    ("phl_get_keys", "i", "PP"),
    ("phl_get_replay", "i", "PPP"),
    ("phl_get_neighbors", "i", "PP"),
    ("phl_get_blur_lines", "i", "PiPPPP"),
    ("phl_get_splat_lists", "i", "PPPP"),
    ("phl_debug_reference_table", "i", "PPqiqPqPPPiPP"),
    ("phl_debug_probe_paths", "i", "PqiPiPiQPiiP"),
    ("phl_debug_slow_copy", "i", "PPqiiS"),
    ("phl_debug_side_streams", "i", ""),
    ("phl_debug_live_blocks", "q", ""),
)


def load_library():
    """Load lib/libphl.so (built by ``python __graft_entry__.py`` / ``make -C csrc``) and declare its signatures."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is not built (run `python __graft_entry__.py`). "
                "There is no CPU fallback for the lattice filter.")
        lib = C.CDLL(LIB_PATH)
        for name, ret, args in _ABI:
            fn = getattr(lib, name, None)       # (an older build loaded through PHL_LIB lacks the newer entry points)
            if fn is not None:
                fn.restype, fn.argtypes = _KINDS[ret], [_KINDS[k] for k in args]
        _lib = lib
        return lib


def _check(rc):
    if rc != 0:
        raise PhlError(rc, load_library().phl_last_error().decode("utf-8", "replace"))


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("phl: no HIP device visible to torch; the lattice filter has no CPU fallback")


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _host(a):
    """A numpy array the library reads or fills on the host."""
    return a.ctypes.data_as(C.c_void_p)


def _launch(device, name, *args):
    """Library function ``name`` on ``device`` with its current stream as the last argument; raises on a failed status.
    Looked up on every call, so that a replaced attribute of the library (a test's spy) is the one that runs."""
    with torch.cuda.device(device):
        _check(getattr(load_library(), name)(*args, _stream(device)))


def _call(name, *args, value=False):
    """Library function ``name`` that takes no stream (sizes, host readers, settings), looked up like _launch's: raises on
    a failed status, or with ``value`` returns what the function returned."""
    rv = getattr(load_library(), name)(*args)
    if value:
        return rv
    _check(rv)


def _flags(subtract_input=False, exact=False, no_tiles=False):
    return (SUBTRACT_INPUT if subtract_input else 0) | (EXACT if exact else 0) | (NO_TILES if no_tiles else 0)


def _default_device(t):
    """The device a result is built on when the caller names none: ``t``'s own GPU, or the current one for anything else."""
    return t.device if (torch.is_tensor(t) and t.is_cuda) else torch.device("cuda", torch.cuda.current_device())


def to_device(t, device):
    """``t.to(device)`` for the reference's calling convention -- pageable CPU tensors (DenseCrf.ipynb:142-152 hands
    CPU tensors to mean_field_infer).  Enqueued on the current stream.

    The runtime's own pageable path is the fast one on this platform (tools/h2d_probe.py: 44-52 GB/s from pageable memory
    at 7 MB ... 1 GB -- it pins the user's pages for the DMA); copying through pinned staging pieces first, as rounds 3-4 did,
    is bound by the host memcpy and by the caching host allocator handing out fresh pinned blocks while earlier pieces are
    still in flight (3-4 GB/s at 128 MB and up, 20 GB/s at 7 MB on the same box; box to box the notebook-sized call swung
    between 1.2 and 5 ms)."""
    device = torch.device(device)
    if t.device == device:
        return t
    return t.to(device, non_blocking=(not t.is_cuda and t.is_pinned()))


def to_host(t):
    """Device tensor -> CPU tensor in pinned memory (one DMA, no bounce through the runtime's staging buffers);
    returns after the copy has completed."""
    if not t.is_cuda:
        return t
    if t.numel() * t.element_size() < (1 << 20):
        return t.cpu()
    out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return out


def _as_device(t, device):
    if t.dtype != torch.float32:
        # the reference extension is float-only (accessor<float,2>, permutohedral.h:214-215)
        raise TypeError(f"phl: expected float32 tensor, got {t.dtype}")
    return t if t.device == device else to_device(t, device)


_parked = []    # lattice handles whose owner died during a stream capture; freed by the next close()


class Lattice:
    """Permutohedral lattice of a feature tensor ``ref`` [n, d] (fp32, any strides).

    Build cost is paid once; ``filter`` then runs splat -> blur -> slice for any [n, vd] values.
    Re-entrant: any number of threads / streams may filter through one Lattice at the same time (the C library
    hands every call its own value workspace; see phl_reserve in include/phl.h).
    """

    def __init__(self, ref, device=None, reference_table=False):
        """reference_table=True: reproduce the reference's hash-table behaviour across its doublings (duplicate
        vertices above M = 16383, see PHL_BUILD_REFERENCE_TABLE in include/phl.h) -- with ``exact=True`` the
        filter is then bit-identical to the reference's CPU path at any size."""
        _require_gpu()
        load_library()
        if ref.dim() != 2:
            raise ValueError(f"ref must be [n, d], got {tuple(ref.shape)}")
        device = torch.device(_default_device(ref) if device is None else device)
        ref_d = _as_device(ref.detach(), device)
        n, d = int(ref_d.shape[0]), int(ref_d.shape[1])
        handle = C.c_void_p()
        with torch.cuda.device(device):
            _call("phl_build_ex", C.byref(handle), _ptr(ref_d), n, d, ref_d.stride(0), ref_d.stride(1), device.index or 0,
                  _stream(device), BUILD_REFERENCE_TABLE if reference_table else 0)
        self._adopt(handle, device, n, d, reference_table)

    def _adopt(self, handle, device, n, d, reference_table):
        """Take ownership of a built lattice: everything a Lattice knows about its handle."""
        self.device, self.n, self.d = device, n, d
        self.reference_table = bool(reference_table)
        self._h = handle
        self.M = int(_call("phl_num_vertices", handle, value=True))
        return self

    # ---- a band cut out of the whole image's lattice (row-band multi-GPU, phl/rowtile.py) ---------------------
    @classmethod
    def whole_image(cls, ref, device=None):
        """The lattice row bands are cut from: the whole image's, with the reference's table behaviour."""
        return cls(ref, device=device, reference_table=True)

    def vertices_of_pixels(self, p0, p1):
        """bool numpy [M]: first-touch vertices touched by pixels [p0, p1)."""
        mask = np.zeros(self.M, np.uint8)
        _launch(self.device, "phl_vertices_of_pixels", self._h, int(p0), int(p1), _host(mask))
        return mask.astype(bool)

    def sub_lattice(self, p0, p1, sel, n_own, ref_band):
        """Lattice of pixels [p0, p1) on the selected vertices ``sel`` (first-touch ids; the first n_own = every vertex those
        pixels touch, then ghosts in the caller's order): phl_sub_lattice in include/phl.h.  The new lattice numbers its
        vertices by position in ``sel``; rows of ghost vertices are M_own + position among the ghosts."""
        sel = np.ascontiguousarray(sel, np.int32)
        ref_d = _as_device(ref_band.detach(), self.device)
        assert ref_d.shape == (p1 - p0, self.d)
        handle = C.c_void_p()
        _launch(self.device, "phl_sub_lattice", C.byref(handle), self._h, int(p0), int(p1), _host(sel), len(sel), int(n_own),
                _ptr(ref_d), ref_d.stride(0), ref_d.stride(1))
        return Lattice.__new__(Lattice)._adopt(handle, self.device, int(p1 - p0), self.d, self.reference_table)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:          # at interpreter shutdown the module globals may be gone
            try:
                # phl_destroy hipFree()s; inside a stream capture that would invalidate the capture
                # (a garbage-collected Lattice can land here at any time), so park the handle instead
                if torch.cuda.is_current_stream_capturing():
                    _parked.append(h)
                    return
                _lib.phl_destroy(h)
                while _parked:
                    _lib.phl_destroy(_parked.pop())
            except Exception:
                pass

    __del__ = close

    @property
    def device_bytes(self):
        return int(_call("phl_device_bytes", self._h, value=True))

    def reserve(self, vd, strided_io=False, exact=False):
        """Pre-size everything a ``filter`` over ``vd`` channels needs, so that the next call -- on any stream,
        e.g. inside a HIP-graph capture -- allocates nothing.  strided_io: also the staging copies channel-major
        (NCHW) views -- and, from 128 channels on, pixel-major rows off the 16-byte grid such as column slices -- go
        through; exact: prepare for ``exact=True`` calls."""
        _call("phl_reserve_ex", self._h, int(vd), (1 if strided_io else 0) | (2 if exact else 0))

    # ---- hot path ---------------------------------------------------------------------------
    def filter(self, src, subtract_input=False, out=None, exact=False, no_tiles=False):
        """``lattice.filter(src, ref)`` of the reference; result lives on ``src``'s device.

        exact: reference-exact arithmetic (pixel-ordered splat sums, per-term divide in slice):
        bit-identical to the reference's CPU path.  The default LDS-staged path agrees to fp32
        rounding (~1e-7 relative).  no_tiles: plain gather kernels (A/B)."""
        if src.dim() != 2 or src.shape[0] != self.n:
            # same text as the reference's assert (gaussian_matrix.py:429-430)
            raise AssertionError("Incompatible shapes {}, and {}".format(tuple(src.shape), (self.n, self.d)))
        src_d = _as_device(src.detach(), self.device)
        vd = int(src_d.shape[1])
        res = out if (out is not None and out.device == self.device) else torch.empty(
            (self.n, vd), dtype=torch.float32, device=self.device)
        _launch(self.device, "phl_filter", self._h, _ptr(src_d), vd, src_d.stride(0), src_d.stride(1), _ptr(res), res.stride(0),
                res.stride(1), _flags(subtract_input, exact, no_tiles))
        if out is not None and out is not res:
            out.copy_(res)
            return out
        if src.device == self.device:
            return res
        return to_host(res) if src.device.type == "cpu" else res.to(src.device)

    # ---- stages (profiling / parity of intermediates) ---------------------------------------
    def splat(self, src, exact=False, no_tiles=False, out=None):
        src_d = _as_device(src.detach(), self.device)
        assert src_d.stride(1) == 1, "stage API takes pixel-major rows"
        vd = int(src_d.shape[1])
        vert = torch.empty((self.M, vd), dtype=torch.float32, device=self.device) if out is None else out
        assert vert.shape == (self.M, vd) and vert.is_contiguous()
        _launch(self.device, "phl_splat", self._h, _ptr(src_d), vd, src_d.stride(0), _ptr(vert), _flags(False, exact, no_tiles))
        return vert

    # ---- splat in parts (row-band exchange overlap, see phl_splat_part in include/phl.h) ------------------
    def chunks_touching(self, rows):
        """bool numpy mask [#chunks]: pixel chunks that contribute to any of the vertex rows (int64 device tensor)."""
        mask = np.zeros(int(_call("phl_num_chunks", self._h, value=True)), np.int32)
        rows = rows.to(self.device, torch.int64).contiguous()
        _launch(self.device, "phl_chunks_touching", self._h, _ptr(rows), int(rows.numel()), _host(mask))
        return mask.astype(bool)

    @property
    def partial_rows(self):
        return int(_call("phl_partial_rows", self._h, value=True))

    def splat_part(self, src, out, partial, chunks, rows, pack_pos=None, pack=None):
        """Run the chunk splat for the listed chunks (int32 device tensor) and complete the listed vertex rows
        (int32 device tensor) of ``out`` [M, vd]; ``partial`` [partial_rows, vd] is shared by the parts of one splat.
        pack_pos (int32 device tensor, one per listed row) / pack [*, vd]: listed row i is also written to
        pack[pack_pos[i]] by the kernel that completes it (the row-band exchange's send buffer)."""
        vd = int(src.shape[1])
        assert src.stride(1) == 1 and out.is_contiguous() and out.shape == (self.M, vd)
        assert chunks.dtype == torch.int32 and rows.dtype == torch.int32 and chunks.is_contiguous() and rows.is_contiguous()
        assert partial.is_contiguous() and partial.shape[0] >= self.partial_rows and partial.shape[1] == vd
        part = (self._h, _ptr(src), vd, src.stride(0), _ptr(out), _ptr(partial), _ptr(chunks), int(chunks.numel()), _ptr(rows),
                int(rows.numel()))
        if pack_pos is None:
            _launch(self.device, "phl_splat_part", *part)
        else:
            assert pack_pos.dtype == torch.int32 and pack_pos.is_contiguous() and pack_pos.numel() == rows.numel()
            assert pack.stride(1) == 1 and pack.shape[1] == vd and pack.dtype == torch.float32
            _launch(self.device, "phl_splat_part_pack", *part, _ptr(pack_pos), _ptr(pack), pack.stride(0))
        return out

    def set_blur_rows(self, ranges):
        """Row-band lattices: per blur axis the rows whose output of that axis is read later, as three ascending
        {begin, end} row ranges (numpy / list [d+1][3][2]); None: all rows.  See phl_set_blur_rows in include/phl.h."""
        if ranges is None:
            _call("phl_set_blur_rows", self._h, None, 0)
            return
        r = np.ascontiguousarray(ranges, np.int64)
        assert r.shape == (self.d + 1, 3, 2), r.shape
        _call("phl_set_blur_rows", self._h, _host(r), self.d + 1)

    def blur_axis(self, axis, vin, vout=None):
        vd = int(vin.shape[1])
        vout = torch.empty_like(vin) if vout is None else vout
        assert vin.is_contiguous() and vout.is_contiguous()
        _launch(self.device, "phl_blur_axis", self._h, int(axis), _ptr(vin), _ptr(vout), vd)
        return vout

    def blur(self, vert, scratch=None):
        """All d+1 axes (two per pass).  ``vert`` is overwritten (it is one of the two ping-pong buffers)."""
        other = torch.empty_like(vert) if scratch is None else scratch
        assert vert.is_contiguous() and other.is_contiguous() and other.shape == vert.shape
        which = C.c_int(0)
        _launch(self.device, "phl_blur", self._h, _ptr(vert), _ptr(other), int(vert.shape[1]), C.byref(which))
        return other if which.value else vert

    def gather_rows(self, vert, idx, out=None):
        """out[r] = vert[idx[r]] (idx: int64 device tensor).  Row-band exchange helper."""
        k, vd = int(idx.numel()), int(vert.shape[1])
        out = torch.empty((k, vd), dtype=torch.float32, device=self.device) if out is None else out
        assert vert.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous() and out.stride(1) == 1
        _launch(self.device, "phl_gather_rows", _ptr(vert), vd, _ptr(idx), k, _ptr(out), out.stride(0) if k else vd)
        return out

    def scatter_add_rows(self, vert, idx, rows):
        """vert[idx[r]] += rows[r]; idx must hold distinct vertex ids."""
        k, vd = int(idx.numel()), int(vert.shape[1])
        assert vert.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous() and (k == 0 or rows.stride(1) == 1)
        _launch(self.device, "phl_scatter_add_rows", _ptr(vert), vd, _ptr(idx), k, _ptr(rows), rows.stride(0) if k else vd)
        return vert

    def slice(self, vert, sub=None, exact=False, out=None, no_tiles=False):
        vd = int(vert.shape[1])
        out = torch.empty((self.n, vd), dtype=torch.float32, device=self.device) if out is None else out
        _launch(self.device, "phl_slice", self._h, _ptr(vert), vd, _ptr(out), out.stride(0), _ptr(sub),
                sub.stride(0) if sub is not None else 0, _flags(False, exact, no_tiles))
        return out

    def filter_grad(self, src, g, ref, need_src=True):
        """Gradients of ``sum(g * filter(src, ref))``: returns (grad_src or None, grad_ref [n, d]) -- the body of
        LatticeFilter.backward (crf/gaussian_matrix.py:435-468) in two fused passes (phl_filter_grad in
        include/phl.h).  d <= FILTER_GRAD_MAX_D = 16: above d = 7 the features are contracted in ceil(d / 7) groups of at
        most 7 columns (8 -> 4+4, 16 -> 6+5+5), each with a wide vertex buffer of (columns + 1) L channels, so the
        workspace is that of the widest group; PHL_GRAD_FEATURES_PER_GROUP (1..7) caps the group size at any d.  Raises
        PhlError(status UNSUPPORTED) for shapes the fused path does not take."""
        src_d = _as_device(src.detach(), self.device).contiguous()
        g_d = _as_device(g.detach(), self.device).contiguous()
        ref_d = _as_device(ref.detach(), self.device)
        assert src_d.shape == g_d.shape and src_d.shape[0] == self.n and ref_d.shape == (self.n, self.d)
        L = int(src_d.shape[1])
        grad_ref = torch.empty((self.n, self.d), dtype=torch.float32, device=self.device)
        grad_src = torch.empty((self.n, L), dtype=torch.float32, device=self.device) if need_src else None
        _launch(self.device, "phl_filter_grad", self._h, _ptr(src_d), src_d.stride(0), _ptr(g_d), g_d.stride(0), L, _ptr(ref_d),
                ref_d.stride(0), ref_d.stride(1), _ptr(grad_ref), _ptr(grad_src), L)
        return grad_src, grad_ref

    def tile_stats(self, vd):
        """Chunk statistics of the LDS-staged path (see phl_tile_stats in include/phl.h)."""
        out = np.zeros(7, np.int64)
        _call("phl_tile_stats", self._h, int(vd), _host(out))
        keys = ("pixels_per_chunk", "chunks", "max_local_vertices", "slots", "multi_chunk_slots", "staged_splat",
                "staged_slice")
        return dict(zip(keys, (int(x) for x in out)))

    def add_vertices(self, keys):
        """Row-band support: append neighbouring-band vertices (distinct int16 keys [K, d]) as
        ghosts; returns, for every key, its ROW in the vertex buffers (int32 [K]).  Updates ``M``."""
        keys = np.ascontiguousarray(keys, np.int16).reshape(-1, self.d)
        vid = np.empty(len(keys), np.int32)
        _launch(self.device, "phl_add_vertices", self._h, _host(keys), len(keys), _host(vid))
        self.M = int(_call("phl_num_vertices", self._h, value=True))
        self._rows = None
        return vid

    @property
    def M_local(self):
        return int(_call("phl_num_local_vertices", self._h, value=True))

    # ---- vertex numbering ---------------------------------------------------------------------
    # keys() / replay() / neighbors() / splat_lists() speak the reference's first-touch vertex ids.  The ROWS of
    # the [M, vd] buffers splat / blur / slice exchange are in the library's internal (locality) order.
    def vertex_rows(self):
        """int64 device tensor [M]: row of first-touch vertex v in the vertex buffers (cached)."""
        hit = getattr(self, "_rows", None)
        if hit is None or hit.numel() != self.M:
            out = np.empty(self.M, np.int32)
            _call("phl_get_vertex_order", self._h, _host(out))
            hit = self._rows = torch.from_numpy(out.astype(np.int64)).to(self.device)
        return hit

    def to_first_touch(self, vert):
        """Vertex buffer with its rows re-ordered to first-touch vertex order (parity checks against the CPU path)."""
        return vert.index_select(0, self.vertex_rows())

    def from_first_touch(self, vert_ft):
        """Inverse of to_first_touch: rows in first-touch order -> a buffer in internal row order."""
        out = torch.empty_like(vert_ft)
        out.index_copy_(0, self.vertex_rows(), vert_ft)
        return out

    # ---- introspection (host copies) --------------------------------------------------------
    def pixel_order(self):
        """int32 [n]: pixels in chunk order (chunk c = pixel_order()[c*P:(c+1)*P], P = tile_stats()['pixels_per_chunk'])."""
        out = np.empty(self.n, np.int32)
        _call("phl_get_pixel_order", self._h, _host(out))
        return out

    def keys(self):
        out = np.empty((self.M, self.d), np.int16)
        _call("phl_get_keys", self._h, _host(out))
        return out

    def replay(self):
        vid = np.empty((self.n, self.d + 1), np.int32)
        w = np.empty((self.n, self.d + 1), np.float32)
        _call("phl_get_replay", self._h, _host(vid), _host(w))
        return vid, w

    def neighbors(self):
        out = np.empty((self.d + 1, self.M, 2), np.int32)
        _call("phl_get_neighbors", self._h, _host(out))
        return out

    def blur_lines(self, group=None):
        """Line lists of the three-axes-per-pass blur (phl_get_blur_lines in include/phl.h).  Without ``group``: the dict
        {groups, items, item_size} (all 0 where the lattice has none).  With it: (vertex [M] first-touch ids in line
        order along axis 3*group+2, minus [M], plus [M] flags -- 0 absent, 1 sliding, 2 evaluate --, item_start
        [items + 1])."""
        info = np.zeros(3, np.int64)
        if group is None:
            _call("phl_get_blur_lines", self._h, 0, None, None, None, _host(info))
            return dict(zip(("groups", "items", "item_size"), (int(x) for x in info)))
        items = self.blur_lines()["items"]
        vertex = np.empty(self.M, np.int32)
        flags = np.empty(self.M, np.int32)
        start = np.empty(items + 1, np.int32)
        _call("phl_get_blur_lines", self._h, int(group), _host(vertex), _host(flags), _host(start), _host(info))
        return vertex, flags & 3, (flags >> 2) & 3, start

    def splat_lists(self):
        ptr = np.empty(self.M + 1, np.int32)
        pix = np.empty(self.n * (self.d + 1), np.int32)
        w = np.empty(self.n * (self.d + 1), np.float32)
        _call("phl_get_splat_lists", self._h, _host(ptr), _host(pix), _host(w))
        return ptr, pix, w


# ---------------------------------------------------------------------------------------------
# fused elementwise steps of the mean-field iteration (crf/crf_module.py:49-52)
def _rowmajor(t):
    return t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1


def _aligned(t):
    """A row operand the compat kernels take as it is: fp32 CUDA [n, L], unit channel stride, 16-byte aligned rows."""
    return _rowmajor(t) and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def softmax_neg_add(E0, G=None, out=None):
    """softmax(-(E0 + G), dim=1) in one pass over HBM (G optional).  CUDA fp32 [n, L] only."""
    if not _rowmajor(E0) or (G is not None and (not _rowmajor(G) or G.shape != E0.shape)):
        raise TypeError("softmax_neg_add: expects fp32 CUDA [n, L] tensors with unit channel stride")
    n, L = E0.shape
    if out is None:
        out = torch.empty((n, L), dtype=torch.float32, device=E0.device)
    _launch(E0.device, "phl_softmax_neg_add", _ptr(E0), E0.stride(0), _ptr(G), G.stride(0) if G is not None else 0, _ptr(out),
            out.stride(0), n, L)
    return out


def _potts_family(Mu):
    """(alpha, beta) if Mu == alpha * ones + beta * eye exactly (the Potts family: the reference's ``potts`` layer is
    (1, -1), crf_module.py:55-64), else None.  One device -> host read."""
    L = Mu.shape[0]
    m = Mu.detach().to(torch.float32)
    if L >= 2:
        alpha = m[0, 1]
        beta = m[0, 0] - alpha
        if bool(((m - alpha) - beta * torch.eye(L, dtype=torch.float32, device=m.device) == 0).all()) and bool(torch.isfinite(m).all()):
            return (float(alpha), float(beta))
    return None


class _MuForms:
    """The forms of one compatibility matrix Mu the kernels read, each made on first use: Mu is fixed during inference.
    Holds Mu, so that its storage address cannot be recycled while the record is cached."""

    def __init__(self, Mu):
        self.Mu = Mu.detach()
        self._forms = {}

    def _form(self, key, device, make):
        hit = self._forms.get(key)
        if hit is None:
            with torch.cuda.device(device):
                hit = make()
                # cached across calls, and a later call may come on another stream: finished before anyone else can see it
                if not torch.cuda.is_current_stream_capturing():
                    torch.cuda.current_stream(device).synchronize()
            self._forms[key] = hit
        return hit

    def uniform(self):
        """_potts_family(Mu), on Mu's own device."""
        if "uniform" not in self._forms:
            self._forms["uniform"] = _potts_family(self.Mu)
        return self._forms["uniform"]

    def mu_t(self, device):
        """Mu^T as a dense fp32 device tensor padded to the MFMA tile width (zero beyond L)."""
        def make():
            L = self.Mu.shape[0]
            Lp = (L + 31) // 32 * 32
            mt = torch.zeros((Lp, Lp), dtype=torch.float32, device=device)
            mt[:L, :L] = self.Mu.to(device, torch.float32).t()
            return mt
        return self._form(("mu_t", str(device)), device, make)

    def planes(self, device):
        """Mu as the split kernels read it (phl_compat_prepare)."""
        def make():
            L = self.Mu.shape[0]
            planes = torch.empty((_call("phl_compat_planes_bytes", L, value=True),), dtype=torch.uint8, device=device)
            _launch(device, "phl_compat_prepare", _ptr(self.mu_t(device)), L, _ptr(planes))
            return planes
        return self._form(("planes", str(device)), device, make)

    def dense(self, device):
        """Mu itself as a dense fp32 [L, L] device tensor (phl_nchw_softmax_compat reads it untransposed)."""
        if self.Mu.dtype == torch.float32 and self.Mu.device == device and self.Mu.is_contiguous():
            return self.Mu
        return self._form(("dense", str(device)), device, lambda: self.Mu.to(device, torch.float32).contiguous())

    def padded(self, Lp, device):
        """(Mu with zero rows / columns up to Lp, the Potts-family structure of the ORIGINAL matrix or False): the padded
        matrix no longer shows it (crf_module._pad_labels)."""
        def make():
            L = self.Mu.shape[0]
            mp = torch.zeros((Lp, Lp), dtype=torch.float32, device=device)
            mp[:L, :L] = self.Mu.to(device, torch.float32)
            return mp
        return self._form(("padded", Lp, str(device)), device, make), self.uniform() or False


_mu_cache = {}


def _mu_forms(Mu):
    """The _MuForms record of Mu, one per (storage, version, shape, strides)."""
    key = (Mu.data_ptr(), Mu._version, tuple(Mu.shape), tuple(Mu.stride()))
    hit = _mu_cache.get(key)
    if hit is None:
        if len(_mu_cache) > 8:
            _mu_cache.clear()
        hit = _mu_cache[key] = _MuForms(Mu)
    return hit


def _mu_uniform(Mu):
    """(alpha, beta) if Mu == alpha * ones + beta * eye exactly, else None; read once per (storage, version) of Mu."""
    return _mu_forms(Mu).uniform()


def _compat_route(L, operands, Mu, uniform=None, structure=True, arith="f32"):
    """(route, uniform) of the compatibility + softmax step for these operands: "uniform" (Potts family, one streaming
    pass), "split", "f32" (the fused MFMA kernels) or "gemm" (library GEMM + fused add / softmax).
    uniform: None = look at Mu; (alpha, beta) = the caller knows it is alpha * ones + beta * eye on the labels that matter
    (a Mu padded with zero rows / columns for labels of probability 0: crf_module._pad_labels); False = it is not."""
    aligned = L % 4 == 0 and all(_aligned(t) for t in operands)
    if uniform is None:
        uniform = _mu_uniform(Mu) if (structure and aligned and L <= 1024) else None
    elif uniform is False or not (structure and aligned and L <= 1024):
        uniform = None
    if uniform is not None:
        return "uniform", uniform
    if aligned and L <= 512 and arith == "split" and _call("phl_compat_planes_bytes", L, value=True):
        return "split", None
    return ("f32" if aligned and L <= 256 else "gemm"), None


def compat_softmax(E0, X, Mu, out=None, logits=False, structure=True, arith=None, uniform=None):
    """softmax(-(E0 + X @ Mu), dim=1): the whole non-lattice half of a mean-field iteration
    (crf/crf_module.py:51-52) for fp32 CUDA E0, X [n, L] and Mu [L, L], in one fused MFMA kernel
    (phl_compat_softmax) when L % 4 == 0 and L <= 256 (label counts that are not a multiple of 32 run on a padded
    tile), or for 256 < L <= 512 with arith="split"; other label counts take a library GEMM followed by the fused
    add + softmax pass.  A Mu of the Potts family
    (alpha * ones + beta * eye, detected once per Mu; ``structure=False`` switches that off) needs no product at all:
    phl_uniform_compat_softmax streams E0, X and Q once.  logits=True returns -(E0 + X @ Mu) instead (CRFasRNN's output).
    arith: "f32" = the f32-input matrix cores (bitwise an fma chain in k order), "split" = bf16 matrix cores on operands
    split three ways, six partial products, f32 accumulation (phl_compat_softmax_split: a 256-label tile for
    128 < L <= 256, a row of L rounded up to 32 for 256 < L <= 512; the same accuracy against float64, 3/8 of the matrix
    time).  Default: "split" for L > 176 -- below that the f32 kernel is bound by its bytes as well and computes no
    padding -- unless PHL_COMPAT_ARITH names one of the two.  Above 256 labels "f32" keeps the library GEMM route.
    uniform: see _compat_route.
    Accuracy contract of arith="split" up to 256 labels (k_compat_split): its fp32 accumulators START AT E0, so every
    accumulation rounds at ulp(|E0|), where ``E0 + X @ Mu`` in torch rounds once.  With |E0| of the size of |X @ Mu| that
    is the error of an fp32 dot product; with an offset on E0 it is not -- measured (tests/test_gpu_energy_range.py,
    DESIGN.md 7.14) 4e-5 in Q at |E0| ~ 3e2 and 6e-3 at 7.65e4 (an 8-bit cost volume), 15 to 20 times torch's fp32 form.
    The softmax is shift-invariant per pixel: a caller with such energies subtracts a per-pixel constant (the row
    minimum) from E0 first, or asks for arith="f32", whose kernels start from E0 minus the row minimum themselves and
    keep torch's accuracy at any offset, as every other route does.  +inf energies (masked labels) give exactly 0
    (logits: -inf) on every route."""
    if arith is None:
        arith = os.environ.get("PHL_COMPAT_ARITH") or ("split" if E0.shape[-1] > 176 else "f32")
    if arith not in ("f32", "split"):
        raise ValueError(f"compat_softmax: arith must be 'f32' or 'split', got {arith!r}")
    if not (_rowmajor(E0) and _rowmajor(X) and X.shape == E0.shape and Mu.shape == (E0.shape[1], E0.shape[1])):
        raise TypeError("compat_softmax: expects fp32 CUDA E0, X [n, L] with unit channel stride and Mu [L, L]")
    n, L = E0.shape
    if out is None:
        out = torch.empty((n, L), dtype=torch.float32, device=E0.device)
    route, uniform = _compat_route(L, (X, E0, out), Mu, uniform, structure, arith)
    dev, flags = E0.device, 1 if logits else 0
    if route == "uniform":                       # Potts family: X @ Mu = alpha rowsum(X) + beta X, one streaming pass
        _launch(dev, "phl_uniform_compat_softmax", _ptr(E0), E0.stride(0), _ptr(X), X.stride(0), C.c_float(uniform[0]),
                C.c_float(uniform[1]), _ptr(out), out.stride(0), n, L, flags)
    elif route == "split":
        forms = _mu_forms(Mu)
        _launch(dev, "phl_compat_softmax_split", _ptr(E0), E0.stride(0), _ptr(X), X.stride(0), _ptr(forms.mu_t(dev)),
                _ptr(forms.planes(dev)), _ptr(out), out.stride(0), n, L, flags)
    elif route == "f32":
        _launch(dev, "phl_compat_softmax", _ptr(E0), E0.stride(0), _ptr(X), X.stride(0), _ptr(_mu_forms(Mu).mu_t(dev)),
                _ptr(out), out.stride(0), n, L, flags)
    else:
        G = X @ Mu.to(dev, torch.float32)
        if logits:
            return out.copy_(-(E0 + G))
        return softmax_neg_add(E0, G, out=out)
    return out


NCHW_PRODUCT, NCHW_UNIFORM, NCHW_SOFTMAX, NCHW_LOGITS = 0, 1, 2, 3       # enum phl_nchw_mode
NCHW_PRODUCT_MAX_L, NCHW_UNIFORM_MAX_L = 256, 1024


def _fp32_cuda(name, *tensors, device=None):
    """TypeError unless every one of ``tensors`` is an fp32 CUDA tensor (on ``device``, where one is given)."""
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and device in (None, t.device)):
            raise TypeError(f"{name}: takes fp32 CUDA tensors{f' on {device}' if device else ''}, got "
                            f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')}")


def _nchw_operands(name, X, G, xname):
    """(B, L, n) of the fp32 CUDA volume X [B, L, H, W] or [B, L, n] and an optional G of the same shape and device."""
    _fp32_cuda(name, *((X,) if G is None else (X, G)))
    if X.dim() not in (3, 4) or (G is not None and (G.shape != X.shape or G.device != X.device)):
        raise ValueError(f"{name}: {xname} [B, L, H, W] or [B, L, n] and G of the same shape and device")
    B, L = int(X.shape[0]), int(X.shape[1])
    return B, L, int(X[0, 0].numel()) if B and L else 0


def _out_or_empty(name, out, shape, device, what):
    """``out`` if it is a contiguous fp32 tensor of ``shape`` on ``device`` (TypeError if it is another), a new one for None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (torch.is_tensor(out) and out.is_cuda and out.is_contiguous() and out.dtype == torch.float32
            and tuple(out.shape) == tuple(shape) and out.device == device):
        raise TypeError(f"{name}: out must be a contiguous fp32 tensor of {what}")
    return out


def _step_operands(name, E0, G, Mu, out=None, *, mu_optional=False, training=False):
    """(e, g, B, L, n, out) of the channel-major step's entry points: E0 and G checked and contiguous (the caller names them:
    a copy must outlive the launch), ``out`` checked or made (_out_or_empty), Mu checked to be an [L, L] tensor (mu_optional:
    or None).  training: the operands are cut from their graph and ``out`` is left alone.  Nothing is read back."""
    B, L, n = _nchw_operands(name, E0, G, "E0")
    if not training:
        out = _out_or_empty(name, out, E0.shape, E0.device, "E0's shape and device")
    if not (Mu is None and mu_optional) and (not torch.is_tensor(Mu) or tuple(Mu.shape) != (L, L)):
        raise ValueError(f"{name}: Mu must be an [L, L] = [{L}, {L}] tensor")
    e, g = (E0.detach(), None if G is None else G.detach()) if training else (E0, G)
    return e.contiguous(), None if g is None else g.contiguous(), B, L, n, out


def nchw_softmax_compat(E0, G=None, Mu=None, *, uniform=None, logits=False, out=None):
    """The non-W half of a CRFasRNN iteration on channel-major tensors, one kernel (phl_nchw_softmax_compat):
    ``out[:, c] = sum_a Mu[a, c] * softmax(-(E0 + G), dim=1)[:, a]`` for fp32 CUDA E0, G [B, L, H, W] (or [B, L, n]; G
    optional) and Mu [L, L] in the _compat_matrix convention; Q and E never exist in memory.  Inputs that are not
    contiguous are made so.
    Mu=None: ``out = softmax(-(E0 + G), dim=1)`` (the caller runs a compatibility module of its own on it).
    uniform: (alpha, beta) = Mu is alpha * ones + beta * eye, the streaming form without a product (Mu may then be None);
    None = look at Mu, once per Mu (_mu_forms: one device -> host read, not one per call); False = it is not.
    logits=True: ``out = -(E0 + G)``, CRFasRNN's return value; G is required, Mu is not read.
    out: a contiguous fp32 tensor of E0's shape, returned.  Raises PhlError with the library's status: 1 for out aliasing
    E0 or G, 7 for more than 256 labels with a general Mu or more than 1024 with a uniform one."""
    e, g, B, L, n, out = _step_operands("nchw_softmax_compat", E0, G, None if logits else Mu, out, mu_optional=True)
    if logits:
        if G is None:
            raise ValueError("nchw_softmax_compat: logits=True needs G")
        mode, M, ab = NCHW_LOGITS, None, (0.0, 0.0)
    else:
        if uniform is None and Mu is not None and L <= NCHW_UNIFORM_MAX_L:
            uniform = _mu_forms(Mu).uniform()
        if uniform:
            mode, M, ab = NCHW_UNIFORM, None, (float(uniform[0]), float(uniform[1]))
        elif Mu is None:
            mode, M, ab = NCHW_SOFTMAX, None, (0.0, 0.0)
        else:
            mode, M, ab = NCHW_PRODUCT, _mu_forms(Mu).dense(E0.device), (0.0, 0.0)
    _launch(E0.device, "phl_nchw_softmax_compat", _ptr(e), _ptr(g), _ptr(M), C.c_float(ab[0]), C.c_float(ab[1]), _ptr(out), B, L, n, mode)
    return out


NCHW_WIDE_MAX_L = 512                # a general Mu: phl_nchw_softmax_compat_wide's range


def nchw_softmax_compat_wide(E0, G=None, Mu=None, *, out=None):
    """``nchw_softmax_compat(E0, G, Mu, uniform=False)`` for up to NCHW_WIDE_MAX_L = 512 labels, one kernel
    (phl_nchw_softmax_compat_wide): ``out[:, c] = sum_a Mu[a, c] * softmax(-(E0 + G), dim=1)[:, a]`` for fp32 CUDA E0, G
    [B, L, H, W] (or [B, L, n]; G optional) and Mu [L, L] in the _compat_matrix convention, always as a product (a Mu of
    the Potts family is not looked for).  Up to 256 labels it runs nchw_softmax_compat's kernels and gives their bits;
    above, the same scheme on a tile of 32 pixels.  Inputs that are not contiguous are made so.
    out: a contiguous fp32 tensor of E0's shape, returned.  Raises PhlError with the library's status: 1 for out aliasing
    E0 or G, 7 for more than 512 labels."""
    e, g, B, L, n, out = _step_operands("nchw_softmax_compat_wide", E0, G, Mu, out)
    M = _mu_forms(Mu).dense(E0.device)
    _launch(E0.device, "phl_nchw_softmax_compat_wide", _ptr(e), _ptr(g), _ptr(M), _ptr(out), B, L, n)
    return out


NCHW_TRAIN_MAX_L = 64                # PHL_NCHW_TRAIN_MAX_L: the label range of the training step and its backward


def nchw_step_train(E0, G=None, Mu=None, *, out=None):
    """The step of ``nchw_softmax_compat`` as training wants it, one kernel (phl_nchw_step_train), at most
    NCHW_TRAIN_MAX_L = 64 labels: ``out[:, c] = sum_a Mu[a, c] * softmax(-(E0 + G), dim=1)[:, a]`` for fp32 CUDA E0, G
    [B, L, H, W] (or [B, L, n]; G optional) and Mu [L, L] in the _compat_matrix convention, always as a product, float64
    between the fp32 loads and the one fp32 store.  Inputs that are not contiguous are made so; Mu is read on the device.
    out: a contiguous fp32 tensor of E0's shape, returned.  Raises PhlError with the library's status: 1 for out aliasing
    an input, 7 for more than 64 labels."""
    e, g, B, L, n, _ = _step_operands("nchw_step_train", E0, G, Mu, training=True)
    M = Mu.detach().to(E0.device, torch.float32).contiguous()      # (uncached: a parameter that changes every step)
    out = _out_or_empty("nchw_step_train", out, E0.shape, E0.device, "E0's shape and device")
    _launch(E0.device, "phl_nchw_step_train", _ptr(e), _ptr(g), _ptr(M), _ptr(out), B, L, n)
    return out


def nchw_step_train_grad(E0, G, Mu, gY, *, need_e=True, need_mu=True):
    """(dE, gMu) of ``nchw_step_train(E0, G, Mu)`` for the upstream gradient gY of E0's shape, one call
    (phl_nchw_step_train_grad): with Q = softmax(-(E0 + G), 1), t = Mu gY and s = sum_a Q_a t_a per pixel, ``dE = Q * (s -
    t)`` -- the gradient of E0 and of G alike -- and ``gMu[a, c] = sum over images and pixels of Q_a * gY_c``.  Only E0, G,
    Mu and gY are read: Q is recomputed.  need_e / need_mu: a part that is not needed is neither computed nor stored and
    comes back as None; the other part's bits do not depend on it.  gY that is not contiguous (autograd hands over
    expanded gradients) is made so.  Float64 sums in a fixed order: the same bits on every call."""
    e, g, B, L, n, _ = _step_operands("nchw_step_train_grad", E0, G, Mu, training=True)
    M = Mu.detach().to(E0.device, torch.float32).contiguous()      # (uncached: a parameter that changes every step)
    _fp32_cuda("nchw_step_train_grad", gY, device=E0.device)
    if gY.shape != E0.shape:
        raise ValueError(f"nchw_step_train_grad: gY must have E0's shape {tuple(E0.shape)}, got {tuple(gY.shape)}")
    if not (need_e or need_mu):
        raise ValueError("nchw_step_train_grad: nothing is asked for (need_e and need_mu are both false)")
    gy = gY.detach().contiguous()
    dE = torch.empty(E0.shape, dtype=torch.float32, device=E0.device) if need_e else None
    # (no tile, no launch: the sum over nothing)
    gMu = (torch.zeros if B * n == 0 else torch.empty)((L, L), dtype=torch.float32, device=E0.device) if need_mu else None
    _launch(E0.device, "phl_nchw_step_train_grad", _ptr(e), _ptr(g), _ptr(M), _ptr(gy), _ptr(dE), _ptr(gMu), B, L, n)
    return dE, gMu


def nchw_step_train_partials(B, L, n):
    """The number of workgroups, and of [L, L] float64 partials, of a ``nchw_step_train_grad`` that computes gMu
    (phl_nchw_step_train_partials): the 64-pixel tiles of the volume, at most 1024 -- a function of (B, L, n) alone."""
    return int(_call("phl_nchw_step_train_partials", int(B), int(L), int(n), value=True))


class NchwStepTrain(torch.autograd.Function):
    """``nchw_step_train(E0, G, Mu)`` with its backward on phl_nchw_step_train_grad.  Saves E0, G and Mu, nothing the
    forward computed.  One call per backward computes only what ``ctx.needs_input_grad`` asks for; E0 and G get the same
    gradient (one tensor, computed when either asks)."""

    @staticmethod
    def forward(ctx, E0, G, Mu):
        ctx.save_for_backward(E0, G, Mu)
        return nchw_step_train(E0, G, Mu)

    @staticmethod
    def backward(ctx, gY):
        E0, G, Mu = ctx.saved_tensors
        need_e, need_mu = any(ctx.needs_input_grad[:2]), ctx.needs_input_grad[2]
        dE = gMu = None
        if need_e or need_mu:
            dE, gMu = nchw_step_train_grad(E0, G, Mu, gY, need_e=need_e, need_mu=need_mu)
            if need_mu:
                gMu = gMu.to(Mu.dtype)
        return (dE if ctx.needs_input_grad[0] else None), (dE if ctx.needs_input_grad[1] else None), gMu


def nchw_step_train_fn(E0, G=None, Mu=None):
    """Differentiable ``nchw_step_train``: NchwStepTrain.apply(E0, G, Mu)."""
    return NchwStepTrain.apply(E0, G, Mu)


NCHW_EXPECT_PIXELS = 1024            # PHL_NCHW_EXPECT_PIXELS: pixels of a workgroup of the expected-label kernels


def _expect_operands(name, X, G, labels):
    """(X, G contiguous, labels as fp32 [L] on X's device or None, B, L, n) of the expected-label entry points."""
    B, L, n = _nchw_operands(name, X, G, "X")
    if labels is not None:
        labels = torch.as_tensor(labels)
        if labels.numel() != L:
            raise ValueError(f"{name}: labels must hold one value per label channel ({L}), got shape {tuple(labels.shape)}")
        labels = labels.detach().reshape(L).to(X.device, torch.float32).contiguous()
    return X.contiguous(), None if G is None else G.contiguous(), labels, B, L, n


def nchw_expected_value(X, G=None, labels=None, *, negate=False, out=None):
    """The expected label of channel-major columns, one kernel (phl_nchw_expected_value):
    ``(softmax(sign * (X + G), dim=1) * labels[None, :, None, None]).sum(1, keepdim=True)``, sign = -1 with ``negate``
    (the mean-field loop's E0 and G) and +1 without (plain logits), for fp32 CUDA X, G [B, L, H, W] -> [B, 1, H, W] (or
    [B, L, n] -> [B, 1, n]; G optional).  X and G are read once; neither the probabilities nor the logits are written.
    Any L >= 1.  Inputs that are not contiguous are made so.
    labels: None = 0, 1, .., L-1; else [L] or anything with L elements ([1, L, 1, 1]), converted to fp32 on X's device;
    anything else (labels per pixel) is a ValueError.  out: a contiguous fp32 tensor of the result's shape, returned."""
    x, g, lab, B, L, n = _expect_operands("nchw_expected_value", X, G, labels)
    shape = (B, 1) + tuple(X.shape[2:])
    out = _out_or_empty("nchw_expected_value", out, shape, X.device, f"shape {shape} on X's device")
    _launch(X.device, "phl_nchw_expected_value", _ptr(x), _ptr(g), _ptr(lab), _ptr(out), B, L, n, 1 if negate else 0)
    return out


def nchw_expected_value_grad(X, G, labels, gout, *, negate=False):
    """gZ = sign * gout * q * (labels - d) with q = softmax(sign * (X + G), dim=1) and d = nchw_expected_value(X, G,
    labels): the gradient of X and of G alike, of X's shape (phl_nchw_expected_value_grad).  gout: the upstream gradient,
    fp32 CUDA with one element per pixel ([B, 1, H, W]).  Only X, G and the labels are read: the column's statistics are
    recomputed.  Same bits on every call."""
    x, g, lab, B, L, n = _expect_operands("nchw_expected_value_grad", X, G, labels)
    _fp32_cuda("nchw_expected_value_grad", gout, device=X.device)
    if gout.numel() != B * n:
        raise ValueError(f"nchw_expected_value_grad: gout must hold one value per pixel ({B} x {n}), got {tuple(gout.shape)}")
    go = gout.contiguous()
    gZ = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    _launch(X.device, "phl_nchw_expected_value_grad", _ptr(x), _ptr(g), _ptr(lab), _ptr(go), _ptr(gZ), B, L, n, 1 if negate else 0)
    return gZ


class NchwExpectedValue(torch.autograd.Function):
    """``nchw_expected_value(X, G, labels, negate=negate)`` with its backward on phl_nchw_expected_value_grad.  Saves X, G
    and the labels, nothing the forward computed.  X and G get the same gradient (one tensor, computed when either asks);
    the labels get none."""

    @staticmethod
    def forward(ctx, X, G=None, labels=None, negate=False):
        ctx.negate = bool(negate)
        labels = None if labels is None else torch.as_tensor(labels)
        ctx.save_for_backward(X, G, labels)
        return nchw_expected_value(X, G, labels, negate=negate)

    @staticmethod
    def backward(ctx, g):
        X, G, labels = ctx.saved_tensors
        gZ = nchw_expected_value_grad(X, G, labels, g, negate=ctx.negate) if any(ctx.needs_input_grad[:2]) else None
        return (gZ if ctx.needs_input_grad[0] else None), (gZ if ctx.needs_input_grad[1] else None), None, None


def nchw_expected_value_fn(X, G=None, labels=None, negate=False):
    """Differentiable ``nchw_expected_value``: NchwExpectedValue.apply(X, G, labels, negate)."""
    return NchwExpectedValue.apply(X, G, labels, negate)


# ---------------------------------------------------------------------------------------------
# the upsampler head's unaries from a scalar disparity (crf/mb_stereo_crf.py; include/phl.h, phl_nchw_scalar.hip)
NCHW_SCALAR_PIXELS = 1024            # PHL_NCHW_SCALAR_PIXELS: pixels of a workgroup of the scalar-unary kernels


def _scalar_operands(name, disp, size, L, gamma, s):
    """(disp contiguous, gamma, s, B, h, w, H, W, L) of the scalar-unary entry points: disp fp32 CUDA [B, 1, h, w] with at
    least one element, gamma and s fp32 tensors of one element on its device (read there, never on the host)."""
    _fp32_cuda(name, disp, gamma, s)
    if disp.dim() != 4 or disp.shape[1] != 1 or disp.numel() == 0:
        raise ValueError(f"{name}: disp must be a non-empty [B, 1, h, w], got {tuple(disp.shape)}")
    if gamma.numel() != 1 or s.numel() != 1 or gamma.device != disp.device or s.device != disp.device:
        raise ValueError(f"{name}: gamma and s must hold one value each on disp's device")
    H, W = (int(v) for v in size)
    L = int(L)
    if L < 2 or H < 1 or W < 1:
        raise ValueError(f"{name}: needs L >= 2 and an output size >= 1 x 1, got L={L}, size={(H, W)}")
    B, _, h, w = (int(v) for v in disp.shape)
    return disp.detach().contiguous(), gamma.detach(), s.detach(), B, h, w, H, W, L


def nchw_scalar_unaries(disp, size, L, gamma, s, *, scale=10.0, threshold=1e-2):
    """(E0 [B, L, H, W], labels [L]) of the upsampler head in two launches, nothing read back on the host
    (phl_nchw_scalar_unaries): with ``up = F.interpolate(disp, size, mode="bilinear", align_corners=False)`` (evaluated in
    float64 per output pixel, never written), ``lmax = up.max()`` and ``labels = linspace(0, lmax, L)``,

        E0 = scale * exp(s) * (sqrt(g^2 + (labels[a] - up)^2) - g) * (up > threshold),      g = gamma * lmax

    -- CRFasRNN's ``-logits * confidence`` for the head's ``logits = -10 * charb.get_energies_from_scalar(up, labels)`` and
    ``confidence = (up > 1e-2).float()``.  disp: fp32 CUDA [B, 1, h, w]; size: (H, W), any ratio; gamma, s: fp32 CUDA tensors
    of one element (charb's parameters), read on the device.  Float64 between the loads and the one fp32 store."""
    d, gm, sv, B, h, w, H, W, L = _scalar_operands("nchw_scalar_unaries", disp, size, L, gamma, s)
    E0 = torch.empty((B, L, H, W), dtype=torch.float32, device=disp.device)
    labels = torch.empty((L,), dtype=torch.float32, device=disp.device)
    _launch(disp.device, "phl_nchw_scalar_unaries", _ptr(d), _ptr(gm), _ptr(sv), _ptr(E0), _ptr(labels), B, h, w, H, W, L,
            float(scale), float(threshold))
    return E0, labels


def nchw_scalar_unaries_grad(disp, size, labels, gamma, s, gE0, *, scale=10.0, threshold=1e-2):
    """(grad_gamma, grad_s), 0-dim fp32, of ``nchw_scalar_unaries`` for the upstream gradient gE0 [B, L, H, W]
    (phl_nchw_scalar_unaries_grad).  labels: the forward's.  gE0 is read once and everything else recomputed from the
    forward's inputs; float64 sums in a fixed order, the same bits on every call.  There is no gradient for disp."""
    _fp32_cuda("nchw_scalar_unaries_grad", labels)
    if labels.dim() != 1:
        raise TypeError("nchw_scalar_unaries_grad: labels must be the [L] tensor the forward returned")
    d, gm, sv, B, h, w, H, W, L = _scalar_operands("nchw_scalar_unaries_grad", disp, size, labels.numel(), gamma, s)
    _fp32_cuda("nchw_scalar_unaries_grad", gE0, labels, device=disp.device)
    if tuple(gE0.shape) != (B, L, H, W):
        raise ValueError(f"nchw_scalar_unaries_grad: gE0 must be {(B, L, H, W)}, got {tuple(gE0.shape)}")
    grad = torch.empty((2,), dtype=torch.float32, device=disp.device)
    _launch(disp.device, "phl_nchw_scalar_unaries_grad", _ptr(d), _ptr(labels.detach().contiguous()), _ptr(gm), _ptr(sv),
            _ptr(gE0.detach().contiguous()), _ptr(grad), B, h, w, H, W, L, float(scale), float(threshold))
    return grad[0], grad[1]


class NchwScalarUnaries(torch.autograd.Function):
    """``nchw_scalar_unaries`` with its backward on phl_nchw_scalar_unaries_grad: gradients for gamma and s, none for
    disp; the labels are marked non-differentiable (the reference's ``float(up.max())`` cuts their graph).  Saves disp,
    the labels, gamma and s -- nothing of E0's size."""

    @staticmethod
    def forward(ctx, disp, size, L, gamma, s, scale=10.0, threshold=1e-2):
        E0, labels = nchw_scalar_unaries(disp, size, L, gamma, s, scale=scale, threshold=threshold)
        ctx.size, ctx.scale, ctx.threshold = tuple(size), scale, threshold
        ctx.save_for_backward(disp, labels, gamma, s)
        ctx.mark_non_differentiable(labels)
        return E0, labels

    @staticmethod
    def backward(ctx, gE0, _glabels):
        disp, labels, gamma, s = ctx.saved_tensors
        gg = gs = None
        if any(ctx.needs_input_grad[3:5]):
            gg, gs = nchw_scalar_unaries_grad(disp, ctx.size, labels, gamma, s, gE0, scale=ctx.scale, threshold=ctx.threshold)
            gg, gs = gg.reshape(gamma.shape), gs.reshape(s.shape)
        return (None, None, None, gg if ctx.needs_input_grad[3] else None, gs if ctx.needs_input_grad[4] else None, None, None)


def nchw_scalar_unaries_fn(disp, size, L, gamma, s, scale=10.0, threshold=1e-2):
    """Differentiable ``nchw_scalar_unaries``: NchwScalarUnaries.apply(disp, size, L, gamma, s, scale, threshold)."""
    return NchwScalarUnaries.apply(disp, size, L, gamma, s, scale, threshold)


# ---------------------------------------------------------------------------------------------
# the unaries from logits and a per-pixel confidence (crf/crf_module.py, CRFasRNN; include/phl.h, phl_nchw_conf.hip)
NCHW_CONF_PIXELS = 1024              # PHL_NCHW_CONF_PIXELS: pixels of a workgroup of the confidence-unary kernels


def _confidence_operands(name, logits, confidence):
    """(logits, confidence contiguous and cut from their graph, B, L, n) of the confidence-unary entry points: fp32 CUDA
    logits [B, L, H, W] or [B, L, n] and a confidence [B, 1, H, W] / [B, 1, n] on the same device."""
    B, L, n = _nchw_operands(name, logits, None, "logits")
    _fp32_cuda(name, confidence, device=logits.device)
    if tuple(confidence.shape) != (B, 1) + tuple(logits.shape[2:]):
        raise ValueError(f"{name}: confidence must be {(B, 1) + tuple(logits.shape[2:])} for logits {tuple(logits.shape)}, "
                         f"got {tuple(confidence.shape)}")
    return logits.detach().contiguous(), confidence.detach().contiguous(), B, L, n


def nchw_confidence_unaries(logits, confidence, *, out=None):
    """CRFasRNN's unaries ``-logits * confidence`` in one kernel that reads the logits once (phl_nchw_confidence_unaries),
    for fp32 CUDA logits [B, L, H, W] (or [B, L, n]) and a confidence [B, 1, H, W] ([B, 1, n]) on the same device: the bits
    of the torch line on finite inputs, signed zeros included.  Any L >= 1.  Inputs that are not contiguous are made so.
    out: a contiguous fp32 tensor of the logits' shape, returned."""
    x, c, B, L, n = _confidence_operands("nchw_confidence_unaries", logits, confidence)
    out = _out_or_empty("nchw_confidence_unaries", out, logits.shape, logits.device, "the logits' shape and device")
    _launch(logits.device, "phl_nchw_confidence_unaries", _ptr(x), _ptr(c), _ptr(out), B, L, n)
    return out


def nchw_confidence_unaries_grad(logits, confidence, gE0, *, need_conf=True, need_logits=False):
    """(grad_conf, grad_logits) of ``nchw_confidence_unaries(logits, confidence)`` for the upstream gradient gE0 of the
    logits' shape, one kernel (phl_nchw_confidence_unaries_grad): ``grad_conf = -(logits * gE0).sum(1, keepdim=True)`` with
    the products and the sum in float64, in label order, stored as fp32 once, and ``grad_logits = -(confidence * gE0)``,
    the bits of fp32 autograd.  need_conf / need_logits: a part that is not needed is neither computed nor stored and comes
    back as None; the other part's bits do not depend on it.  gE0 is read once, the logits only for grad_conf, the
    confidence only for grad_logits.  gE0 that is not contiguous is made so.  The same bits on every call."""
    x, c, B, L, n = _confidence_operands("nchw_confidence_unaries_grad", logits, confidence)
    _fp32_cuda("nchw_confidence_unaries_grad", gE0, device=logits.device)
    if gE0.shape != logits.shape:
        raise ValueError(f"nchw_confidence_unaries_grad: gE0 must have the logits' shape {tuple(logits.shape)}, got {tuple(gE0.shape)}")
    if not (need_conf or need_logits):
        raise ValueError("nchw_confidence_unaries_grad: nothing is asked for (need_conf and need_logits are both false)")
    ge = gE0.detach().contiguous()
    gc = torch.empty(confidence.shape, dtype=torch.float32, device=logits.device) if need_conf else None
    gl = torch.empty(logits.shape, dtype=torch.float32, device=logits.device) if need_logits else None
    _launch(logits.device, "phl_nchw_confidence_unaries_grad", _ptr(x), _ptr(c), _ptr(ge), _ptr(gc), _ptr(gl), B, L, n)
    return gc, gl


class NchwConfidenceUnaries(torch.autograd.Function):
    """``nchw_confidence_unaries(logits, confidence)`` with its backward on phl_nchw_confidence_unaries_grad.  Saves the
    logits and the confidence, nothing the forward computed -- no ``-logits`` lives until the backward.  One call per
    backward computes only what ``ctx.needs_input_grad`` asks for."""

    @staticmethod
    def forward(ctx, logits, confidence):
        ctx.save_for_backward(logits, confidence)
        return nchw_confidence_unaries(logits, confidence)

    @staticmethod
    def backward(ctx, gE0):
        logits, confidence = ctx.saved_tensors
        need_logits, need_conf = ctx.needs_input_grad
        gc = gl = None
        if need_conf or need_logits:
            gc, gl = nchw_confidence_unaries_grad(logits, confidence, gE0, need_conf=need_conf, need_logits=need_logits)
        return gl, gc


def nchw_confidence_unaries_fn(logits, confidence):
    """Differentiable ``nchw_confidence_unaries``: NchwConfidenceUnaries.apply(logits, confidence)."""
    return NchwConfidenceUnaries.apply(logits, confidence)


# ---------------------------------------------------------------------------------------------
# backward of the compatibility + softmax step (CRF training; include/phl.h, phl_compat_grad.hip)
def _grad_operand(t, n, L):
    """fp32 CUDA [n, L] with unit channel stride and 16-byte aligned rows, as the backward kernels read it."""
    if not (t.shape == (n, L) and _aligned(t)):
        t = t.to(torch.float32).clone(memory_format=torch.contiguous_format)
    return t


def _mu_operand(Mu, L, device):
    """Mu as phl_compat_grad_x reads it: a dense fp32 [L][L] with row stride L (the ABI takes no stride for Mu), 16-byte
    aligned -- a row-padded or offset view is copied."""
    if tuple(Mu.shape) != (L, L):
        raise TypeError(f"compat_grad_x: Mu must be [{L}, {L}], got {tuple(Mu.shape)}")
    m = Mu.detach().to(device, torch.float32)
    if not (m.shape == (L, L) and m.stride() == (L, 1) and m.data_ptr() % 16 == 0):
        m = m.clone(memory_format=torch.contiguous_format)
    return m


def _check_grad_domain(name, L, *tensors):
    """The backward kernels take fp32 CUDA operands with L % 4 == 0 and 4 <= L <= 512: checked when the forward records
    a graph, so that an input the backward cannot take fails there, with this message, not at backward time."""
    for t in tensors:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32):
            raise TypeError(f"{name}: the differentiable form takes fp32 CUDA tensors, got {t.dtype} on {t.device}")
    if not (L % 4 == 0 and 4 <= L <= 512):
        raise ValueError(f"{name}: the backward kernels take L % 4 == 0 and 4 <= L <= 512 labels, got L = {L} "
                         "(pad the labels, as crf_module._label_pad does, or use the plain torch ops)")


def softmax_neg_grad(Q, gQ, out=None):
    """dE = Q * (sum_c gQ Q - gQ): the gradient of Q = softmax(-E) with respect to E, one pass (phl_softmax_neg_grad)."""
    n, L = Q.shape
    Q, gQ = _grad_operand(Q, n, L), _grad_operand(gQ, n, L)
    if out is None:
        out = torch.empty((n, L), dtype=torch.float32, device=Q.device)
    _launch(Q.device, "phl_softmax_neg_grad", _ptr(Q), Q.stride(0), _ptr(gQ), gQ.stride(0), _ptr(out), out.stride(0), n, L)
    return out


def uniform_compat_grad(Q, gQ, alpha, beta):
    """(dE, gX) for Mu = alpha * ones + beta * eye in one pass (phl_uniform_compat_grad).  Q = None: logits mode,
    dE = -gQ."""
    n, L = gQ.shape
    gQ = _grad_operand(gQ, n, L)
    if Q is not None:
        Q = _grad_operand(Q, n, L)
    dE = torch.empty((n, L), dtype=torch.float32, device=gQ.device)
    gX = torch.empty_like(dE)
    _launch(gQ.device, "phl_uniform_compat_grad", _ptr(Q), Q.stride(0) if Q is not None else 0, _ptr(gQ), gQ.stride(0),
            C.c_float(alpha), C.c_float(beta), _ptr(dE), dE.stride(0), _ptr(gX), gX.stride(0), n, L)
    return dE, gX


def compat_grad_x(dE, Mu, scale=1.0):
    """scale * dE @ Mu^T on the f32-input matrix cores (phl_compat_grad_x); Mu is [L, L] as the forward takes it."""
    n, L = dE.shape
    dE = _grad_operand(dE, n, L)
    Mu = _mu_operand(Mu, L, dE.device)
    gX = torch.empty((n, L), dtype=torch.float32, device=dE.device)
    _launch(dE.device, "phl_compat_grad_x", _ptr(dE), dE.stride(0), _ptr(Mu), C.c_float(scale), _ptr(gX), gX.stride(0), n, L)
    return gX


def compat_mu_grad(X, dE, scale=1.0, out=None, accumulate=False):
    """scale * X^T @ dE as a dense [L, L] (phl_compat_mu_grad): per-range fp32 partials in a workspace, summed in a fixed
    order in fp64 -- the same bits on every run.  accumulate=True adds to ``out``."""
    n, L = dE.shape
    X, dE = _grad_operand(X, n, L), _grad_operand(dE, n, L)
    if out is None:
        out = torch.empty((L, L), dtype=torch.float32, device=dE.device)
        accumulate = False
    elif not (out.is_contiguous() and out.dtype == torch.float32 and out.shape == (L, L)):
        raise TypeError("compat_mu_grad: out must be a contiguous fp32 [L, L] tensor")
    ws = torch.empty((max(1, _call("phl_compat_mu_grad_workspace_bytes", n, L, value=True)),), dtype=torch.uint8, device=dE.device)
    _launch(dE.device, "phl_compat_mu_grad", _ptr(X), X.stride(0), _ptr(dE), dE.stride(0), C.c_float(scale), n, L, _ptr(ws), _ptr(out),
            1 if accumulate else 0)
    return out


class SoftmaxNegAdd(torch.autograd.Function):
    """Q = softmax(-(E0 + G)) (phl_softmax_neg_add; G optional) with its backward on phl_softmax_neg_grad: the first
    step of a differentiable mean-field loop, and the step of one that applies W after Mu (CRFasRNN)."""

    @staticmethod
    def forward(ctx, E0, G=None):
        if any(ctx.needs_input_grad):
            _check_grad_domain("SoftmaxNegAdd", E0.shape[-1], E0, G)
        E0 = E0 if _rowmajor(E0) else E0.contiguous()
        if G is not None and not _rowmajor(G):
            G = G.contiguous()
        Q = softmax_neg_add(E0, G)
        ctx.save_for_backward(Q)
        return Q

    @staticmethod
    def backward(ctx, g):
        Q, = ctx.saved_tensors
        dE = softmax_neg_grad(Q, g) if any(ctx.needs_input_grad[:2]) else None
        return (dE if ctx.needs_input_grad[0] else None), (dE if ctx.needs_input_grad[1] else None)


class CompatProduct(torch.autograd.Function):
    """Y = Q @ M on the f32 matrix cores (phl_compat_grad_x with M^T), backward gQ = gY M^T (phl_compat_grad_x) and
    gM = Q^T gY (phl_compat_mu_grad), each only when asked for.  The compatibility applied BEFORE W, as CRFasRNN does
    (``W(Mu(Q))``, crf_module.py:98): with a W whose backward is taken to be W itself (the lattice filter), the gradient
    of M then is the one the reference computes."""

    @staticmethod
    def forward(ctx, Q, M):
        _check_grad_domain("CompatProduct", Q.shape[-1], Q, M)
        ctx.save_for_backward(Q, M)
        return compat_grad_x(Q, M.detach().t().contiguous())

    @staticmethod
    def backward(ctx, gY):
        Q, M = ctx.saved_tensors
        gQ = compat_grad_x(gY, M) if ctx.needs_input_grad[0] else None
        gM = compat_mu_grad(Q, gY) if ctx.needs_input_grad[1] else None
        return gQ, gM


class CompatSoftmax(torch.autograd.Function):
    """softmax(-(E0 + X @ Mu)) (or its logits -(E0 + X @ Mu)) on the fused forward kernels of ``compat_softmax``, with
    the backward on the library's kernels: dE in one pass over Q and the incoming gradient (phl_softmax_neg_grad),
    gX = dE Mu^T and gMu = X^T dE on the f32 matrix cores (phl_compat_grad_x, phl_compat_mu_grad).  A Mu of the Potts
    family detected on Mu itself gets dE and gX from one streaming pass (phl_uniform_compat_grad).  Only the gradients
    autograd asks for are computed.  The forward writes a fresh tensor; it saves Q (not in logits mode), X and Mu.

    uniform: as for ``compat_softmax``; a structure the caller asserts for the labels that matter (a padded Mu) serves
    the forward only -- the backward then takes the dense product, whose padding columns are exactly 0.  The backward
    takes the Potts-family shortcut only for a structure detected on Mu itself.

    Domain when a gradient is recorded: fp32 CUDA E0, X, Mu and L % 4 == 0, 4 <= L <= 512 (else TypeError / ValueError in
    the forward); without one, everything ``compat_softmax`` takes."""

    @staticmethod
    def forward(ctx, E0, X, Mu, logits=False, uniform=None):
        if any(ctx.needs_input_grad[:3]):
            _check_grad_domain("CompatSoftmax", E0.shape[-1], E0, X, Mu)
        E0 = E0 if _rowmajor(E0) else E0.contiguous()
        X = X if _rowmajor(X) else X.contiguous()
        _, found = _compat_route(E0.shape[1], (X, E0), Mu, uniform)
        out = compat_softmax(E0, X, Mu, logits=logits, uniform=found or False)
        ctx.logits, ctx.uniform = bool(logits), (found if uniform is None else None)
        ctx.save_for_backward(None if logits else out, X, Mu)
        return out

    @staticmethod
    def backward(ctx, g):
        Q, X, Mu = ctx.saved_tensors
        need_e0, need_x, need_mu = ctx.needs_input_grad[:3]
        n, L = g.shape
        g = _grad_operand(g, n, L)
        gE0 = gX = gMu = None
        uni = ctx.uniform if need_x else None
        if ctx.logits:                           # out = -E: dE = -g; the products take g with scale -1
            if uni is not None:
                dE, gX = uniform_compat_grad(None, g, *uni)
                gE0 = dE if need_e0 else None
            else:
                gE0 = -g if need_e0 else None
                if need_x:
                    gX = compat_grad_x(g, Mu, -1.0)
            if need_mu:
                gMu = compat_mu_grad(X, g, -1.0)
        else:
            if uni is not None:
                dE, gX = uniform_compat_grad(Q, g, *uni)
            else:
                dE = softmax_neg_grad(Q, g)
                if need_x:
                    gX = compat_grad_x(dE, Mu, 1.0)
            gE0 = dE if need_e0 else None
            if need_mu:
                gMu = compat_mu_grad(X, dE, 1.0)
        if gMu is not None and gMu.dtype != Mu.dtype:
            gMu = gMu.to(Mu.dtype)
        return gE0, gX, gMu, None, None


def compat_softmax_fn(E0, X, Mu, logits=False, uniform=None):
    """Differentiable ``compat_softmax``: CompatSoftmax.apply(E0, X, Mu, logits, uniform).  With a gradient recorded it
    takes fp32 CUDA tensors and L % 4 == 0, 4 <= L <= 512 (the backward kernels' range), and says so in the forward."""
    return CompatSoftmax.apply(E0, X, Mu, logits, uniform)


def softmax_neg_add_fn(E0, G=None):
    """Differentiable ``softmax_neg_add(E0, G)``: SoftmaxNegAdd.apply(E0, G)."""
    return SoftmaxNegAdd.apply(E0, G)


def compat_product_fn(Q, M):
    """Differentiable Q @ M on the library's kernels: CompatProduct.apply(Q, M)."""
    return CompatProduct.apply(Q, M)


CRITERIA = {"AD": 0, "SD": 1, "nprod": 2}


def cost_volume(img1, img2, max_disp=None, window_size=9, criterion="AD", out=None):
    """Unary stereo cost volume on the device: the reference's ``disparity_badness(img1, img2, window_size,
    criterion)`` (crf/depth.py:36-53), returned as E_0 [h*w, max_disp] fp32 pixel-major (what
    ``mean_field_infer`` takes after the notebook's reshape, DenseCrf.ipynb cell 7).
    img1/img2: [h, w, c] float tensors or numpy arrays; max_disp defaults to w // 6 (:40)."""
    a, b = _sweep_views("cost_volume", img1, img2, False)
    _, h, w, c = (int(v) for v in a.shape)
    L, crit = _sweep_request(w, max_disp, criterion)
    dev = _sweep_device(img1)
    a, b = (v.to(device=dev, dtype=torch.float32).contiguous() for v in (a, b))      # the kernel's ABI is dense [h, w, c]
    res = torch.empty((h * w, L), dtype=torch.float32, device=dev) if out is None else out
    assert res.shape == (h * w, L) and res.stride(1) == 1 and res.dtype == torch.float32
    _launch(dev, "phl_cost_volume", _ptr(a), _ptr(b), h, w, c, L, int(window_size), crit, _ptr(res), res.stride(0) if L else 0)
    return res


COSTVOL_NEGATE = 1                   # PHL_COSTVOL_NEGATE
COSTVOL_NCHW_TILE = (64, 8, 8)       # (PHL_COSTVOL_NCHW_TX, _TY, _DC): pixels in x, pixels in y, disparities of a workgroup


def _sweep_views(name, img1, img2, channels_first):
    """Both images of a sweep as [B, H, W, C] views of what the caller passed (no GPU needed): [H, W] / [H, W, C] arrays
    or tensors are one pair, [B, C, H, W] tensors with ``channels_first``."""
    def view(v):
        t = torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v)
        if channels_first:
            return t.permute(0, 2, 3, 1) if t.dim() == 4 else None
        t = t[..., None] if t.dim() == 2 else t
        return t[None] if t.dim() == 3 else None

    a, b = view(img1), view(img2)
    if a is None or b is None or a.shape != b.shape:
        form = "[B, C, H, W]" if channels_first else "[H, W, C] or [H, W]"
        raise ValueError(f"{name}: images must both be {form}, got {tuple(np.shape(img1))} and {tuple(np.shape(img2))}")
    return a, b


def _sweep_operands(a, b, dev):
    """fp32 tensors on ``dev`` with one set of strides: an fp32 CUDA tensor stays where it is, whatever its strides; the
    second image is copied into the first one's layout only if the two differ."""
    a, b = a.to(device=dev, dtype=torch.float32), b.to(device=dev, dtype=torch.float32)
    if any(n > 1 and sa != sb for n, sa, sb in zip(a.shape, a.stride(), b.stride())):
        b = torch.empty_strided(a.shape, a.stride(), dtype=torch.float32, device=dev).copy_(b)
    return a, b, tuple(int(v) for v in a.shape), tuple(int(s) for s in a.stride())


def _sweep_device(img1):
    _require_gpu()
    return _default_device(img1)


def _sweep_request(w, max_disp, criterion):
    """(max_disp, criterion code): max_disp defaults to w // 6 (crf/depth.py:40), a criterion is one of CRITERIA's names
    or the reference's function of that name."""
    return (w // 6 if max_disp is None else int(max_disp)), CRITERIA[getattr(criterion, "__name__", criterion)]


def cost_volume_nchw(img1, img2, max_disp=None, window_size=9, criterion="AD", negate=False, out=None, channels_first=False):
    """The cost volume of ``cost_volume`` in the channel-major layout of CRFasRNN and the heads: fp32 [B, L, H, W], written
    once (csrc/phl_costvol_nchw.hip).  ``negate=True`` gives the reference's unary logits, ``-1 * disparity_badness``
    permuted to [L, H, W] (crf/dataloader.py:54-57,83).  Images: [H, W, C] / [H, W] numpy or torch (B = 1), or
    [B, C, H, W] torch tensors with ``channels_first=True``; fp32 CUDA tensors are read through their strides without a
    copy.  ``out``: any fp32 CUDA view [B, L, H, W] with unit x stride.  max_disp defaults to w // 6 (crf/depth.py:40)."""
    a, b = _sweep_views("cost_volume_nchw", img1, img2, channels_first)
    B, h, w, c = (int(v) for v in a.shape)
    L, crit = _sweep_request(w, max_disp, criterion)
    if out is not None and (tuple(out.shape) != (B, L, h, w) or out.dtype != torch.float32 or (w > 1 and out.stride(3) != 1)):
        raise ValueError(f"cost_volume_nchw: out must be fp32 [{B}, {L}, {h}, {w}] with unit x stride, got {out.dtype} "
                         f"{tuple(out.shape)} with strides {tuple(out.stride())}")
    dev = _sweep_device(img1)
    if out is not None and out.device != dev:
        raise ValueError(f"cost_volume_nchw: out is on {out.device}, the images on {dev}")
    a, b, _, (ibs, iys, ixs, ics) = _sweep_operands(a, b, dev)
    res = torch.empty((B, L, h, w), dtype=torch.float32, device=dev) if out is None else out
    _launch(dev, "phl_cost_volume_nchw", _ptr(a), _ptr(b), B, h, w, c, ibs, iys, ixs, ics, L, int(window_size), crit,
            COSTVOL_NEGATE if negate else 0, _ptr(res), res.stride(0), res.stride(1), res.stride(2))
    return res


def disparity_wta(img1, img2, max_disp=None, window_size=9, criterion="AD", return_cost=False, channels_first=False):
    """Winner-takes-all disparity of the same sweep, the reference's ``disparity_estimate`` (crf/depth.py:31-34): int32
    [B, H, W], the smallest disparity of minimal cost as ``np.argmin`` gives it, and with ``return_cost`` the fp32 minimum
    beside it -- the argmin / min of ``cost_volume_nchw`` bit for bit, without the volume (4 bytes per pixel, not 4 L)."""
    a, b = _sweep_views("disparity_wta", img1, img2, channels_first)
    B, h, w, c = (int(v) for v in a.shape)
    L, crit = _sweep_request(w, max_disp, criterion)
    if L == 0:
        raise ValueError("disparity_wta: max_disp = 0, an argmin over nothing")
    dev = _sweep_device(img1)
    a, b, _, (ibs, iys, ixs, ics) = _sweep_operands(a, b, dev)
    disp = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    cost = torch.empty((B, h, w), dtype=torch.float32, device=dev) if return_cost else None
    _launch(dev, "phl_disparity_wta", _ptr(a), _ptr(b), B, h, w, c, ibs, iys, ixs, ics, L, int(window_size), crit,
            _ptr(disp), _ptr(cost), disp.stride(0), disp.stride(1))
    return (disp, cost) if return_cost else disp


# ---------------------------------------------------------------------------------------------
# separable Gaussian of the guided filter (crf/guided.py; include/phl.h, phl_blur.hip)
def _blur_view(x, dim):
    """(outer, h, inner) of a contiguous tensor along ``dim`` (non-negative, as the reference takes it)."""
    if not 0 <= dim < x.dim():
        raise ValueError(f"box_blur: dim must be in 0..{x.dim() - 1}, got {dim}")
    shape = tuple(int(s) for s in x.shape)
    outer = int(np.prod(shape[:dim], dtype=np.int64))
    inner = int(np.prod(shape[dim + 1:], dtype=np.int64))
    return outer, shape[dim], inner


def _blur_operand(t):
    _fp32_cuda("box_blur", t)
    return t if t.is_contiguous() else t.contiguous()


def box_blur(x, r, dim, passes=3, out=None):
    """``passes`` normalised box passes of radius r along ``dim`` (phl_box_blur): one kernel for the whole cascade while
    its LDS fits, one launch per pass above that.  fp32 CUDA; any strides (copied contiguous)."""
    x = _blur_operand(x)
    outer, h, inner = _blur_view(x, dim)
    out = _out_or_empty("box_blur", out, x.shape, x.device, "the input's shape and device")
    _launch(x.device, "phl_box_blur", _ptr(x), _ptr(out), outer, h, inner, int(r), int(passes))
    return out


def box_blur_fused_max_r(inner_is_one, passes=3, grad=False):
    """Largest r that the fused cascade kernel (grad=True: the fused sigma-gradient) takes."""
    return int(_call("phl_box_blur_fused_max_r", 1 if inner_is_one else 0, int(passes), 1 if grad else 0, value=True))


def box_blur_grad(v, g, r, dim, sigma, need_x=True, need_sigma=True):
    """Backward of the 3-pass Gaussian (phl_box_blur_grad): (grad_x = B(g) or None, grad_sigma as a 0-d fp32 device
    tensor or None).  Without need_sigma only the plain cascade on g runs.  Above the fused kernel's radius the four
    cascades g, g f, v, v f run as box_blur calls and the contraction as fp64 torch ops."""
    v, g = _blur_operand(v), _blur_operand(g)
    if v.shape != g.shape or v.device != g.device:
        raise ValueError("box_blur_grad: v and g must have the same shape and device")
    if not need_sigma:
        return (box_blur(g, r, dim) if need_x else None), None
    outer, h, inner = _blur_view(v, dim)
    gx = torch.empty_like(v) if need_x else None
    gs = torch.empty((), dtype=torch.float32, device=v.device)
    try:
        _launch(v.device, "phl_box_blur_grad", _ptr(v), _ptr(g), outer, h, inner, int(r), C.c_double(float(sigma)), _ptr(gx),
                _ptr(gs))
        return gx, gs
    except PhlError as e:
        if e.status != ERR_UNSUPPORTED:          # r above the fused kernel's limit
            raise
    shape = (1,) * dim + (h,) + (1,) * (v.dim() - dim - 1)
    f = (torch.arange(h, device=v.device, dtype=torch.float64) / float(sigma)).reshape(shape)
    Bg, Bv = box_blur(g, r, dim), box_blur(v, r, dim)
    Bgf, Bvf = box_blur((g * f).float(), r, dim), box_blur((v * f).float(), r, dim)
    vd, gd = v.double(), g.double()
    D = vd * f * Bg - vd * Bgf + gd * f * Bv - gd * Bvf
    gs = ((D * f).sum() - (Bg.double() * vd).sum()) / float(sigma)
    return (Bg if need_x else None), gs.float()


# ---------------------------------------------------------------------------------------------
# box-window guided filter and its backward (crf/guided.py; include/phl.h, phl_guided.hip)
_nearest_maps = OrderedDict()


def _nearest_index_maps(H, W, s, device):
    """int32 device maps of F.interpolate(mode='nearest') between (H, W) and (H // s, W // s): (row_of_low [h], col_of_low
    [w], low_of_row [H], low_of_col [W]).  torch interpolates an arange itself, on the tensors' own device, so the kernel
    cannot disagree with torch's float rounding of floor(dst * in / out).  Cached per (H, W, s, device)."""
    key = (H, W, s, str(device))
    maps = _nearest_maps.get(key)
    if maps is None:
        def nearest(n_in, n_out):
            if n_in == n_out:
                return torch.arange(n_in, dtype=torch.int32, device=device)
            src = torch.arange(n_in, dtype=torch.float32, device=device).reshape(1, 1, n_in, 1)
            return torch.nn.functional.interpolate(src, size=(n_out, 1), mode="nearest").reshape(n_out).to(torch.int32)

        h, w = H // s, W // s
        maps = (nearest(H, h), nearest(W, w), nearest(h, H), nearest(w, W))
        _nearest_maps[key] = maps
        while len(_nearest_maps) > 16:
            _nearest_maps.popitem(last=False)
    return maps


def guided_filter(y, x, r, eps, *, subsample=1, scale=1.0, subtract=None, out=None, full_cov=False):
    """The box-window guided filter of ``y`` [B, cy, H, W] by the guide ``x`` [B, cx, H, W] (phl_guided_filter; forward
    only): ``out = guided(y, x) * scale - subtract``.  ``r`` is the full-resolution radius; with ``subsample = s > 1`` the
    linear model is solved on nearest samples at (H // s, W // s) with radius r // s and upsampled by nearest
    (FastGuidedFilter).  ``eps``: a number or a tensor of cx values (softplus(omega) stays on the device).  fp32 CUDA
    tensors of any strides (copied contiguous); any radius (above phl_guided_filter_max_r at the solving resolution the
    kernels read the image from memory instead of LDS tiles); PhlError status 7 for more than 16 guide channels.
    ``full_cov``: the linear model over the whole covariance matrix of the guide channels, A = cov_yx (cov_xx + diag(eps))^-1
    (phl_guided_filter_full; PhlError status 7 for more than GUIDED_FULL_MAX_CX guide channels), instead of one model per
    channel."""
    return _guided_forward("guided_filter", "phl_guided_filter_full" if full_cov else "phl_guided_filter", y, x, r, eps, subsample,
                           scale, subtract, out)


def guided_filter_labels_per_chunk(B, cy, cx, h, w, *, full=False, need_y=False, need_x=False, need_eps=False, grad=None,
                                   full_cov=False):
    """Labels (of the B * cy planes of y) that one chunk of a guided_filter call holds at the solving resolution h x w,
    or, with any ``need_*`` flag or ``grad=True``, of the guided_filter_grad call that is asked for those gradients
    (``full``: subsample == 1; ``full_cov``: of the guided_filter_full_grad call -- the forward's chunks do not depend on
    the model).  A guided_filter_bilinear_grad call holds the labels of the guided_filter_grad call with ``full=False``,
    and a guided_filter_bilinear_full_grad call those of the guided_filter_full_grad call with ``full=False``: the same
    per-label planes.  Host arithmetic of the library (phl_guided_filter_labels_per_chunk,
    phl_guided_filter_full_grad_labels_per_chunk), no device needed."""
    needs = (1 if need_y else 0) | (2 if need_x else 0) | (4 if need_eps else 0)
    if grad is None:
        grad = needs != 0
    if full_cov and grad:
        return int(_call("phl_guided_filter_full_grad_labels_per_chunk", int(B), int(cy), int(cx), int(h), int(w), 1 if full else 0,
                         needs, value=True))
    return int(_call("phl_guided_filter_labels_per_chunk", int(B), int(cy), int(cx), int(h), int(w), 1 if full else 0,
                     needs if grad else -1, value=True))


def guided_filter_bilinear(y, x, r, eps, *, subsample, scale=1.0, subtract=None, out=None, full_cov=False):
    """FastGuidedFilter(mode='bilinear') (phl_guided_filter_bilinear; its backward: guided_filter_bilinear_grad, with ``full_cov``
    guided_filter_bilinear_full_grad):
    guided_filter with the linear model solved on ``F.interpolate(., size=(H // s, W // s), mode='bilinear')`` of y and x, radius r // s, and its window means
    interpolated back to (H, W) the same way, ``out = (sum_c U(mean_A_c) x_c + U(mean_b)) * scale - subtract``.  The taps
    are computed on the device (no index maps).  Tensor rules of guided_filter; ``subsample`` >= 2 (at 1 both
    interpolations are the identity: guided_filter).  ``full_cov``: the model over the whole covariance matrix, up to
    GUIDED_FULL_MAX_CX guide channels (PhlError status 7 above, as above 16 channels without it)."""
    if int(subsample) < 2:
        raise ValueError(f"guided_filter_bilinear: needs subsample >= 2, got {subsample}")
    return _guided_forward("guided_filter_bilinear", "phl_guided_filter_bilinear", y, x, r, eps, subsample, scale, subtract, out,
                           maps=False, flags=GUIDED_BILINEAR_FULL_COV if full_cov else 0)


def guided_filter_bilinear_labels_per_chunk(B, cy, cx, h, w):
    """Labels per chunk of a guided_filter_bilinear call at the solving resolution h x w
    (phl_guided_filter_bilinear_labels_per_chunk: host arithmetic of the library, no device needed)."""
    return int(_call("phl_guided_filter_bilinear_labels_per_chunk", int(B), int(cy), int(cx), int(h), int(w), value=True))


def _guided_forward(name, entry, y, x, r, eps, subsample, scale, subtract, out, maps=True, flags=None):
    """guided_filter (either model) and (no ``maps``, a ``flags`` word at the end) guided_filter_bilinear: one argument
    list, three entry points."""
    _, e, dims, maps = _guided_launch_args(name, y, x, subtract, "subtract", r, eps, subsample, maps=maps)
    out = _out_or_empty(name, out, y.shape, y.device, "y's shape and device")
    if dims is None:
        return out
    yc, xc = y.contiguous(), x.contiguous()
    sub = None if subtract is None else (yc if subtract is y else subtract.contiguous())
    _launch(y.device, entry, _ptr(yc), _ptr(xc), _ptr(sub), _ptr(out), *dims, *(() if maps is None else (_ptr(m) for m in maps)),
            _ptr(e), C.c_float(float(scale)), *(() if flags is None else (flags,)))
    return out


def _guided_launch_args(name, y, x, third, third_name, r, eps, subsample, launch=True, maps=True):
    """What guided_filter, guided_filter_bilinear and guided_filter_grad (``name``) share: the checks of y, x and ``third``
    (subtract or g: y's shape, may be None), of subsample and r; then (cx, eps as the kernels read it, the launch's (B, cy,
    cx, H, W, h, w, r // s), its four index maps -- None without ``maps``).  The last two are None when y has no elements or
    the caller launches nothing."""
    _fp32_cuda(name, y, x, *(() if third is None else (third,)))
    if y.dim() != 4 or x.dim() != 4 or y.shape[0] != x.shape[0] or y.shape[2:] != x.shape[2:] or x.device != y.device:
        raise ValueError(f"{name}: y [B, cy, H, W] and x [B, cx, H, W] on one device, got {tuple(y.shape)} and {tuple(x.shape)}")
    if third is not None and (third.shape != y.shape or third.device != y.device):
        raise ValueError(f"{name}: {third_name} must have y's shape and device")
    s, r = int(subsample), int(r)
    if s < 1 or r < 0:
        raise ValueError(f"{name}: needs subsample >= 1 and r >= 0, got {subsample} and {r}")
    B, cy, H, W = (int(v) for v in y.shape)
    cx = int(x.shape[1])
    e = _guided_eps(eps, cx, y.device, name)
    if y.numel() == 0 or not launch:
        return cx, e, None, None
    if H // s == 0 or W // s == 0:
        raise ValueError(f"{name}: a {H} x {W} image has no pixels at subsample {s}")
    return cx, e, (B, cy, cx, H, W, H // s, W // s, r // s), _nearest_index_maps(H, W, s, y.device) if maps else None


def _guided_eps(eps, cx, device, name):
    """eps of the guided filter as the kernels read it: [cx] fp32 on the device, detached."""
    if not torch.is_tensor(eps):
        return torch.full((cx,), float(eps), dtype=torch.float32, device=device)
    e = eps.detach().to(device=device, dtype=torch.float32).reshape(-1)
    if e.numel() == 1 and cx != 1:
        e = e.expand(cx)
    if e.numel() != cx:
        raise ValueError(f"{name}: eps has {e.numel()} values for {cx} guide channels")
    return e.contiguous()


def guided_filter_grad(y, x, g, r, eps, *, subsample=1, scale=1.0, subtract_is_y=False, need_y=True, need_x=False, need_eps=False):
    """Backward of ``guided_filter(y, x, r, eps, subsample=, scale=, subtract=y if subtract_is_y else None)`` for the upstream
    gradient ``g`` [B, cy, H, W] (phl_guided_filter_grad): ``(grad_y, grad_x, grad_eps)``, None for those not asked for;
    grad_eps has cx values.  Nothing of the forward is needed: the kernels recompute it from y, x and eps.  The same tensor
    rules as guided_filter (fp32 CUDA, any strides, any radius; PhlError status 7 for more than 16 guide channels); the
    same bits on every run."""
    return _guided_grad("guided_filter_grad", "phl_guided_filter_grad", y, x, g, r, eps, subsample, scale, subtract_is_y, need_y, need_x,
                        need_eps)


def guided_filter_full_grad(y, x, g, r, eps, *, subsample=1, scale=1.0, subtract_is_y=False, need_y=True, need_x=False,
                            need_eps=False):
    """Backward of ``guided_filter(..., full_cov=True)`` (phl_guided_filter_full_grad): arguments, return value and rules
    of guided_filter_grad; PhlError status 7 for more than GUIDED_FULL_MAX_CX guide channels."""
    return _guided_grad("guided_filter_full_grad", "phl_guided_filter_full_grad", y, x, g, r, eps, subsample, scale, subtract_is_y,
                        need_y, need_x, need_eps)


def guided_filter_bilinear_grad(y, x, g, r, eps, *, subsample, scale=1.0, subtract_is_y=False, need_y=True, need_x=False,
                                need_eps=False):
    """Backward of ``guided_filter_bilinear(y, x, r, eps, subsample=, scale=, subtract=y if subtract_is_y else None)``
    (phl_guided_filter_bilinear_grad; the diagonal model): arguments, return value and rules of guided_filter_grad, with
    ``subsample`` >= 2 as the forward (then 2 (H // s) <= H, which the kernels need).  The labels per chunk are
    ``guided_filter_labels_per_chunk(B, cy, cx, h, w, need_y=, need_x=, need_eps=)``."""
    if int(subsample) < 2:
        raise ValueError(f"guided_filter_bilinear_grad: needs subsample >= 2, got {subsample}")
    return _guided_grad("guided_filter_bilinear_grad", "phl_guided_filter_bilinear_grad", y, x, g, r, eps, subsample, scale,
                        subtract_is_y, need_y, need_x, need_eps, maps=False, flags=0)


def guided_filter_bilinear_full_grad(y, x, g, r, eps, *, subsample, scale=1.0, subtract_is_y=False, need_y=True, need_x=False,
                                     need_eps=False):
    """Backward of ``guided_filter_bilinear(..., full_cov=True)`` (phl_guided_filter_bilinear_full_grad): arguments, return
    value and rules of guided_filter_bilinear_grad; PhlError status 7 for more than GUIDED_FULL_MAX_CX guide channels.  The
    labels per chunk are ``guided_filter_labels_per_chunk(B, cy, cx, h, w, full_cov=True, need_y=, need_x=, need_eps=)``."""
    if int(subsample) < 2:
        raise ValueError(f"guided_filter_bilinear_full_grad: needs subsample >= 2, got {subsample}")
    return _guided_grad("guided_filter_bilinear_full_grad", "phl_guided_filter_bilinear_full_grad", y, x, g, r, eps, subsample, scale,
                        subtract_is_y, need_y, need_x, need_eps, maps=False)


def _guided_grad(name, entry, y, x, g, r, eps, subsample, scale, subtract_is_y, need_y, need_x, need_eps, maps=True, flags=None):
    """guided_filter_grad, guided_filter_full_grad and (no ``maps``) guided_filter_bilinear_grad (a ``flags`` word at the
    end) and guided_filter_bilinear_full_grad: one argument list, four entry points."""
    cx, e, dims, maps = _guided_launch_args(name, y, x, g, "g", r, eps, subsample, need_y or need_x or need_eps, maps)
    new = torch.zeros if y.numel() == 0 else torch.empty
    gy = new(y.shape, dtype=torch.float32, device=y.device) if need_y else None
    gx = new(x.shape, dtype=torch.float32, device=y.device) if need_x else None
    ge = new((cx,), dtype=torch.float32, device=y.device) if need_eps else None
    if dims is None:
        return gy, gx, ge
    yc, xc, gc = y.contiguous(), x.contiguous(), g.contiguous()         # (named: a copy must outlive the launch)
    _launch(y.device, entry, _ptr(yc), _ptr(xc), _ptr(gc), _ptr(gy), _ptr(gx), _ptr(ge), *dims,
            *(() if maps is None else (_ptr(m) for m in maps)), _ptr(e), C.c_float(float(scale)), 1 if subtract_is_y else 0,
            *(() if flags is None else (flags,)))
    return gy, gx, ge


def _guided_fn_forward(forward, ctx, y, x, eps, r, subsample, scale, subtract_is_y, **model):
    """forward of the four Functions below: only y, x and eps are saved."""
    ctx.save_for_backward(y, x, eps)
    ctx.args = (int(r), int(subsample), float(scale), bool(subtract_is_y))
    return forward(y, x, r, eps, subsample=subsample, scale=scale, subtract=y if subtract_is_y else None, **model)


def _guided_fn_backward(grad, ctx, g):
    """... and their backward: one call of ``grad`` computes the gradients that are asked for; that of eps has eps's shape."""
    y, x, eps = ctx.saved_tensors
    r, s, scale, sub = ctx.args
    need = ctx.needs_input_grad
    gy, gx, ge = grad(y, x, g, r, eps, subsample=s, scale=scale, subtract_is_y=sub, need_y=need[0], need_x=need[1], need_eps=need[2])
    if ge is not None:
        ge = (ge.sum() if eps.numel() == 1 and ge.numel() != 1 else ge).reshape(eps.shape).to(eps.dtype)
    return gy, gx, ge, None, None, None, None


class GuidedFilterFn(torch.autograd.Function):
    """``guided_filter(y, x, r, eps) * scale - (y if subtract_is_y else 0)`` with its backward on the library's kernels
    (guided_filter_grad): only y, x and eps are saved, one backward call computes the gradients that are asked for.
    ``eps`` is a tensor of cx values (or one); its gradient has its shape.  No double backward."""

    @staticmethod
    def forward(ctx, *args):
        return _guided_fn_forward(guided_filter, ctx, *args)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _guided_fn_backward(guided_filter_grad, ctx, g)


class GuidedFilterFullFn(torch.autograd.Function):
    """GuidedFilterFn for the full-covariance model: ``guided_filter(y, x, r, eps, full_cov=True) * scale - (y if
    subtract_is_y else 0)`` with its backward on guided_filter_full_grad."""

    @staticmethod
    def forward(ctx, *args):
        return _guided_fn_forward(guided_filter, ctx, *args, full_cov=True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _guided_fn_backward(guided_filter_full_grad, ctx, g)


class GuidedFilterBilinearFn(torch.autograd.Function):
    """GuidedFilterFn for mode='bilinear': ``guided_filter_bilinear(y, x, r, eps, subsample=) * scale - (y if
    subtract_is_y else 0)`` with its backward on guided_filter_bilinear_grad."""

    @staticmethod
    def forward(ctx, *args):
        return _guided_fn_forward(guided_filter_bilinear, ctx, *args)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _guided_fn_backward(guided_filter_bilinear_grad, ctx, g)


class GuidedFilterBilinearFullFn(torch.autograd.Function):
    """GuidedFilterBilinearFn for the full-covariance model: ``guided_filter_bilinear(y, x, r, eps, subsample=,
    full_cov=True) * scale - (y if subtract_is_y else 0)`` with its backward on guided_filter_bilinear_full_grad."""

    @staticmethod
    def forward(ctx, *args):
        return _guided_fn_forward(guided_filter_bilinear, ctx, *args, full_cov=True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _guided_fn_backward(guided_filter_bilinear_full_grad, ctx, g)


def stream_copy(dst, src):
    """float4 streaming copy (HBM ceiling probe for bench.py)."""
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
    _launch(src.device, "phl_stream_copy", _ptr(src), _ptr(dst), src.numel())
    return dst


def copy2d(dst, src):
    """dst[...] = src[...] for 2-D fp32 device tensors of equal shape and ANY strides, through the library's LDS-tiled
    transpose (phl_copy2d): the NCHW <-> pixel-major hops of the batched API."""
    assert dst.shape == src.shape and dst.dim() == 2 and dst.is_cuda and src.device == dst.device
    assert dst.dtype == torch.float32 and src.dtype == torch.float32
    _launch(dst.device, "phl_copy2d", _ptr(src), src.stride(0), src.stride(1), _ptr(dst), dst.stride(0), dst.stride(1),
            int(dst.shape[0]), int(dst.shape[1]))
    return dst


def expected_value(Q, labels):
    """Q @ labels (expected disparity per pixel) for CUDA fp32 Q [n, L], labels [L]."""
    if not _rowmajor(Q) or labels.dtype != torch.float32 or labels.numel() != Q.shape[1]:
        raise TypeError("expected_value: expects fp32 CUDA Q [n, L] and labels [L]")
    labels = labels.to(Q.device).contiguous()
    out = torch.empty((Q.shape[0],), dtype=torch.float32, device=Q.device)
    _launch(Q.device, "phl_expected_value", _ptr(Q), Q.stride(0), _ptr(labels), _ptr(out), Q.shape[0], Q.shape[1])
    return out


# ---------------------------------------------------------------------------------------------
# invisible lattice cache for the reference's stateless call shape
_CACHE_SIZE = int(os.environ.get("PHL_LATTICE_CACHE", "4"))
_cache = OrderedDict()
_cache_lock = threading.Lock()


# The drop-in boundary -- ``filter(src, ref)`` and everything of ``crf.*`` that reaches it through ``lattice_for`` --
# builds its lattices with the REFERENCE'S table behaviour (Lattice(reference_table=True): its duplicate vertices
# above M = 16383 included), so that what replaces ``lattice.filter`` returns what ``lattice.filter`` returned at
# any size.  PHL_REFERENCE_TABLE=0 selects the defect-free table instead (one vertex per key; a few ms less per build).
_REFERENCE_TABLE = os.environ.get("PHL_REFERENCE_TABLE", "1") not in ("", "0")


def _cache_key(ref, device=None):
    # device=None means what Lattice() resolves it to (ref's own GPU, or the current one for a CPU tensor): the same
    # lattice must be found whether a caller names that device or not (forward with device=dev, backward without)
    device = torch.device(_default_device(ref) if device is None else device)
    idx = device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else None)
    return (ref.device.type, ref.device.index, ref.data_ptr(), tuple(ref.shape), tuple(ref.stride()), ref._version,
            (device.type, idx))


def lattice_for(ref, device=None):
    """Cached Lattice for ``ref`` (built on ``device``; default: ref's own device, or the current one for a CPU
    tensor).  The entry keeps ``ref`` alive, so its storage address cannot be recycled while cached; an in-place
    update bumps ``ref._version`` and misses."""
    _require_gpu()
    if _CACHE_SIZE <= 0:
        return Lattice(ref, device=device, reference_table=_REFERENCE_TABLE)
    key = _cache_key(ref, device)
    with _cache_lock:
        hit = _cache.get(key)
        if hit is not None:
            _cache.move_to_end(key)
            return hit[0]
    lat = Lattice(ref, device=device, reference_table=_REFERENCE_TABLE)
    with _cache_lock:
        _cache[key] = (lat, ref)
        while len(_cache) > max(_CACHE_SIZE, _cache_floor[0]):
            _cache.popitem(last=False)
    return lat


_cache_floor = [0]      # batched_filter keeps one lattice per batch item alive across mean-field iterations


def clear_cache():
    with _cache_lock:
        _cache.clear()


def batch_devices(t=None):
    """Devices a batch of independent volumes is spread over (first row: "one image per GPU, no
    RCCL; host-side scatter of inputs / gather of outputs only").  CPU inputs -- the reference's calling
    convention, whose batch mode runs one worker process per image (crf/gaussian_matrix.py:370-377) -- go to all
    visible GPUs; tensors that already live on a GPU stay there (moving an [n, L] volume over xGMI costs more
    than filtering it) unless PHL_BATCH_DEVICES says otherwise ("all" or a comma list of indices)."""
    _require_gpu()
    env = os.environ.get("PHL_BATCH_DEVICES", "")
    ndev = torch.cuda.device_count()
    if env == "all":
        return [torch.device("cuda", i) for i in range(ndev)]
    if env:
        return [torch.device("cuda", int(i)) for i in env.split(",")]
    if t is not None and t.is_cuda:
        return [t.device]
    return [torch.device("cuda", i) for i in range(ndev)]


_batch_streams = {}


def _deal(bs, devices, inputs, outputs, item):
    """Deal the items 0 .. bs-1 of a batch over ``devices``, item i on devices[i % len(devices)], every device on its own
    side stream: the side stream waits for the current stream of every device that holds one of ``inputs`` (they may
    still be in flight on the caller's stream), ``item(i, device)`` runs under the device and stream guards, and at the
    end the current stream of every device that holds one of ``outputs`` waits for the side streams; CPU outputs are
    complete on return."""
    sources = list(dict.fromkeys(t.device for t in inputs if t.is_cuda))
    homes = list(dict.fromkeys(t.device for t in outputs if t.is_cuda))
    used = []
    for i in range(bs):
        dev = devices[i % len(devices)]
        st = _batch_streams.get(dev)
        if st is None:
            st = _batch_streams[dev] = torch.cuda.Stream(device=dev)
        for d in sources:
            st.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.device(dev), torch.cuda.stream(st):
            item(i, dev)
        used.append(st)
    for st in used:
        for d in homes:
            torch.cuda.current_stream(d).wait_stream(st)
        if any(not t.is_cuda for t in outputs):
            st.synchronize()


def batched_filter(srcs, refs, devices=None, subtract_input=False):
    """Independent lattice per batch item: srcs [bs, n, vd], refs [bs, n, d] (any strides) -> [bs, n, vd] on
    srcs' device.  Item i runs on devices[i % len(devices)], each device on its own side stream, so that with
    several GPUs the items (and, for CPU inputs, their PCIe copies) proceed in parallel; no collective."""
    bs = srcs.shape[0]
    assert refs.shape[0] == bs and srcs.shape[1] == refs.shape[1], "Incompatible shapes {}, and {}".format(tuple(srcs.shape), tuple(refs.shape))
    devices = [torch.device(d) for d in (devices or batch_devices(srcs))]
    _cache_floor[0] = max(_cache_floor[0], min(bs, 64))
    out = torch.empty((bs,) + tuple(srcs.shape[1:]), dtype=torch.float32, device=srcs.device)

    def item(i, dev):
        lat = lattice_for(refs[i].detach(), device=dev)
        s = srcs[i].detach()
        res = lat.filter(s.to(dev, non_blocking=True) if s.device != dev else s, subtract_input=subtract_input)
        out[i].copy_(res, non_blocking=True)

    _deal(bs, devices, (srcs, refs), (out,), item)
    return out


def batched_filter_grad(srcs, refs, g, need_src=True, devices=None):
    """Per-item Lattice.filter_grad for a batch (the body of BatchedLatticeFilter.backward, crf/gaussian_matrix.py:402-421):
    srcs, g [bs, n, L], refs [bs, n, d] (any strides) -> (grad_srcs [bs, n, L] or None, grad_refs [bs, n, d]) on the
    inputs' devices.  Items are dealt over the same devices and side streams as batched_filter, so every item meets the
    lattice its forward pass cached.  d <= FILTER_GRAD_MAX_D = 16, in feature groups above d = 7 (Lattice.filter_grad).
    Raises PhlError(status 7) if the fused kernels do not take the shape."""
    bs = srcs.shape[0]
    devices = [torch.device(d) for d in (devices or batch_devices(srcs))]
    grad_refs = torch.empty(tuple(refs.shape), dtype=torch.float32, device=refs.device)
    grad_srcs = torch.empty(tuple(srcs.shape), dtype=torch.float32, device=srcs.device) if need_src else None

    def item(i, dev):
        r = refs[i].detach()
        lat = lattice_for(r, device=dev)
        gs, gr = lat.filter_grad(srcs[i].detach().to(dev, non_blocking=True), g[i].detach().to(dev, non_blocking=True),
                                 r.to(dev, non_blocking=True), need_src=need_src)
        grad_refs[i].copy_(gr, non_blocking=True)
        if need_src:
            grad_srcs[i].copy_(gs, non_blocking=True)

    _deal(bs, devices, (srcs, refs, g), (grad_refs, grad_srcs) if need_src else (grad_refs,), item)
    return grad_srcs, grad_refs


def filter(src, ref):
    """Drop-in for the reference's ``lattice.filter(src, ref)``: src [n, vd], ref [n, d], fp32.

    Argument order is the reference's (src first, ref second; lattice.cpp:6)."""
    if src.shape[0] != ref.shape[0]:
        raise AssertionError("Incompatible shapes {}, and {}".format(tuple(src.shape), tuple(ref.shape)))
    return lattice_for(ref.detach()).filter(src)
