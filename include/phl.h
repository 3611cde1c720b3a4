/*
 * phl.h -- C ABI of the MI355X-native permutohedral-lattice filter ("phl").
 *
 * This is the drop-in boundary for the dense-CRF mean-field message-passing step of
 * mfinzi/depth-estimation.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repo).  Plain pointers and sizes only: no torch types.
 *
 * Reference boundary being replaced
 *   python : latticefilter = lattice.filter            crf/gaussian_matrix.py:15-16
 *   C++    : at::Tensor filter(at::Tensor src, at::Tensor ref)
 *                                                      crf/lattice/lite/lattice.cpp:6-15
 *   engine : PermutohedralLattice::filter / splat / blur / slice
 *                                                      crf/lattice/lite/permutohedral.h:199-548
 *
 * Design difference (MI355X-first): the reference rebuilds the lattice inside every filter()
 * call although `ref` never changes during mean-field inference.  Here the
 * lattice is an object: build once per `ref` (phl_build), filter many value sets
 * (phl_filter).  phl_filter_once() keeps the reference's one-shot call shape.
 *
 * All pointers named *_dev are DEVICE pointers to fp32 (the reference is fp32 only,
 * permutohedral.h:16-19).  Strides are in ELEMENTS, so permuted NCHW views
 * (gaussian_matrix.py:348-349) are accepted without a host copy.  All work is enqueued on
 * the caller's HIP stream (NULL = default stream); functions that return host data
 * synchronise that stream.  Functions return PHL_OK or an error code and never abort;
 * phl_last_error() gives the message for the calling thread.
 */
#ifndef PHL_H
#define PHL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHL_VERSION 100 /* major*10000 + minor*100 + patch */

typedef struct phl_lattice phl_lattice; /* opaque, owns device memory */
typedef void *phl_stream;               /* hipStream_t */

enum phl_status {
    PHL_OK = 0,
    PHL_ERR_INVALID = 1,     /* bad argument (NULL, negative size, d out of range, ...) */
    PHL_ERR_SHAPE = 2,       /* rows of src and ref differ: reference asserts
                                "Incompatible shapes {}, and {}" (gaussian_matrix.py:429-430,
                                permutohedral.h:204) */
    PHL_ERR_HIP = 3,         /* a HIP runtime call failed (message has hipGetErrorString) */
    PHL_ERR_NO_DEVICE = 4,   /* no gfx950 device: the product path has NO CPU fallback */
    PHL_ERR_KEY_RANGE = 5,   /* a lattice coordinate left int16: the reference stores keys as
                                `short` (permutohedral.h:39,398) and silently wraps */
    PHL_ERR_TOO_LARGE = 6,   /* n*(d+1) does not fit int32 indexing */
    PHL_ERR_UNSUPPORTED = 7
};

enum phl_filter_flags {
    PHL_FILTER_DEFAULT = 0,
    /* out = filter(src) - src : LatticeGaussian.forward, gaussian_matrix.py:302-303, and
       BatchedAdjacency.forward :352, fused into the slice epilogue */
    PHL_FILTER_SUBTRACT_INPUT = 1,
    /* Reference-exact arithmetic: splat sums every vertex in ascending pixel order (gather
       kernel) and slice divides every term by (1 + 2^-d) (permutohedral.h:455, :480), so the
       result is BIT-IDENTICAL to the reference's CPU path.  The default instead uses the
       LDS-staged chunk splat (per-chunk partial sums) and one final multiply by 1/(1+2^-d):
       same algorithm, fp32 rounding differences of ~1e-7 relative, ~1.3x faster. */
    PHL_FILTER_EXACT = 4,
    /* do not use the LDS-staged chunk kernels at all (plain gather splat and slice) */
    PHL_FILTER_NO_TILES = 8,
    /* phl_filter_once only (it builds its own lattice): the defect-free table, one vertex per key, instead of the
       reference's table behaviour (PHL_BUILD_REFERENCE_TABLE), which is what the one-shot call -- the drop-in for
       lattice.filter(src, ref) -- builds by default */
    PHL_FILTER_CLEAN_TABLE = 16
};

enum phl_build_flags {
    PHL_BUILD_DEFAULT = 0,
    /* Reproduce the observable behaviour of the reference's hash table across its doublings
     * (permutohedral.h:59-62, :101-103: lookup() hashes with the capacity it had BEFORE lookupOffset() grows
     * the table, so the one key in flight at each doubling -- first at M = 16383 -- is probed from a stale
     * slot and usually gets a SECOND vertex; blur then sees only one of the two).  Default: every key has one
     * vertex (the algorithm without that defect; identical to the reference below M = 16383 and on all but
     * 0.3-4 % of rows above).  With this flag vertex numbering, duplicate vertices and their visibility are
     * exactly the reference's and PHL_FILTER_EXACT is bit-identical to the reference's CPU path at any size.
     * Costs one host replay of the table per build (csrc/phl_reftable.hip). */
    PHL_BUILD_REFERENCE_TABLE = 1
};

/* Limits. */
#define PHL_MAX_D 16 /* feature dimensions supported by the device build */

int phl_version(void);
const char *phl_last_error(void);
const char *phl_status_string(int status);
/* Number of visible HIP devices (0 if none); never initialises a device context. */
int phl_device_count(void);

/* ---- lattice construction ---------------------------------------------------------------
 * Replaces PermutohedralLattice(d, vd, n) + the geometry half of splat() for all n pixels
 * (permutohedral.h:328-372, :376-447, :458-460) + the neighbour lookups of blur() (:504-522).
 * ref_dev: [n][d] fp32 with element strides (row_stride, col_stride).
 * Vertices are numbered in first-touch order of the (pixel, remainder) sequence -- the same
 * numbering the reference's insertion-ordered hash table produces (permutohedral.h:70-77). */
int phl_build(phl_lattice **out, const float *ref_dev, int64_t n, int d, int64_t ref_row_stride,
              int64_t ref_col_stride, int device, phl_stream stream);
/* phl_build with phl_build_flags. */
int phl_build_ex(phl_lattice **out, const float *ref_dev, int64_t n, int d, int64_t ref_row_stride,
                 int64_t ref_col_stride, int device, phl_stream stream, unsigned build_flags);
/* Frees device memory (hipFree): like any free it must not run while a stream capture is in
 * progress on the device (the Python binding parks handles that die during a capture). */
int phl_destroy(phl_lattice *lat);

int64_t phl_num_pixels(const phl_lattice *lat);
int64_t phl_num_vertices(const phl_lattice *lat); /* == hashTable.size() after splat */
int phl_num_dims(const phl_lattice *lat);
int phl_device(const phl_lattice *lat);
/* Device bytes held by the lattice (tables + value workspace). */
int64_t phl_device_bytes(const phl_lattice *lat);

/* phl_build keeps one grow-only device scratch block for its temporaries (so that building a
 * lattice per video frame performs no hipMalloc for work arrays; PHL_SCRATCH_MAX_MB caps it,
 * 0 disables).  phl_trim_scratch() gives the block back. */
int phl_trim_scratch(void);

/* ---- row-band multi-GPU support -------------------------------------------------------------
 * Append vertices that exist in a NEIGHBOURING row band of the same image ("ghost" vertices:
 * no local pixel splats into them) so that blur() sees the same neighbourhood it would see in
 * the whole-image lattice.  keys_host: [count][d] int16, distinct.  vid_host[i] receives the
 * local vertex id of key i (an existing vertex when this band already has it, else a new id
 * >= phl_num_local_vertices()).  No reference counterpart: the reference is single-process. */
int phl_add_vertices(phl_lattice *lat, const int16_t *keys_host, int64_t count, int32_t *vid_host,
                     phl_stream stream);   /* vid_host: ROW of each key in the [M][vd] vertex buffers */
int64_t phl_num_local_vertices(const phl_lattice *lat); /* vertices created by this lattice's own pixels */
/* A band's lattice CUT OUT OF the whole image's lattice `whole` (built with PHL_BUILD_REFERENCE_TABLE, so that the band
 * inherits the reference's vertices -- the duplicates its hash table creates at its doublings, permutohedral.h:59-62,101-103,
 * and which of them every lookup resolved to -- instead of re-deriving a defect-free lattice from its own pixels).
 * Pixels [p0, p1) of `whole` become pixels 0 .. p1-p0-1; sel_host lists the n_sel vertices of `whole` to keep (first-touch
 * ids, distinct): the first n_own must cover every vertex those pixels touch, the rest are ghosts (vertices of the
 * neighbouring bands within blur's reach), kept in the caller's order behind the own vertices.  The new lattice's
 * first-touch numbering is the position in sel_host.  ref_dev: the band's own features [p1-p0][d] (chunk grid).
 * phl_vertices_of_pixels: mask_host[v] = 1 iff a pixel of [p0, p1) touches first-touch vertex v (else 0), [phl_num_vertices].
 * No reference counterpart (the reference is single-process). */
int phl_vertices_of_pixels(phl_lattice *lat, int64_t p0, int64_t p1, unsigned char *mask_host, phl_stream stream);
int phl_sub_lattice(phl_lattice **out, phl_lattice *whole, int64_t p0, int64_t p1, const int32_t *sel_host, int64_t n_sel,
                    int64_t n_own, const float *ref_dev, int64_t ref_row_stride, int64_t ref_col_stride, phl_stream stream);

/* Pre-size everything phl_filter(vd) needs (the [M][vd] ping-pong buffers, the partial-row buffer
 * of the chunk splat or the contribution lists of the gather splat) so that the NEXT call, on any stream,
 * allocates nothing and never synchronises: required before hipGraph capture.
 *
 * Threading: a lattice is re-entrant.  Its tables are read-only after the build; the buffers a filter call
 * writes live in workspaces handed out per call (reused in stream order, a second one is allocated when two
 * streams are in flight at once), so any number of host threads / streams may call phl_filter, phl_splat,
 * phl_blur, phl_slice on one handle concurrently.  phl_add_vertices and phl_destroy are not concurrent with
 * anything. */
int phl_reserve(phl_lattice *lat, int vd);
/* phl_reserve with options: PHL_RESERVE_STRIDED_IO also sizes the staging copies that channel-major (NCHW) views -- and
 * pixel-major rows whose stride or base address is off the 16-byte grid, from 128 channels on -- go through (channel
 * counts >= 128 that are not a multiple of 4 are always staged, at the width rounded up: sized without the flag),
 * PHL_RESERVE_EXACT prepares for PHL_FILTER_EXACT calls (builds the pixel-sorted lists). */
enum phl_reserve_flags { PHL_RESERVE_STRIDED_IO = 1, PHL_RESERVE_EXACT = 2 };
int phl_reserve_ex(phl_lattice *lat, int vd, unsigned reserve_flags);

/* ---- the hot path -----------------------------------------------------------------------
 * out = slice(blur(splat(src)))  == lattice.filter(src, ref) of the reference
 * (lattice.cpp:6-10 -> permutohedral.h:236-238, :260, :264-276).
 * src_dev/out_dev: [n][vd] fp32, element strides; out may not alias src. */
int phl_filter(phl_lattice *lat, const float *src_dev, int vd, int64_t src_row_stride,
               int64_t src_col_stride, float *out_dev, int64_t out_row_stride,
               int64_t out_col_stride, unsigned flags, phl_stream stream);

/* One-shot call with the reference's argument order (src first, ref second):
 * builds, filters, destroys -- what lattice.filter(src, ref) does on every call.  The lattice is built with
 * PHL_BUILD_REFERENCE_TABLE (results are the reference's at any size) unless flags has PHL_FILTER_CLEAN_TABLE. */
int phl_filter_once(const float *src_dev, int vd, int64_t src_row_stride, int64_t src_col_stride,
                    const float *ref_dev, int d, int64_t ref_row_stride, int64_t ref_col_stride,
                    int64_t n, float *out_dev, int64_t out_row_stride, int64_t out_col_stride,
                    unsigned flags, int device, phl_stream stream);

/* Backward of one filter call w.r.t. the FEATURES (and the source), replacing the body of
 * LatticeFilter.backward, crf/gaussian_matrix.py:435-468: for out = filter(src, ref) and an incoming gradient g [n][L],
 *     grad_ref[i][k] = -2 sum_l ( src_il f_ik (Wg)_il - src_il (W(g f_k))_il + g_il f_ik (Ws)_il - g_il (W(s f_k))_il )
 * (:463; W = this lattice's splat-blur-slice, f = ref) and, if grad_src != NULL, grad_src = W g (:446 -- the
 * operator is symmetric).  The reference materialises the 2L(1+d)-channel operand [g, g(x)ref, src, src(x)ref],
 * filters it and contracts the 2L(1+d)-channel result; here the products are formed on the weights inside the
 * splat and the contraction inside the slice, so HBM sees src and g twice, the wide vertex buffer
 * [M][(1+d)L] (two passes) and [n][d] -- never a wide per-pixel tensor.  ref must be the array the lattice was
 * built from.  src, g, grad_src: pixel-major rows (unit channel stride), 16-byte aligned, L % 4 == 0;
 * d <= PHL_FILTER_GRAD_MAX_D = 16.  grad_ref: dense [n][d].  PHL_ERR_UNSUPPORTED for shapes outside that (callers then
 * filter the wide operand).
 * Feature groups: column k needs only block 0 (W x) and block 1+k (W(x f_k)) of the wide vertex rows, so the d features
 * are contracted in ceil(d / 7) groups of at most 7 columns, sized as evenly as possible (8 -> 4+4, 15 -> 5+5+5,
 * 16 -> 6+5+5); every group is a wide splat, blur and contracting slice of (columns + 1) L channels, and the workspace
 * is that of the widest group, not of d + 1 blocks.  d <= 7 is one group holding every feature.  The environment
 * variable PHL_GRAD_FEATURES_PER_GROUP (1..7, read on every call) caps the group size at any d. */
#define PHL_FILTER_GRAD_MAX_D 16
int phl_filter_grad(phl_lattice *lat, const float *src_dev, int64_t src_row_stride, const float *g_dev,
                    int64_t g_row_stride, int L, const float *ref_dev, int64_t ref_row_stride, int64_t ref_col_stride,
                    float *grad_ref_dev, float *grad_src_dev, int64_t grad_src_row_stride, phl_stream stream);

/* ---- stage-level entry points (profiling, roofline measurement, parity of intermediates) --
 * vert buffers are dense [M][vd] fp32 device arrays owned by the caller. */
/* value half of splat(): vert[v] = sum over (pixel,weight) of w*src[pixel]   (:454-455) */
int phl_splat(phl_lattice *lat, const float *src_dev, int vd, int64_t src_row_stride,
              float *vert_dev, unsigned flags, phl_stream stream);
/* one blur axis, Jacobi: dst[v] = 2*(1/4 src[n1] + 1/2 src[v] + 1/4 src[n2])   (:498-533) */
int phl_blur_axis(phl_lattice *lat, int axis, const float *vert_src_dev, float *vert_dst_dev, int vd,
                  phl_stream stream);
/* blur(): all d+1 axes in order 0..d (:486-548), ping-ponging between the caller's two [M][vd]
 * buffers (input in vert_a).  Consecutive axes are taken two per pass (same bits as two
 * phl_blur_axis calls, half the traffic over the vertex array).  *result_in_b = 1 if the result
 * ends up in vert_b, 0 if in vert_a. */
int phl_blur(phl_lattice *lat, float *vert_a_dev, float *vert_b_dev, int vd, int *result_in_b, phl_stream stream);
/* Row-band exchange helpers (no reference counterpart): out[r] = vert[idx[r]] and vert[idx[r]] += in[r]
 * for k rows of vd channels (vd % 4 == 0, 16-byte aligned); idx_dev: int64 on the device, DISTINCT
 * within one scatter call (no atomics: the sum order stays fixed).  Current device, given stream. */
int phl_gather_rows(const float *vert_dev, int vd, const int64_t *idx_dev, int64_t k, float *out_dev,
                    int64_t out_row_stride, phl_stream stream);
int phl_scatter_add_rows(float *vert_dev, int vd, const int64_t *idx_dev, int64_t k, const float *in_dev,
                         int64_t in_row_stride, phl_stream stream);
/* The chunk splat in two (or more) parts, for overlapping the row-band exchange with compute: run only the listed
 * pixel chunks, then complete exactly the listed vertex rows.  A rank first splats the chunks that touch its
 * boundary vertices (phl_chunks_touching) and completes those rows -- they can travel -- and then the interior
 * chunks and all other rows while the exchange is in flight.  partial_dev: caller-owned [phl_partial_rows()][vd]
 * scratch shared by the parts of one splat (rows shared between an early and a late chunk are summed by the late
 * part).  Every chunk must appear in exactly one part and every vertex row in exactly one part that runs after all
 * chunks touching it.  No reference counterpart. */
int64_t phl_num_chunks(const phl_lattice *lat);
int64_t phl_partial_rows(const phl_lattice *lat);
/* mask_host[c] = 1 iff pixel chunk c contributes to any of the k listed vertex rows (device int64 array) */
int phl_chunks_touching(phl_lattice *lat, const int64_t *rows_dev, int64_t k, int32_t *mask_host /* [phl_num_chunks] */,
                        phl_stream stream);
int phl_splat_part(phl_lattice *lat, const float *src_dev, int vd, int64_t src_row_stride, float *vert_dev,
                   float *partial_dev, const int32_t *chunks_dev, int64_t nchunks_sel, const int32_t *rows_dev,
                   int64_t nrows, phl_stream stream);
/* phl_splat_part that also fills the exchange's send buffer: listed row i is written to pack_dev[pack_pos_dev[i]]
 * (rows of pack_row_stride floats; pack_pos < 0: not packed) by the kernel that completes it, instead of a separate
 * gather afterwards.  src_dev may be NULL when no chunks are listed.  pack_pos_dev == NULL: plain phl_splat_part. */
int phl_splat_part_pack(phl_lattice *lat, const float *src_dev, int vd, int64_t src_row_stride, float *vert_dev,
                        float *partial_dev, const int32_t *chunks_dev, int64_t nchunks_sel, const int32_t *rows_dev,
                        int64_t nrows, const int32_t *pack_pos_dev, float *pack_dev, int64_t pack_row_stride,
                        phl_stream stream);
/* Row-band lattices: per blur axis a, the rows whose OUTPUT of axis a is read by anything later (the next axes' stencils,
 * finally slice) as three ascending, non-overlapping row ranges ranges[a][k] = {begin, end} (empty ranges allowed).  The
 * blur of phl_blur / phl_filter then computes only those rows (a pass over the axis pair (2p, 2p+1) computes the rows
 * named for axis 2p+1); the others keep stale values nobody reads.  A band carries ghost vertices 2-3 lattice steps deep
 * for the FIRST axes' stencils; later axes need fewer of them and slice none (phl/rowtile.py derives the sets from the
 * neighbour tables).  ranges == NULL: all rows again.  phl_add_vertices resets it.  Like phl_add_vertices it belongs to
 * the assembly of a band's lattice: not concurrent with filter calls on the handle.  No reference counterpart. */
int phl_set_blur_rows(phl_lattice *lat, const int64_t *ranges /* [d+1][3][2] */, int naxes);
/* slice(): out[p] = sum_i w_i * vert[v_i] / (1 + 2^-d)                        (:473-483) */
int phl_slice(phl_lattice *lat, const float *vert_dev, int vd, float *out_dev, int64_t out_row_stride,
              const float *sub_dev /* NULL or src to subtract */, int64_t sub_row_stride, unsigned flags,
              phl_stream stream);

/* ---- mean-field elementwise steps around the filter ----------------------
 * out[p,:] = softmax(-(E0[p,:] + G[p,:])) over the L labels of every pixel; G may be NULL.
 * Fuses `E = E_0 + (W@Q)@Mu; Q = softmax(-E, dim=1)` of mean_field_infer (crf/crf_module.py:49-52)
 * into one pass.  Rows are pixel-major with unit channel stride; row strides in elements. */
int phl_softmax_neg_add(const float *E0_dev, int64_t e0_row_stride, const float *G_dev, int64_t g_row_stride,
                        float *out_dev, int64_t out_row_stride, int64_t n, int L, phl_stream stream);
/* out[p,:] = softmax(-(E0[p,:] + X[p,:] @ Mu)): the whole non-lattice half of a mean-field iteration
 * (`E = E_0 + (W@Q)@Mu; Q = softmax(-E)`, crf/crf_module.py:51-52, with X = W@Q) in ONE kernel -- the
 * compatibility product on the fp32-input matrix cores (exact f32, as the reference computes), +E0 and the row
 * softmax applied to the accumulators, so G and E never exist in memory.
 * mu_t_dev is Mu TRANSPOSED and zero-padded to the tile width Lp = 32*ceil(L/32): a dense [Lp][Lp] array with
 * mu_t[c*Lp + k] = Mu[k][c] for c, k < L and 0 elsewhere (Charbonnier / Potts compatibilities are symmetric: their
 * own transpose).  Needs L % 4 == 0, L <= 256, all three row strides % 4 == 0 and 16-byte aligned E0 / X / out /
 * mu_t (else PHL_ERR_UNSUPPORTED: the caller keeps its GEMM + phl_softmax_neg_add).  Rows have unit channel stride.
 * flags: PHL_COMPAT_LOGITS writes -(E0 + X @ Mu) instead of its softmax (CRFasRNN returns the logits of the last
 * iteration, crf_module.py:103). */
enum phl_compat_flags { PHL_COMPAT_SOFTMAX = 0, PHL_COMPAT_LOGITS = 1 };
int phl_compat_softmax(const float *E0_dev, int64_t e0_row_stride, const float *X_dev, int64_t x_row_stride,
                       const float *mu_t_dev, float *out_dev, int64_t out_row_stride, int64_t n, int L, unsigned flags,
                       phl_stream stream);
/* The same step for 128 < L <= 512 on the bf16 matrix cores (sixteen times the f32 rate; it pays from L ~ 176 on, below
 * that the f32 kernel is bound by its bytes as well).  128 < L <= 256 runs on one 256-label tile, padded above L;
 * 256 < L <= 512 on a kernel of its own whose row is L rounded up to 32 (344 labels compute as 352; it also computes
 * the two cross terms mL + lM, for energies of a few hundred).  Both operands are split
 * into three bf16 addends each -- x = h + m + l, eight significant bits apiece, exact -- and the six partial products
 * that matter (hH + hM + mH + hL + lH + mM; the dropped ones are below 2^-23 |x mu|).  Products of bf16 pairs are exact
 * in f32 and the matrix cores accumulate in f32: the result carries the rounding of an f32 dot product (measured next
 * to phl_compat_softmax against float64: tests/test_gpu_meanfield.py), at 3/8 of the matrix time, which makes the step
 * the streaming pass over E0, X and Q that its bytes say.  The compatibility matrix is PREPARED once per Mu:
 *   phl_compat_planes_bytes(L)   size of the prepared planes (384 KiB up to 256 labels, up to 1.5 MiB at 512), 0 if
 *                                the split kernels do not take this L
 *   phl_compat_prepare           mu_t_dev ([Lp][Lp], as for phl_compat_softmax) -> planes_dev (16-byte aligned)
 *   phl_compat_softmax_split     the step; same arguments and flags as phl_compat_softmax plus the planes (mu_t_dev
 *                                serves the last n % 128 rows -- n % 64 above 256 labels -- which run the f32 chain)
 * PHL_ERR_UNSUPPORTED for other L / alignments (the caller stays with phl_compat_softmax). */
size_t phl_compat_planes_bytes(int L);
int phl_compat_prepare(const float *mu_t_dev, int L, void *planes_dev, phl_stream stream);
int phl_compat_softmax_split(const float *E0_dev, int64_t e0_row_stride, const float *X_dev, int64_t x_row_stride,
                             const float *mu_t_dev, const void *planes_dev, float *out_dev, int64_t out_row_stride,
                             int64_t n, int L, unsigned flags, phl_stream stream);
/* The same step for compatibility matrices of the Potts family, Mu = alpha*J + beta*I (J all ones; the reference's
 * `potts` layer is alpha = 1, beta = -1, crf_module.py:55-64): X @ Mu = alpha*rowsum(X) + beta*X, so
 * out[p,:] = softmax(-(E0[p,:] + alpha*sum_c X[p,c] + beta*X[p,:])) is one streaming pass, no matrix product.
 * Needs L % 4 == 0, L <= 1024, row strides % 4 == 0 and 16-byte aligned E0 / X / out (else PHL_ERR_UNSUPPORTED).
 * flags: phl_compat_flags. */
int phl_uniform_compat_softmax(const float *E0_dev, int64_t e0_row_stride, const float *X_dev, int64_t x_row_stride,
                               float alpha, float beta, float *out_dev, int64_t out_row_stride, int64_t n, int L,
                               unsigned flags, phl_stream stream);
/* ---- the same half of the iteration for channel-major (NCHW) data: CRFasRNN with a W that is not the lattice ----
 * CRFasRNN evaluates W(Mu(Q)) on [B, L, H, W] tensors (crf/crf_module.py:66-79, 97-103), so what lies between two W
 * calls is the dual of phl_compat_softmax -- softmax first, then the product -- in one kernel:
 *   PHL_NCHW_PRODUCT   out[b,c,p] = sum_a mu[a*L + c] * softmax_a(-(E0[b,a,p] + G[b,a,p]))
 *                      mu is the dense [L][L] matrix itself (row stride L, NOT transposed; a scale such as charb's exp(s)
 *                      already inside).  1 <= L <= 256.  The softmax is max-subtracted (expf, one 1.0f / s per pixel) over
 *                      an LDS-staged [L][64 pixels] block; the product is an f32 fma chain in a order, on the f32-input
 *                      matrix cores above 32 labels and on the vector unit up to 32.
 *   PHL_NCHW_UNIFORM   mu = alpha*J + beta*I (the Potts family; `potts` is alpha = 1, beta = -1, crf_module.py:55-64):
 *                      out = alpha * colsum(Q) + beta * Q, the column sum computed; one streaming pass, no product.
 *                      L <= 1024.  mu is ignored.
 *   PHL_NCHW_SOFTMAX   out = Q: for a compatibility module that is not a matrix (the caller runs it on Q).  Any L >= 1.
 *   PHL_NCHW_LOGITS    out = -(E0 + G): what CRFasRNN returns after the last iteration (:103).  G is required.  Any L >= 1.
 * E0, G, out: contiguous fp32 [B][L][n] on the device, n = H*W; G may be NULL except for the logits (the first step of
 * the loop is Q = softmax(-E0)).  Any n: float4 accesses along the pixel axis when n % 4 == 0 and E0 / G / out are
 * 16-byte aligned, dwords otherwise.  alpha / beta are read in uniform mode only.  No atomics: the same bits on every
 * run.  Status, checked before any HIP call: PHL_ERR_INVALID for negative sizes, L < 1, an unknown mode or non-finite
 * alpha / beta in uniform mode; then zero elements (B == 0 or n == 0) are PHL_OK with nothing launched; then
 * PHL_ERR_INVALID for NULL E0 / out, NULL mu in product mode, NULL G in logits mode or out aliasing E0 or G;
 * PHL_ERR_TOO_LARGE when B*L*n*4 bytes leave int64 or the workgroups (64 pixels each; 256 above 256 labels) leave
 * 2^31 - 1; PHL_ERR_UNSUPPORTED for L outside the mode's range (the caller keeps its torch ops). */
enum phl_nchw_mode { PHL_NCHW_PRODUCT = 0, PHL_NCHW_UNIFORM = 1, PHL_NCHW_SOFTMAX = 2, PHL_NCHW_LOGITS = 3 };
int phl_nchw_softmax_compat(const float *E0_dev, const float *G_dev, const float *mu_dev, float alpha, float beta,
                            float *out_dev, int B, int L, int64_t n, int mode, phl_stream stream);
/* PHL_NCHW_PRODUCT for 1 <= L <= 512: what a general mu needs at the reference's label counts above 256 (max_disp =
 * w / 6: 341 at 2048 columns, 480 at 2880).  Up to 256 labels it runs the code of phl_nchw_softmax_compat(...,
 * PHL_NCHW_PRODUCT) and gives its bits; for 256 < L <= 512 the same scheme on an LDS-staged [L][32 pixels] block (64 KiB
 * at 512 labels, two workgroups per CU): the max-subtracted column softmax with eight partials per pixel combined in a
 * fixed order, then the product on the f32-input matrix cores, mu read from global memory / L2: an fma chain in a order
 * over each block of 32 labels, the blocks' sums added in an order that is a function of the workgroup's index alone (a
 * third of one long chain's rounding at 341 labels; equal columns at different pixels may differ in the last bits).
 * Operands, the float4 / dword rule and the order of the checks are phl_nchw_softmax_compat's: PHL_ERR_INVALID for
 * B < 0, n < 0 or L < 1; then B == 0 or n == 0 is PHL_OK with nothing launched; then PHL_ERR_INVALID for NULL E0 / out /
 * mu or out aliasing E0 or G; PHL_ERR_TOO_LARGE when B*L*n*4 bytes leave int64 or the workgroups (64 pixels each; 32
 * above 256 labels) leave 2^31 - 1; PHL_ERR_UNSUPPORTED for L > 512.  No atomics: the same bits on every run. */
int phl_nchw_softmax_compat_wide(const float *E0_dev, const float *G_dev, const float *mu_dev, float *out_dev, int B,
                                 int L, int64_t n, phl_stream stream);
/* The same step for TRAINING, 1 <= L <= PHL_NCHW_TRAIN_MAX_L = 64 labels (the reference trains at 18 and at w / 6 = 60),
 * with its backward; the arithmetic between the fp32 loads and the fp32 stores is float64, so every output is the
 * float64 result rounded once.  Per pixel column, with Q_a = softmax_a(-(E0_a + G_a)):
 *   phl_nchw_step_train        out[b,c,p] = sum_a mu[a*L + c] * Q_a
 *   phl_nchw_step_train_grad   for the upstream gradient gY of out:  t_a = sum_c mu[a*L + c] * gY_c,  s = sum_a Q_a t_a,
 *                              dE[b,a,p] = Q_a * (s - t_a)              -- the gradient of E0 and of G alike
 *                              gmu[a*L + c] = sum over b, p of Q_a[b,p] * gY_c[b,p]
 *                              Nothing but the forward's inputs and gY is read: Q is recomputed.
 * E0, G, gY, out, dE: contiguous fp32 [B][L][n] on the device, n = H*W; G may be NULL.  mu, gmu: dense fp32 [L][L], row
 * stride L, NOT transposed.  Either of dE / gmu may be NULL, and that part is then neither computed nor stored; both
 * NULL is PHL_ERR_INVALID.  A workgroup owns tiles of 64 consecutive pixels and all L labels of them in LDS (Q as
 * doubles, at most 52.25 KiB: two workgroups per CU): a max-subtracted softmax, then fma chains in label order on the
 * vector unit, the four partials of a pixel combined in a fixed order; mu is laid out once per call as doubles in a
 * stream-ordered scratch of at most 32 KiB and read through scalar loads.  float4 accesses along the pixel axis when
 * n % 4 == 0 and every volume pointer is 16-byte aligned, dwords otherwise.  gmu: R =
 * phl_nchw_step_train_partials(B, L, n) workgroups -- a function of its arguments alone, never of the device: the
 * number of 64-pixel tiles B * ceil(n / 64), at most 1024; 0 for B < 1, L < 1 or n < 1 -- walk the tiles w, w + R, ..
 * with their share of every gmu element in registers, write one [L][L] double partial each to a stream-ordered scratch
 * (at most 32 MiB), and a second kernel adds the R partials in index order and stores fp32.  No atomics: the same bits
 * on every call, and dE's bits do not depend on whether gmu is asked for (nor gmu's on dE).
 * Status, checked before any HIP call: PHL_ERR_INVALID for negative sizes or L < 1; then B == 0 or n == 0 is PHL_OK
 * with nothing launched; then PHL_ERR_INVALID for NULL E0 / mu / out (gY; both of dE and gmu) or an output that is one
 * of the inputs or the other output; PHL_ERR_TOO_LARGE when B*L*n*4 bytes leave int64 or the 64-pixel tiles leave
 * 2^31 - 1; PHL_ERR_UNSUPPORTED for L > PHL_NCHW_TRAIN_MAX_L (the caller keeps its torch ops). */
#define PHL_NCHW_TRAIN_MAX_L 64
int phl_nchw_step_train(const float *E0_dev, const float *G_dev, const float *mu_dev, float *out_dev, int B, int L,
                        int64_t n, phl_stream stream);
int phl_nchw_step_train_grad(const float *E0_dev, const float *G_dev, const float *mu_dev, const float *gY_dev,
                             float *dE_dev, float *gmu_dev, int B, int L, int64_t n, phl_stream stream);
int phl_nchw_step_train_partials(int B, int L, int64_t n);
/* ---- the expected label of a channel-major column: the end of the CRFasRNN heads (crf/mb_stereo_crf.py) -----------
 * Every head finishes with logits2average_depth(CRF(...)): a softmax over the label channels, a broadcast product with
 * the labels and a sum.  Here that is one kernel, and with negate != 0 it takes the loop's E0 and G as they are, so the
 * logits of the last iteration are never written:
 *   out[b, p] = sum_a labels[a] * softmax_a( sign * (X[b,a,p] + G[b,a,p]) ),   sign = negate ? -1 : +1
 * X, G: contiguous fp32 [B][L][n] on the device (G may be NULL), labels fp32 [L] on the device or NULL for 0, 1, ..,
 * L-1, out [B][n].  Any L >= 1, any n, any B.  A thread owns four pixels and walks the label planes once, eight planes
 * in flight, with a running maximum, sum and label-weighted sum per pixel (rescaled once per eight planes when the
 * maximum rises; the arithmetic between the fp32 loads and stores is float64); it ends with one division per pixel.
 * float4 accesses along the pixel axis when n % 4 == 0 and X / G / out are 16-byte aligned, dwords otherwise.  No LDS,
 * no atomics, a fixed label order: the same bits on every run.
 * phl_nchw_expected_value_grad: with z = sign * (X + G), q = softmax(z), d = sum_a labels[a] q_a and the upstream
 * gradient gout [B][n]:   gZ[b,a,p] = sign * gout[b,p] * q_a * (labels[a] - d)   -- the gradient of X and of G alike,
 * [B][L][n].  Nothing but the forward's inputs is needed: the kernel recomputes the column's maximum, sum and d (the
 * forward's code) and then reads X and G a second time to write gZ.  There is no gradient for the labels.
 * Status, checked before any HIP call: PHL_ERR_INVALID for negative sizes or L < 1; then zero elements (B == 0 or
 * n == 0) are PHL_OK with nothing launched; then PHL_ERR_INVALID for NULL X / out (gout / gZ) or an output that is one
 * of the inputs; PHL_ERR_TOO_LARGE when B*L*n*4 bytes leave int64 or the workgroups (PHL_NCHW_EXPECT_PIXELS pixels
 * each) leave 2^31 - 1.  Every label count is taken: there is no PHL_ERR_UNSUPPORTED. */
#define PHL_NCHW_EXPECT_PIXELS 1024
int phl_nchw_expected_value(const float *X_dev, const float *G_dev, const float *labels_dev, float *out_dev, int B, int L,
                            int64_t n, int negate, phl_stream stream);
int phl_nchw_expected_value_grad(const float *X_dev, const float *G_dev, const float *labels_dev, const float *gout_dev,
                                 float *gZ_dev, int B, int L, int64_t n, int negate, phl_stream stream);
/* ---- the unary energies of the upsampler head from a scalar disparity (crf/mb_stereo_crf.py, CRFdepthUpsampler) ------
 * For disp [B][1][h][w] and an output size (H, W): up[b,y,x] = torch's bilinear interpolation with align_corners=False,
 * no antialias, any ratio (src = max(0, (dst + 0.5) * in/out - 0.5), i0 = floor(src), i1 = min(i0 + 1, in - 1), lambda =
 * src - i0), evaluated in float64 from the fp32 samples; lmax = the fp32 value nearest to max(up) over the batch;
 * labels[i] = the fp32 value nearest to lmax * i / (L - 1) (labels[0] = 0, labels[L-1] = lmax exactly);
 *   E0[b,a,y,x] = scale * exp(s) * (sqrt(g^2 + d^2) - g),  g = gamma * lmax,  d = labels[a] - up[b,y,x]
 * where (float)up > (float)threshold, and +0.0 elsewhere -- the reference's -(-10 get_energies_from_scalar(up, labels)) *
 * (up > 1e-2) with scale = 10, threshold = 1e-2.  Float64 between the fp32 loads and the one fp32 store.
 * phl_nchw_scalar_unaries: two launches on the stream, nothing read back.  The first evaluates up per output pixel (no
 * [B][H][W] plane is written), reduces the maximum and writes labels[L]; the second writes E0 [B][L][H*W], a thread owning
 * four pixels and walking the L planes: float4 stores when H*W % 4 == 0 and E0 is 16-byte aligned, dwords otherwise.
 * gamma, s: one fp32 value each IN DEVICE MEMORY (charb's parameters).  Its scratch (the maxima of the at most 256 workgroups of the first launch) is a
 * stream-ordered allocation.
 * phl_nchw_scalar_unaries_grad: from disp, labels (the forward's), gamma, s and the upstream gE0 [B][L][H*W]
 *   grad[0] = grad_gamma = sum gE0 * c * scale * exp(s) * lmax * (g / r - 1),  r = sqrt(g^2 + d^2)  (r == 0: the term is 0)
 *   grad[1] = grad_s     = sum gE0 * E0
 * with c the mask above and lmax = labels[L-1].  gE0 is read once, everything else recomputed; products and sums are
 * float64, one partial pair per workgroup added in index order by a second kernel: no atomics, the same bits on every
 * call.  disp, labels and lmax get no gradient (the reference's float(up.max()) cuts that graph).
 * Status, checked before any HIP call: PHL_ERR_INVALID for L < 2, any of h, w, H, W < 1 or B < 0; then B == 0 is PHL_OK
 * with nothing launched; then PHL_ERR_INVALID for a NULL pointer or an output that is one of the inputs;
 * PHL_ERR_TOO_LARGE when B*L*H*W*4 or B*h*w*4 bytes leave int64 or the workgroups (PHL_NCHW_SCALAR_PIXELS pixels each)
 * leave 2^31 - 1. */
#define PHL_NCHW_SCALAR_PIXELS 1024
int phl_nchw_scalar_unaries(const float *disp_dev, const float *gamma_dev, const float *s_dev, float *E0_dev, float *labels_dev,
                            int B, int h, int w, int H, int W, int L, double scale, double threshold, phl_stream stream);
int phl_nchw_scalar_unaries_grad(const float *disp_dev, const float *labels_dev, const float *gamma_dev, const float *s_dev,
                                 const float *gE0_dev, float *grad_dev, int B, int h, int w, int H, int W, int L, double scale,
                                 double threshold, phl_stream stream);
/* ---- the unary energies from logits and a per-pixel confidence (crf/crf_module.py, CRFasRNN: -logits * confidence) ----
 * logits, E0, gE0, grad_logits: contiguous fp32 [B][L][n] on the device, n = H*W; conf, grad_conf: [B][n].
 *   phl_nchw_confidence_unaries        E0[b,a,p] = -(logits[b,a,p] * conf[b,p])
 *   phl_nchw_confidence_unaries_grad   for the upstream gradient gE0 of E0:
 *                                      grad_conf[b,p]     = -sum_a logits[b,a,p] * gE0[b,a,p]
 *                                      grad_logits[b,a,p] = -(conf[b,p] * gE0[b,a,p])
 * One kernel each.  A thread owns four pixels, loads their confidences once and walks the label planes, eight planes in
 * flight: the forward reads the logits once and writes E0 once; the backward reads gE0 once, the logits once where
 * grad_conf is asked for and the confidences where grad_logits is.  Either of grad_conf / grad_logits may be NULL, and
 * that part is then neither computed nor stored (nor its operand read); the other part's bits do not depend on it; both
 * NULL is PHL_ERR_INVALID.  E0 and grad_logits are one correctly rounded fp32 product each, negated: on finite inputs the
 * bits of torch's (-logits) * confidence and -(gE0 * confidence), signed zeros included.  grad_conf: the products (exact)
 * and the sum are float64, added in label order a = 0 .. L-1, and stored as fp32 once.  float4 accesses along the pixel
 * axis when n % 4 == 0 and every pointer is 16-byte aligned, dwords otherwise.  No LDS, no atomics, no scratch: the same
 * bits on every call.
 * Status, checked before any HIP call: PHL_ERR_INVALID for negative sizes or L < 1; then zero elements (B == 0 or
 * n == 0) are PHL_OK with nothing launched; then PHL_ERR_INVALID for a NULL logits / conf / E0 (gE0; both of grad_conf
 * and grad_logits) or an output that is one of the inputs or the other output; PHL_ERR_TOO_LARGE when B*L*n*4 bytes
 * leave int64 or the workgroups (PHL_NCHW_CONF_PIXELS pixels each) leave 2^31 - 1.  Every label count is taken: there is
 * no PHL_ERR_UNSUPPORTED. */
#define PHL_NCHW_CONF_PIXELS 1024
int phl_nchw_confidence_unaries(const float *logits_dev, const float *conf_dev, float *E0_dev, int B, int L, int64_t n,
                                phl_stream stream);
int phl_nchw_confidence_unaries_grad(const float *logits_dev, const float *conf_dev, const float *gE0_dev,
                                     float *grad_conf_dev /* [B][n] or NULL */, float *grad_logits_dev /* [B][L][n] or NULL */,
                                     int B, int L, int64_t n, phl_stream stream);
/* ---- backward of the compatibility + softmax step (CRF training) ---------------------------------------------
 * Forward: Q = softmax(-E), E = E0 + X Mu.  With the upstream gradient gQ: dE = Q (s - gQ), s[p] = sum_c gQ[p,c] Q[p,c];
 * gE0 = dE, gX = dE Mu^T, gMu = X^T dE.  All entry points: fp32 rows with unit channel stride, row strides % 4 == 0,
 * 16-byte aligned pointers, L % 4 == 0, 4 <= L <= 512 (else PHL_ERR_UNSUPPORTED), any n.
 *   phl_softmax_neg_grad      dE from Q and gQ in one pass (the backward of phl_softmax_neg_add as well).
 *   phl_uniform_compat_grad   the same pass for Mu = alpha*J + beta*I, which also writes gX = alpha*rowsum(dE) + beta*dE;
 *                             Q == NULL: logits mode (the step returned -E), dE = -gQ.
 *   phl_compat_grad_x         gX = scale * dE Mu^T on the f32-input matrix cores (exact f32); Mu is the [L][L] matrix
 *                             itself, row stride L, NOT transposed.  scale = -1 with dE = g_out serves logits mode.
 *   phl_compat_mu_grad        gMu = scale * X^T dE (+ gMu if accumulate) into a dense [L][L]: one fp32 partial per pixel
 *                             range into the workspace, then the partials summed in range order in fp64 -- no atomics,
 *                             the result is the same bit for bit on every run.
 *   phl_compat_mu_grad_workspace_bytes(n, L) = R * L * L * 4 with R = max(1, min(ceil(n / 64), C, floor(2^24 / L^2)))
 *                             pixel ranges, C = floor(256 * max(1, floor(16 / (c * min(c, floor(16 / c))))) / slabs),
 *                             c = ceil(L / 64), slabs = ceil(L / (64 min(c, floor(16 / c)))); where slabs > 1 and R >= 8,
 *                             R is rounded down to a multiple of 8.  At most 64 MiB; 0 for an L the kernels do not take. */
int phl_softmax_neg_grad(const float *Q_dev, int64_t q_row_stride, const float *gQ_dev, int64_t gq_row_stride, float *dE_dev,
                         int64_t de_row_stride, int64_t n, int L, phl_stream stream);
int phl_uniform_compat_grad(const float *Q_dev, int64_t q_row_stride, const float *gQ_dev, int64_t gq_row_stride, float alpha,
                            float beta, float *dE_dev, int64_t de_row_stride, float *gX_dev, int64_t gx_row_stride, int64_t n,
                            int L, phl_stream stream);
int phl_compat_grad_x(const float *dE_dev, int64_t de_row_stride, const float *mu_dev, float scale, float *gX_dev,
                      int64_t gx_row_stride, int64_t n, int L, phl_stream stream);
size_t phl_compat_mu_grad_workspace_bytes(int64_t n, int L);
int phl_compat_mu_grad(const float *X_dev, int64_t x_row_stride, const float *dE_dev, int64_t de_row_stride, float scale,
                       int64_t n, int L, void *workspace_dev, float *gMu_dev, int accumulate, phl_stream stream);
/* out[p] = sum_c Q[p,c]*labels[c] : the expected disparity `mf @ labels`
 * (Experiments/DenseCrf.ipynb cell 11). */
int phl_expected_value(const float *Q_dev, int64_t q_row_stride, const float *labels_dev, float *out_dev,
                       int64_t n, int L, phl_stream stream);

/* ---- caller side of the path: the unary cost volume E_0 ---------------------
 * disparity_badness(img1, img2, window_size, criterion), crf/depth.py:36-53, on the device:
 *   out[(y*w+x)*out_row_stride + k] = sum over the window x window neighbourhood (scipy 'reflect'
 *   borders on the cost array, :51-52) of  sum_ch criterion(img1[y,x,ch], img2[y,x-k,ch])  with
 *   img2 = 0 left of the image (:44-50), k = 0..max_disp-1.
 * img1/img2: [h][w][channels] fp32 device arrays (1..4 channels), window odd <= 17,
 * criterion 0 = AD (:26-27), 1 = SD (:24-25), 2 = nprod (:28-29).  The reference takes
 * max_disp = w // 6 (:40); here it is the caller's argument.  Output is pixel-major fp32, the
 * layout phl_filter reads. */
int phl_cost_volume(const float *img1_dev, const float *img2_dev, int h, int w, int channels, int max_disp,
                    int window, int criterion, float *out_dev, int64_t out_row_stride, phl_stream stream);

/* ---- the same sweep for the channel-major consumers, and its winner-takes-all disparity (phl_costvol_nchw.hip;
 * what it shares with phl_costvol.hip: phl_costvol_common.h) ----
 * crf/dataloader.py:54-57,83: the unary logits of CRFdepthRefiner / CRFwUncertainty are -1 * disparity_badness(left,
 * right, ws, criterion), permuted to [L, H, W]; crf/depth.py:31-34: disparity_estimate is the argmin of
 * disparity_badness (crf/depth.py:36-53, the mathematics of phl_cost_volume above) over the disparities.
 *   phl_cost_volume_nchw  out[b*out_bs + k*out_ls + y*out_ys + x] = cost(b, y, x, k), or -cost with
 *                         PHL_COSTVOL_NEGATE (the reference's logits; a cost of exactly 0 becomes -0.0, as -1 * 0.0).
 *   phl_disparity_wta     disp[b*o_bs + y*o_ys + x] = the smallest k that attains min_k cost(b, y, x, k), as np.argmin;
 *                         cost_dev, when not NULL, gets that minimum (positive cost) at the same strides.  Nothing of
 *                         size h*w*max_disp is allocated or written.  Its window sums are formed by the same device
 *                         code, tile geometry and order as phl_cost_volume_nchw's: the result is the argmin of that
 *                         call's output bit for bit.  Inputs are taken as finite.
 * Both images are read in place through one set of ELEMENT strides (batch, row, column, channel): interleaved
 * [H][W][C] is (0, W*C, C, 1) with batch 1, planar [B][C][H][W] is (C*H*W, W, 1, H*W).  1..4 channels, odd window
 * <= 17, criterion 0 = AD, 1 = SD, 2 = nprod.  The x stride of every output is 1; rows may start off the 16-byte grid
 * (they are then written with 4-byte stores).  A workgroup makes PHL_COSTVOL_NCHW_TY x _TX pixels for _DC disparities.
 * Deterministic: no atomics, the same bytes on every call.
 * Status, checked in this order and before any HIP call: PHL_ERR_UNSUPPORTED for channels, window or criterion outside
 * that set or unknown flag bits; PHL_ERR_INVALID for negative sizes, and for max_disp == 0 in phl_disparity_wta (an
 * argmin over nothing); then batch == 0, h*w == 0 or (volume) max_disp == 0 are PHL_OK with nothing launched, whatever
 * the pointers; PHL_ERR_INVALID for a NULL image or output, for out_ys < w, out_ls smaller than what h rows span or
 * out_bs smaller than what one item spans (rows would overlap), and for an output that overlaps an image (or cost_dev
 * overlapping disp_dev); PHL_ERR_TOO_LARGE when byte offsets leave int64 or the workgroups leave 2^31 - 1. */
#define PHL_COSTVOL_NEGATE 1u
#define PHL_COSTVOL_NCHW_TX 64
#define PHL_COSTVOL_NCHW_TY 8
#define PHL_COSTVOL_NCHW_DC 8
int phl_cost_volume_nchw(const float *img1_dev, const float *img2_dev, int batch, int h, int w, int channels,
                         int64_t img_bs, int64_t img_ys, int64_t img_xs, int64_t img_cs,
                         int max_disp, int window, int criterion, unsigned flags,
                         float *out_dev, int64_t out_bs, int64_t out_ls, int64_t out_ys, phl_stream stream);
int phl_disparity_wta(const float *img1_dev, const float *img2_dev, int batch, int h, int w, int channels,
                      int64_t img_bs, int64_t img_ys, int64_t img_xs, int64_t img_cs,
                      int max_disp, int window, int criterion,
                      int32_t *disp_dev, float *cost_dev /* may be NULL */, int64_t o_bs, int64_t o_ys, phl_stream stream);

/* ---- separable Gaussian of the guided filter (crf/guided.py: box_filter, gaussian_blur) -------------------------
 * Dense contiguous fp32 viewed as [outer][h][inner]; every (outer, inner) line is filtered along h by `passes` box
 * passes  B_r(x)[i] = sum(x[max(0, i-r+1) .. min(h-1, i+r)]) / (min(i, r) + min(h-1-i, r) + 1).
 *   phl_box_blur        dst = B_r^passes(src), all passes in one kernel while its LDS fits (r up to
 *                       phl_box_blur_fused_max_r), else one launch per pass through stream-ordered temporaries.
 *                       src and dst must not overlap.
 *   phl_box_blur_grad   the backward of the 3-pass Gaussian with f[i] = i / sigma:
 *                         grad_x     = B(g)                                     (written if grad_x != NULL)
 *                         grad_sigma = -sum(grad_f f) / sigma - sum(B(g) v) / sigma,
 *                         grad_f     = -(v f B(g) - v B(g f) + g f B(v) - g B(v f))
 *                       as one fp32 on the device (written if grad_sigma_dev != NULL; per-workgroup fp64 partials in
 *                       a stream-ordered temporary, summed in a fixed order: the same bits on every run).  Without
 *                       grad_sigma_dev it is phl_box_blur(g, grad_x, ..., 3).
 * Status, checked before any HIP call: PHL_ERR_INVALID for negative sizes, r < 1, passes outside 1..8, sigma not
 * > 0, NULL data pointers (when there is at least one element), src == dst, grad_x aliasing v / g, or neither grad_x
 * nor grad_sigma_dev; PHL_ERR_TOO_LARGE when outer*h*inner*4 bytes leave int64 or the lines make more than 2^31-1
 * workgroups; PHL_ERR_UNSUPPORTED from phl_box_blur_grad with grad_sigma_dev when min(r, h) exceeds
 * phl_box_blur_fused_max_r(inner == 1, 3, 1) (the caller then composes it from phl_box_blur calls).
 * Zero elements: PHL_OK (grad_sigma_dev set to 0). */
int phl_box_blur(const float *src_dev, float *dst_dev, int64_t outer, int64_t h, int64_t inner, int r, int passes,
                 phl_stream stream);
int phl_box_blur_grad(const float *v_dev, const float *g_dev, int64_t outer, int64_t h, int64_t inner, int r, double sigma,
                      float *grad_x_dev, float *grad_sigma_dev, phl_stream stream);
/* largest r the single fused kernel takes for these passes (grad != 0: phl_box_blur_grad's); INT32_MAX for one pass */
int phl_box_blur_fused_max_r(int inner_is_one, int passes, int grad);

/* ---- box-window guided filter (crf/guided.py: GuidedFilter, FastGuidedFilter, BatchedGuidedAdjacency) -------------
 * Forward only.  Contiguous NCHW fp32: y [B][cy][H][W] (filtered), x [B][cx][H][W] (guide), out [B][cy][H][W], src NULL
 * or [B][cy][H][W].  S_r(t) = sum of t over the (2r+1)^2 window clipped to the image, mean(t) = S_r(t) / S_r(1).  The
 * linear model is solved at the resolution h x w <= H x W on nearest samples (FastGuidedFilter; h = H, w = W and
 * identity maps give the plain filter), with r the radius AT THAT RESOLUTION:
 *   yl = y[.., row_of_low[i], col_of_low[j]], xl likewise
 *   A_lc = (mean(yl_l xl_c) - mean(yl_l) mean(xl_c)) / (mean(xl_c^2) - mean(xl_c)^2 + eps[c])
 *   b_l  = mean(yl_l) - sum_c A_lc mean(xl_c)
 *   out_l[I][J] = (sum_c mean(A_lc)[i][j] x_c[I][J] + mean(b_l)[i][j]) * scale - src_l[I][J],  i = low_of_row[I], j = low_of_col[J]
 * Index maps are int32 on the device: row_of_low [h], col_of_low [w] (values in 0..H-1 / 0..W-1) and low_of_row [H],
 * low_of_col [W] (non-decreasing, values in 0..h-1 / 0..w-1) -- torch's own nearest maps, see phl.guided_filter.
 * eps: [cx] fp32 on the device.  Window sums are kept in fp64 over direct sliding windows (no image-long prefix sums);
 * no atomics: the same bits on every run.  Temporaries are stream-ordered allocations.
 * Status, checked before any HIP call: PHL_ERR_INVALID for negative sizes, cx < 1, r < 0, h > H, w > W, an empty solving
 * resolution of a non-empty image, a non-finite scale, NULL pointers (src may be NULL) or out aliasing an input;
 * PHL_ERR_TOO_LARGE when H*W or B*cy leave int32, a side exceeds 2^30 or the byte counts leave int64;
 * PHL_ERR_UNSUPPORTED for cx > PHL_GUIDED_MAX_CX (the caller keeps its torch path).  Any r: while
 * min(r, max(h, w)) <= phl_guided_filter_max_r() a workgroup keeps its tile and halo in LDS; above it the same kernels
 * run their streamed form, which reads the image from memory in strips and needs no LDS that grows with r (slower).
 * Zero elements: PHL_OK. */
#define PHL_GUIDED_MAX_CX 16
int phl_guided_filter(const float *y_dev, const float *x_dev, const float *src_dev, float *out_dev, int B, int cy, int cx, int H,
                      int W, int h, int w, int r, const int *row_of_low_dev, const int *col_of_low_dev, const int *low_of_row_dev,
                      const int *low_of_col_dev, const float *eps_dev, float scale, phl_stream stream);
/* The same filter with the full covariance of the guide channels (the model the reference keeps as commented lines,
 * crf/gaussian_matrix.py:204-212; its backward: phl_guided_filter_full_grad); arguments, maps, window sums and out exactly as phl_guided_filter, but
 *   S_cd = mean(xl_c xl_d) - mean(xl_c) mean(xl_d)      P = (S + diag(eps))^-1      A_lc = sum_d cov_ld P_dc
 * with cov_ld = mean(yl_l xl_d) - mean(yl_l) mean(xl_d); cx = 1 is the model above.  P is computed once per image in fp64
 * (L D L^T without pivoting; a non-positive pivot, eps <= 0 on a flat window, gives inf or nan) and kept as
 * cx (cx + 1) / 2 fp64 planes at the solving resolution; A is rounded to fp32 once.  No atomics: the same bits on every run.
 * Status as phl_guided_filter, then PHL_ERR_UNSUPPORTED for cx > PHL_GUIDED_FULL_MAX_CX (the caller keeps its torch
 * path), all before any HIP call.  The tiled radius and the labels per chunk are those of phl_guided_filter. */
#define PHL_GUIDED_FULL_MAX_CX 4
int phl_guided_filter_full(const float *y_dev, const float *x_dev, const float *src_dev, float *out_dev, int B, int cy, int cx, int H,
                           int W, int h, int w, int r, const int *row_of_low_dev, const int *col_of_low_dev,
                           const int *low_of_row_dev, const int *low_of_col_dev, const float *eps_dev, float scale,
                           phl_stream stream);
int phl_guided_filter_max_r(void);  /* largest window radius (at the solving resolution) of the LDS-tiled form */
/* Labels (planes of y) per chunk of a call: the labels B * cy are processed in chunks whose per-label temporaries stay
 * within a fixed budget.  h x w is the solving resolution; needs = -1 asks for phl_guided_filter, otherwise for
 * phl_guided_filter_grad with the bit mask 1 = grad_y, 2 = grad_x, 4 = grad_eps, and full != 0 for h x w = H x W (the
 * forward ignores it).  Host arithmetic only, no HIP call; the same function sizes the chunks of the two entry points.
 * 0 for sizes below 1 or another needs. */
int phl_guided_filter_labels_per_chunk(int B, int cy, int cx, int h, int w, int full, int needs);

/* Backward of phl_guided_filter with src = NULL (subtract_is_y = 0) or src = y (subtract_is_y != 0): g [B][cy][H][W] is the
 * gradient of out; grad_y [B][cy][H][W], grad_x [B][cx][H][W] and grad_eps [cx] are written (never accumulated into), each
 * may be NULL, all three NULL is PHL_OK with nothing launched.  Nothing of the forward is saved: the statistics and the
 * coefficients are recomputed from y, x and eps.  row_of_low / col_of_low must be strictly increasing (torch's nearest
 * maps are), so that the samples of two low-resolution pixels never coincide.  Window sums, label sums and every product
 * that feeds them are fp64; labels are summed in index order and grad_eps by a fixed two-stage reduction, without
 * atomics: the same bits on every run.  Every gradient is rounded to fp32 once.  Temporaries are stream-ordered
 * allocations, among them one fp64 plane [B][cx][H][W] when grad_x is asked for.
 * Status as phl_guided_filter (checked before any HIP call; g must not be NULL; a gradient must not alias an input or
 * another gradient).  Any r: above phl_guided_filter_grad_max_r() the streamed form of the window sums runs. */
int phl_guided_filter_grad(const float *y_dev, const float *x_dev, const float *g_dev, float *grad_y_dev, float *grad_x_dev,
                           float *grad_eps_dev, int B, int cy, int cx, int H, int W, int h, int w, int r,
                           const int *row_of_low_dev, const int *col_of_low_dev, const int *low_of_row_dev,
                           const int *low_of_col_dev, const float *eps_dev, float scale, int subtract_is_y, phl_stream stream);
int phl_guided_filter_grad_max_r(void);   /* largest radius of the backward's LDS-tiled form */
/* Backward of phl_guided_filter_full: the argument list, the outputs, the maps and the rules of phl_guided_filter_grad.
 * With P, A and cov_ld as there, gA_lc / gb_l the window-summed gradients of mean(A) / mean(b), gA'_lc = gA_lc - gb_l m_c:
 *   gcov_ld = sum_c gA'_lc P_cd      gS_cd = -1/2 sum_l (A_lc gcov_ld + A_ld gcov_lc)      grad_eps_c = sum gS_cc
 * and gS enters grad_x through all cx (cx + 1) / 2 products xl_c xl_d.  mx and P are recomputed once per call (fp64), the
 * per-label terms of gS and of the gradient of mean(xl) are fp64 planes summed over the labels in index order; no atomics,
 * the same bits on every run, every gradient rounded to fp32 once.
 * Status as phl_guided_filter_grad, then (after the zero-element return) PHL_ERR_UNSUPPORTED for
 * cx > PHL_GUIDED_FULL_MAX_CX, then the aliasing check; all before any HIP call.  The tiled radius is
 * phl_guided_filter_grad_max_r(). */
int phl_guided_filter_full_grad(const float *y_dev, const float *x_dev, const float *g_dev, float *grad_y_dev, float *grad_x_dev,
                                float *grad_eps_dev, int B, int cy, int cx, int H, int W, int h, int w, int r,
                                const int *row_of_low_dev, const int *col_of_low_dev, const int *low_of_row_dev,
                                const int *low_of_col_dev, const float *eps_dev, float scale, int subtract_is_y, phl_stream stream);
/* Labels per chunk of a phl_guided_filter_full_grad call; needs is the bit mask 1 = grad_y, 2 = grad_x, 4 = grad_eps, the
 * other arguments as phl_guided_filter_labels_per_chunk.  0 for sizes below 1, cx > PHL_GUIDED_FULL_MAX_CX or another needs. */
int phl_guided_filter_full_grad_labels_per_chunk(int B, int cy, int cx, int h, int w, int full, int needs);

/* FastGuidedFilter(mode='bilinear'), the forward (backward: phl_guided_filter_bilinear_grad): the tensors, eps, the window sums and the status rules of
 * phl_guided_filter, but no index maps -- with D = F.interpolate(., size=(h, w), mode='bilinear') and
 * U = F.interpolate(., size=(H, W), mode='bilinear') (align_corners=False, no antialias)
 *   (mean(A), mean(b)) = the model of phl_guided_filter on D(y), D(x), r the radius at h x w
 *   out_l = (sum_c U(mean(A_lc)) x_c + U(mean(b_l))) * scale - src_l
 * and with PHL_GUIDED_BILINEAR_FULL_COV in flags the model of phl_guided_filter_full.  Per axis the taps of output
 * index o, mapping n_in samples to n_out, are torch's, computed on the device in fp64:
 *   s = max((o + 0.5) * (n_in / n_out) - 0.5, 0)   i0 = min(int(s), n_in - 1)   i1 = min(i0 + 1, n_in - 1)   lam = s - i0
 * D(y) and D(x) are rounded to fp32 once (never written to memory); from there on the roundings are those of
 * phl_guided_filter; U and the sum over the channels are fp64, out is rounded once.  No atomics: the same bits on
 * every run.  Temporaries are stream-ordered: the statistics, and per chunk of labels 2 (cx + 1) fp32 planes at h x w.
 * Status, before any HIP call: as phl_guided_filter (without the maps); then, after the zero-element return,
 * PHL_ERR_UNSUPPORTED for unknown flag bits or, with the flag, cx > PHL_GUIDED_FULL_MAX_CX; then PHL_ERR_INVALID for
 * out aliasing an input.  The tiled radius is phl_guided_filter_max_r(). */
#define PHL_GUIDED_BILINEAR_FULL_COV 1u
int phl_guided_filter_bilinear(const float *y_dev, const float *x_dev, const float *src_dev, float *out_dev, int B, int cy, int cx,
                               int H, int W, int h, int w, int r, const float *eps_dev, float scale, unsigned flags,
                               phl_stream stream);
/* Labels per chunk of a phl_guided_filter_bilinear call (the window-mean planes join the coefficient planes in the
 * budget); host arithmetic only.  0 for sizes below 1. */
int phl_guided_filter_bilinear_labels_per_chunk(int B, int cy, int cx, int h, int w);
/* Backward of phl_guided_filter_bilinear (the diagonal model, flags = 0) with src = NULL (subtract_is_y = 0) or src = y
 * (subtract_is_y != 0): g, the three gradients (each may be NULL, all NULL is PHL_OK with nothing launched), the
 * recomputation from y, x and eps, the fp64 sums in a fixed order without atomics and the single rounding of every
 * gradient are those of phl_guided_filter_grad.  D(y) and D(x) are taken again with the forward's taps, weights and
 * rounding, so the model is the forward's bit for bit; the gradients of mean(A) and mean(b) are scale * U^T(g x_c) and
 * scale * U^T(g), gathered per low-resolution pixel over the one range of rows and columns whose taps of U include it;
 * grad_x gets scale * sum_l g_l U(mean(A_lc)) with U's four taps; and the gradients of D(y), D(x) return through D^T.
 * D^T is a gather as well, and that rests on one assumption: with H >= 2 h the source coordinates of consecutive
 * samples of D are at least 2 apart, so a full-resolution row is a tap of at most one low-resolution row (columns
 * likewise with W >= 2 w), and every full-resolution pixel is written once, with 0 where it is nobody's tap.  Hence
 * 2 h <= H and 2 w <= W are required.
 * Status, before any HIP call: as phl_guided_filter_bilinear (g must not be NULL); then, after the zero-element return,
 * PHL_ERR_UNSUPPORTED for cx > PHL_GUIDED_MAX_CX, for any flag bit (PHL_GUIDED_BILINEAR_FULL_COV included: the
 * full-covariance backward is phl_guided_filter_bilinear_full_grad below) and for 2 h > H or 2 w > W; then
 * PHL_ERR_INVALID for a gradient aliasing an input or another gradient.  The tiled radius is
 * phl_guided_filter_grad_max_r().  The per-label temporaries are those of phl_guided_filter_grad below full resolution,
 * so phl_guided_filter_labels_per_chunk(B, cy, cx, h, w, 0, needs) gives the labels per chunk of this call too. */
int phl_guided_filter_bilinear_grad(const float *y_dev, const float *x_dev, const float *g_dev, float *grad_y_dev,
                                    float *grad_x_dev, float *grad_eps_dev, int B, int cy, int cx, int H, int W, int h, int w,
                                    int r, const float *eps_dev, float scale, int subtract_is_y, unsigned flags,
                                    phl_stream stream);
/* Backward of phl_guided_filter_bilinear(..., flags = PHL_GUIDED_BILINEAR_FULL_COV) with src = NULL (subtract_is_y = 0)
 * or src = y (subtract_is_y != 0): the gradients of phl_guided_filter_full_grad (gcov, gS, grad_eps_c = sum gS_cc, gS
 * entering grad_x through all cx (cx + 1) / 2 products) on the low-resolution planes, connected to the full resolution
 * by the four bilinear pieces of phl_guided_filter_bilinear_grad: D(y) and D(x) taken again with the forward's taps,
 * weights and rounding, so that mx, P and A are the forward's bit for bit; scale * U^T(g x_c) and scale * U^T(g) as
 * gathers; scale * sum_l g_l U(mean(A_lc)) with U's four taps in grad_x; and D^T as the gather of the one
 * low-resolution pixel that taps a full-resolution one, which requires 2 h <= H and 2 w <= W as there.  fp64 window
 * sums, labels summed in index order, a fixed two-stage grad_eps reduction, no atomics, every gradient rounded once.
 * Status, before any HIP call: as phl_guided_filter_bilinear_grad up to the zero-element and nothing-asked-for returns
 * (there are no flags); then PHL_ERR_UNSUPPORTED for cx > PHL_GUIDED_FULL_MAX_CX, then for 2 h > H or 2 w > W; then
 * PHL_ERR_INVALID for a gradient aliasing an input or another gradient.  The tiled radius is
 * phl_guided_filter_grad_max_r().  The per-label temporaries are those of phl_guided_filter_full_grad below full
 * resolution, so phl_guided_filter_full_grad_labels_per_chunk(B, cy, cx, h, w, 0, needs) gives the labels per chunk of
 * this call too. */
int phl_guided_filter_bilinear_full_grad(const float *y_dev, const float *x_dev, const float *g_dev, float *grad_y_dev,
                                         float *grad_x_dev, float *grad_eps_dev, int B, int cy, int cx, int H, int W, int h,
                                         int w, int r, const float *eps_dev, float scale, int subtract_is_y,
                                         phl_stream stream);

/* Plain float4 streaming copy dst <- src (n_floats % 4 == 0, 16-byte aligned): measures the
 * HBM read+write ceiling of the box that the roofline fractions are compared with. */
int phl_stream_copy(const float *src_dev, float *dst_dev, int64_t n_floats, phl_stream stream);
/* dst[r*dst_rs + c*dst_cs] = src[r*src_rs + c*src_cs] for rows x cols floats (LDS-tiled: both sides coalesced): the
 * transpose between the reference's NCHW tensors (BatchedAdjacency's channel-major [n, L] views,
 * crf/gaussian_matrix.py:345-349) and the pixel-major rows the kernels work on.  Current device, given stream. */
int phl_copy2d(const float *src_dev, int64_t src_row_stride, int64_t src_col_stride, float *dst_dev, int64_t dst_row_stride,
               int64_t dst_col_stride, int64_t rows, int cols, phl_stream stream);

/* Chunk ("tile") statistics of the LDS-staged path: out[0]=pixels per chunk, [1]=#chunks,
 * [2]=max local vertices per chunk, [3]=(chunk,vertex) slots S, [4]=slots of vertices fed by
 * several chunks, [5]=1 if the staged splat / [6]=slice would be chosen for this vd. */
int phl_tile_stats(const phl_lattice *lat, int vd, int64_t out[7]);

/* ---- introspection for parity tests (synchronous device->host copies) ---------------------
 * Vertex ids in these calls are the reference's: first-touch (insertion) order, the numbering its hash table
 * produces.  ROWS of the [M][vd] vertex buffers the stage-level calls take are in the library's internal
 * (locality) order instead: row_of_vertex[v] = row that holds first-touch vertex v; phl_add_vertices returns rows.
 * Ghost vertices come last in both numberings. */
int phl_get_vertex_order(phl_lattice *lat, int32_t *row_of_vertex_host /* [M] */);
/* Pixels in chunk order: chunk c of the LDS-staged kernels holds pixels pix_order[c*P ... (c+1)*P), P = phl_tile_stats()[0]. */
int phl_get_pixel_order(phl_lattice *lat, int32_t *pix_order_host /* [n] */);
int phl_get_keys(phl_lattice *lat, int16_t *keys_host /* [M][d] */);
int phl_get_replay(phl_lattice *lat, int32_t *vid_host /* [n][d+1] */, float *w_host /* [n][d+1] */);
int phl_get_neighbors(phl_lattice *lat, int32_t *nbr_host /* [d+1][M][2], -1 = absent */);
/* The line lists of the three-axes-per-pass blur (axis groups (3g, 3g+1 | 3g+2), built where the blur runs at least one
 * triple and the lattice has no ghost vertices).  info = { groups, work items per group, nominal item size }, all 0
 * where there are none; with the three arrays null only info is filled.  Group `group`: vertex_host[i] = first-touch
 * id of list entry i (every vertex once, in line order along axis 3g+2); flags_host[i] = minus | plus << 2, where the
 * two outer operands of the last blur come from: 0 absent (zero), 1 the neighbouring entry's value, 2 evaluated from
 * neighbors()[3g+2][v]; work item k is entries [item_start_host[k], item_start_host[k+1]). */
int phl_get_blur_lines(phl_lattice *lat, int group, int32_t *vertex_host /* [M] */, int32_t *flags_host /* [M] */,
                       int32_t *item_start_host /* [items + 1] */, int64_t info[3]);
int phl_get_splat_lists(phl_lattice *lat, int32_t *ptr_host /* [M+1] */, int32_t *pixel_host /* [n(d+1)] */,
                        float *w_host /* [n(d+1)] */);

/* Test hook, host only (no device needed): the table replay behind PHL_BUILD_REFERENCE_TABLE on host arrays.
 * keys_clean [M][d] = distinct keys in first-touch order, cand_vid [N] = index into them for every
 * (pixel, remainder) candidate in order.  Returns the reference's key list (insertion order, duplicates
 * included), the vertex every candidate's lookup resolved to, the vertices its final table cannot reach and
 * the neighbour a doubling inside blur() decides (-2: no such doubling). */
int phl_debug_reference_table(const int16_t *keys_clean, const int32_t *cand_vid, int64_t M, int d, int64_t N,
                              int16_t *keys_ref_out, int64_t keys_ref_cap, int64_t *M_ref_out,
                              int32_t *cand_ref_vid_out, int32_t *hidden_out, int hidden_cap, int *n_hidden_out,
                              int *blur_first_nbr_out);

/* Test hook: the one assumption of the analytic table replay -- no tracked key's probe path in the reference's table
 * (linear probing, permutohedral.h:84-106, capacity `cap` = a power of two >= 2^15) runs past the last slot -- checked
 * for a caller-made key set on the device (on_device = 1: the kernels the build uses) or on the host (0).
 * keys_clean [n_clean][d]; extra_clean / stale_clean / check index into it (entries filed a second time under `cap`,
 * entries filed under cap / 2, keys whose paths are asked about).  *result_out = 1 if none wraps. */
int phl_debug_probe_paths(const int16_t *keys_clean, int64_t n_clean, int d, const int32_t *extra_clean, int n_extra,
                          const int32_t *stale_clean, int n_stale, uint64_t cap, const int32_t *check, int n_check,
                          int on_device, int *result_out);

/* Test hook: dst <- src (n_floats % 4 == 0, 16-byte aligned) copied `repeat` times by `workgroups` workgroups of 256 threads:
 * a long-running kernel with the footprint of a point-to-point transfer (a few wave slots, next to no HBM bandwidth), for
 * rehearsing on one GPU how much of an exchange of a given duration a schedule hides (tools/band_time.py wire variants). */
int phl_debug_slow_copy(const float *src_dev, float *dst_dev, int64_t n_floats, int workgroups, int repeat, phl_stream stream);
/* Test hook: side streams the calling thread holds for the reference-table build (one per device the thread has
 * built such a lattice on; building on devices A, B, A, B ... must not create more than two). */
int phl_debug_side_streams(void);
/* Test hook: device blocks the block cache has handed out and not yet got back, over all lattices, workspaces and builds
 * in flight in the process.  Building, using and destroying lattices leaves it where it was; so does a build that fails. */
int64_t phl_debug_live_blocks(void);

#ifdef __cplusplus
}
#endif
#endif /* PHL_H */
