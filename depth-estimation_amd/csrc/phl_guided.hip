// phl_guided.hip -- the box-window guided filter (crf/guided.py: GuidedFilter, FastGuidedFilter, BatchedGuidedAdjacency,
// GuidedAdjacency), forward and backward, NCHW fp32.
//
// S_r(t) = sum of t over the (2r+1)^2 window clipped to the image, N = S_r(1), mean(t) = S_r(t) / N.  At the solving
// resolution h x w (the nearest-sampled H x W image; h = H, w = W for the plain filter), per guide channel c and label l:
//   mx_c = mean(x_c)   var_c = mean(x_c^2) - mx_c^2   my_l = mean(y_l)   cov_lc = mean(y_l x_c) - my_l mx_c
//   A_lc = cov_lc / (var_c + eps_c)       b_l = my_l - sum_c A_lc mx_c
//   out_l = (sum_c mean(A_lc)[lo(p)] x_c[p] + mean(b_l)[lo(p)]) * scale - src_l[p]      at every full-resolution pixel p
// The nearest index maps (low -> full for sampling, full -> low for the upsampling) come from the caller.
//
// The forward is three kernels (the backward follows further down), all built on one tile routine (tile_fill + tile_sums): a workgroup of 256 owns a 32 x 64 tile of one low-resolution
// plane, fills the tile plus a halo of r (zero outside the image) into LDS as fp32, forms the horizontal window sums of
// every halo row by a sliding fp64 sum (work item = row x column segment, lanes across rows, odd row strides: no bank
// conflict) into an fp64 LDS plane, then the vertical window sums by a second sliding fp64 sum (lane = column, wave =
// 8 rows), which leaves the 8 window sums of a thread's pixels in registers.  No image-long prefix sums, no atomics:
// a window sum is exact to fp64 rounding whatever the image size, and every run gives the same bits.
//   k_guide_stats   per (image, tile), channels in a loop: mx_c (fp64 plane) and 1 / (var_c + eps_c) (fp32 plane)
//   k_guide_coef    per (image x label, tile): the sums of y and y x_c -> A_lc (rounded to fp32 once; b_l uses the
//                   rounded value, so the model stays consistent) and b_l, as cx + 1 low-resolution fp32 planes
//   k_guide_apply   per (image x label, tile): window means of the cx + 1 planes into LDS, four planes at a time, then
//                   the full-resolution pixels that map into the tile: fp64 sum over the channels, * scale - src, one
//                   rounding into out (with more than four planes the partial sum passes through out between groups)
// (phl_guided_filter_full, the model over the whole covariance matrix of the guide channels: k_guide_stats_full and
// k_guide_coef_full in the places of the first two, in the section after k_guide_apply; its backward's kernels after the
// diagonal backward's.  phl_guided_filter_bilinear, FastGuidedFilter(mode='bilinear'): the first two kernels of either
// model with a four-tap tile fill (BL), then k_guide_mean and k_guide_up in the place of k_guide_apply; its backwards are
// the BL forms of the two nearest ones.)
// The kernels come first, model by model; the host side is the last section of the file: one argument record (Args), one
// trait for the two models (Model<CX>, CX = 0 the diagonal one), forward<ST, CX, BL> and backward<ST, CX, BL> for every
// variant, one dispatch over (tiled, CX, BL), and one checked front (checked()) that every entry point calls.
// Above the radius whose halo tiles fit LDS (phl_guided_filter_max_r) the same kernels run a streamed form of the tile
// routine (tile_sums_stream): strips of image rows, horizontal sums straight from memory, LDS independent of r.  The
// kernels of both directions reach the two forms through one front end (plane_sums, square_sums, product_sums).
// The coefficient planes are a stream-ordered temporary; labels are processed in chunks whose planes stay within
// kChunkBytes, so that k_guide_apply finds them in the Infinity Cache.
#include <math.h>

#include <utility>

#include "phl_internal.h"

namespace {

constexpr int TH = 32, TW = 64;     // tile of low-resolution pixels per workgroup
constexpr int NT = 256;             // threads: lane = tile column, wave = 8 tile rows
constexpr int RPT = TH / 4;         // rows per thread
constexpr int HSP = TW + 1;         // row stride of the fp64 plane: 16 consecutive rows hit 16 different bank pairs
constexpr int NCO = 3;              // halo columns per lane: a halo row is at most 64 * NCO words
constexpr int FU = 8;               // halo rows per wave whose loads tile_fill issues together
constexpr int FUB = 2;              // ... of its bilinear form, four taps an element
constexpr int SR = 64;               // rows per strip of the streamed form
constexpr int GRP = 4;              // coefficient planes per pass of k_guide_apply
constexpr size_t kMaxLds = 160 << 10;
constexpr size_t kChunkBytes = (size_t)96 << 20;
constexpr int kGradParts = 3;        // fp64 planes per (label, channel) that the backward sums over labels (NPART below)

__host__ __device__ inline int halo_rows(int r) { return TH + 2 * r; }
__host__ __device__ inline int halo_stride(int r) { return (TW + 2 * r) | 1; }   // odd: lanes across rows, distinct banks
// LDS of a workgroup: the fp64 plane, `ntiles` fp32 halo tiles, and k_guide_apply's window means
inline size_t tile_lds(int r, int ntiles, bool apply)
{
    return (size_t)halo_rows(r) * HSP * sizeof(double) + (size_t)ntiles * halo_rows(r) * halo_stride(r) * sizeof(float) +
           (apply ? (size_t)GRP * TH * TW * sizeof(float) : 0) + (size_t)halo_rows(r) * sizeof(int);
}
inline size_t max_lds(int r) { return max(tile_lds(r, 2, false), tile_lds(r, 1, true)); }
// ... of the streamed form (any radius): a strip of the fp64 plane, and k_guide_apply's window means
inline size_t stream_lds(bool apply) { return (size_t)SR * HSP * sizeof(double) + (apply ? (size_t)GRP * TH * TW * sizeof(float) : 0); }
enum { KIND_STATS = 0, KIND_COEF = 1, KIND_APPLY = 2 };

// samples in the window of pixel i along an axis of length n
__device__ __forceinline__ int win_count(int i, int r, int n) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// torch's bilinear tap (align_corners=False) of output index o along an axis that maps n_in samples to n_out, sc =
// (double)n_in / n_out: the two source indices and the weight of the second, all in fp64 as the float64 torch form.
// (The intrinsics keep the compiler from contracting the product and the subtraction into one rounding.)
__device__ __forceinline__ void bil_tap(int o, double sc, int n_in, int &i0, int &i1, double &lam)
{
    const double src = fmax(__dsub_rn(__dmul_rn((double)o + 0.5, sc), 0.5), 0.0);
    i0 = min((int)src, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    lam = fmin(fmax(src - (double)i0, 0.0), 1.0);
}
// the bilinear sample from its four taps, in fp64
__device__ __forceinline__ double bil_mix(float v00, float v01, float v10, float v11, double ly, double lx)
{
    const double a = (1.0 - lx) * (double)v00 + lx * (double)v01, b = (1.0 - lx) * (double)v10 + lx * (double)v11;
    return (1.0 - ly) * a + ly * b;
}

struct Tile {
    double *hs;     // [TH + 2r][HSP] horizontal window sums
    float *in;      // [TH + 2r][halo_stride] the tile and its halo
    float *in2;     // a second one (k_guide_coef: the guide channel beside y); k_guide_apply keeps its means here
    int *rowoff;    // [TH + 2r] offset of every halo row in a source plane, -1 outside the image
    int co[NCO];    // this lane's halo columns lane, lane + 64, ...: offset in a source row, -1 outside the image
    int r, ti, tj, h, w;
    const int *rmap, *cmap;     // low-resolution row / column -> row / column of a source plane (null: the identity)
    int ph, pw;                 // source planes are ph x pw
    // the bilinear sampler (BL: the low-resolution image is F.interpolate(plane, (h, w), mode='bilinear'), no maps): the
    // axis scales ph / h and pw / w and, beside co, the second tap of this lane's halo columns and its weight
    double sy, sx;
    int co1[NCO];
    double clam[NCO];
    // element (i, j) of the low-resolution image in a source plane, straight from memory (the streamed form)
    template <bool BL = false>
    __device__ __forceinline__ float ld(const float *__restrict__ plane, int i, int j) const
    {
        if constexpr (BL) {
            int i0, i1, j0, j1;
            double ly, lx;
            bil_tap(i, sy, ph, i0, i1, ly);
            bil_tap(j, sx, pw, j0, j1, lx);
            const float *p0 = plane + (int64_t)i0 * pw, *p1 = plane + (int64_t)i1 * pw;
            return (float)bil_mix(p0[j0], p0[j1], p1[j0], p1[j1], ly, lx);          // D(.) is held in fp32, as the tile holds it
        } else {
            const int I = rmap ? min(max(rmap[i], 0), ph - 1) : i, J = cmap ? min(max(cmap[j], 0), pw - 1) : j;
            return plane[(int64_t)I * pw + J];
        }
    }
    // this thread's pixels are (i0() + k, j()), k < RPT; count(k) is N of pixel k (an axis outside the image counts 1)
    __device__ __forceinline__ int i0() const { return ti + (threadIdx.x >> 6) * RPT; }
    __device__ __forceinline__ int j() const { return tj + (threadIdx.x & 63); }
    __device__ __forceinline__ double count(int k) const
    {
        return (double)(i0() + k < h ? win_count(i0() + k, r, h) : 1) * (double)(j() < w ? win_count(j(), r, w) : 1);
    }
};

// in[ih][jh] = plane[rowoff[ih] + co] at the low-resolution pixel (ti - r + ih, tj - r + jh), 0 outside the image; the
// row's padding word is filled as well.  The loads of FU rows are issued before the first store: a fill costs a few
// memory latencies, not one per row.  BL: every element is the bilinear sample of four taps (the row taps from bil_tap,
// the column taps from the tile), rounded to fp32 once; FUB rows together keep as many loads in flight as FU do.
template <bool BL = false>
__device__ __forceinline__ void tile_fill(const Tile &t, float *__restrict__ in, const float *__restrict__ plane)
{
    const int HH = halo_rows(t.r), st = halo_stride(t.r);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (BL) {
        for (int ih0 = wave; ih0 < HH; ih0 += 4 * FUB) {
            float v[FUB][NCO];
#pragma unroll
            for (int u = 0; u < FUB; u++) {
                const int ih = ih0 + 4 * u, i = t.ti - t.r + ih;
                const bool row = ih < HH && i >= 0 && i < t.h;
                int i0, i1;
                double ly;
                bil_tap(row ? i : 0, t.sy, t.ph, i0, i1, ly);
                const float *p0 = plane + (int64_t)i0 * t.pw, *p1 = plane + (int64_t)i1 * t.pw;
#pragma unroll
                for (int m = 0; m < NCO; m++)
                    v[u][m] = row && t.co[m] >= 0 ? (float)bil_mix(p0[t.co[m]], p0[t.co1[m]], p1[t.co[m]], p1[t.co1[m]], ly, t.clam[m]) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < FUB; u++) {
                const int ih = ih0 + 4 * u;
#pragma unroll
                for (int m = 0; m < NCO; m++)
                    if (ih < HH && lane + 64 * m < st) in[ih * st + lane + 64 * m] = v[u][m];
            }
        }
        return;
    }
    for (int ih0 = wave; ih0 < HH; ih0 += 4 * FU) {
        float v[FU][NCO];
#pragma unroll
        for (int u = 0; u < FU; u++) {
            const int ih = ih0 + 4 * u;
            const int ro = ih < HH ? t.rowoff[ih] : -1;
#pragma unroll
            for (int m = 0; m < NCO; m++) v[u][m] = ro >= 0 && t.co[m] >= 0 ? plane[(int64_t)ro + t.co[m]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < FU; u++) {
            const int ih = ih0 + 4 * u;
#pragma unroll
            for (int m = 0; m < NCO; m++)
                if (ih < HH && lane + 64 * m < st) in[ih * st + lane + 64 * m] = v[u][m];
        }
    }
}

// window sums of val(e), e the element's index in a filled tile: res[k] = S_r at pixel (ti + wave * RPT + k, tj + lane).
// val runs in fp64, so a product of two fp32 tiles enters the sums exactly.  Two barriers inside; the caller's next
// tile_fill may follow at once (nobody reads a tile after the second barrier).
template <typename V>
__device__ __forceinline__ void tile_sums(const Tile &t, double (&res)[RPT], V val)
{
    const int r = t.r, HH = halo_rows(r), st = halo_stride(r);
    __syncthreads();
    const int nseg = HH >= NT ? 1 : min(TW, NT / HH);
    const int seglen = (TW + nseg - 1) / nseg;
    for (int it = threadIdx.x; it < HH * nseg; it += NT) {
        const int ih = it % HH, j0 = (it / HH) * seglen, j1 = min(TW, j0 + seglen);
        const int row = ih * st;
        double *o = t.hs + ih * HSP;
        double s = 0.0;
        int jh = j0, j = j0;
        for (; jh + 3 <= j0 + 2 * r; jh += 4) {          // four loads in flight, not one
            const double a0 = val(row + jh), a1 = val(row + jh + 1), a2 = val(row + jh + 2), a3 = val(row + jh + 3);
            s += (a0 + a1) + (a2 + a3);
        }
        for (; jh <= j0 + 2 * r; jh++) s += val(row + jh);
        for (; j + 4 <= j1; j += 4) {                    // (the last step of a row reads its padding word at most)
            const int e = row + j + 2 * r + 1;
            const double d0 = val(e) - val(row + j), d1 = val(e + 1) - val(row + j + 1), d2 = val(e + 2) - val(row + j + 2),
                         d3 = val(e + 3) - val(row + j + 3);
            const double s1 = s + d0, s2 = s1 + d1, s3 = s2 + d2;
            o[j] = s, o[j + 1] = s1, o[j + 2] = s2, o[j + 3] = s3;
            s = s3 + d3;
        }
        for (; j < j1; j++) {
            o[j] = s;
            if (j + 1 < j1) s += val(row + j + 2 * r + 1) - val(row + j);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, i0 = (threadIdx.x >> 6) * RPT;
    const double *col = t.hs + lane;
    double s = 0.0;
    int ih = i0;
    for (; ih + 3 <= i0 + 2 * r; ih += 4) s += (col[ih * HSP] + col[(ih + 1) * HSP]) + (col[(ih + 2) * HSP] + col[(ih + 3) * HSP]);
    for (; ih <= i0 + 2 * r; ih++) s += col[ih * HSP];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        res[k] = s;
        if (k + 1 < RPT) s += col[(i0 + k + 2 * r + 1) * HSP] - col[(i0 + k) * HSP];
    }
}

// The same sums for any radius, with LDS that does not grow with it: g(i, j) reads element (i, j) of the low-resolution
// image from memory.  The image rows that the tile's windows reach are taken in strips of SR; per strip every row's
// horizontal window sums (clipped to the image) go into the fp64 plane, and every thread adds the part of its pixels'
// vertical windows that lies in the strip, again as a sliding sum.  Slower than the tiled form (no staging, one memory
// latency per step of a chain); taken only where the tiled form's LDS would not fit.
template <typename G>
__device__ __forceinline__ void tile_sums_stream(const Tile &t, double (&res)[RPT], G g)
{
    constexpr int SEG = TW / (NT / SR);
    const int r = t.r, lane = threadIdx.x & 63, i0 = t.ti + (threadIdx.x >> 6) * RPT;
    const int lo = max(0, t.ti - r), hi = min(t.h, t.ti + TH + r);
#pragma unroll
    for (int k = 0; k < RPT; k++) res[k] = 0.0;
    for (int a = lo; a < hi; a += SR) {
        const int b = min(hi, a + SR);
        __syncthreads();
        const int i = a + (int)(threadIdx.x % SR), j0 = (int)(threadIdx.x / SR) * SEG;
        if (i < b) {
            int jl = t.tj + j0 - r, jr = t.tj + j0 + r;
            double s = 0.0;
            for (int jj = max(0, jl); jj <= min(t.w - 1, jr); jj++) s += g(i, jj);
            double *o = t.hs + (i - a) * HSP + j0;
            for (int j = 0; j < SEG; j++) {
                o[j] = s;
                ++jr;
                if (jr >= 0 && jr < t.w) s += g(i, jr);
                if (jl >= 0 && jl < t.w) s -= g(i, jl);
                ++jl;
            }
        }
        __syncthreads();
        const double *col = t.hs + lane;
        double s = 0.0;
        for (int ii = max(a, i0 - r); ii < min(b, i0 + r + 1); ii++) s += col[(ii - a) * HSP];
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            res[k] += s;
            const int e = i0 + k + r + 1, l = i0 + k - r;
            if (e >= a && e < b) s += col[(e - a) * HSP];
            if (l >= a && l < b) s -= col[(l - a) * HSP];
        }
    }
}

// The workgroup's tile over dynamic LDS (ST: the streamed form, which keeps no halo tile).  Source planes are ph x pw;
// low-resolution row i / column j is their row rmap[i] / column cmap[j] (null maps: the identity).  Ends with a barrier
// (rowoff is read by every wave).
template <bool ST, bool BL = false>
__device__ __forceinline__ Tile make_tile(int r, int h, int w, const int *__restrict__ rmap, const int *__restrict__ cmap, int ph,
                                          int pw, int kind)
{
    extern __shared__ double lds_d[];
    Tile t;
    t.hs = lds_d;
    t.r = r, t.h = h, t.w = w;
    t.ti = blockIdx.y * TH, t.tj = blockIdx.x * TW;
    t.rmap = rmap, t.cmap = cmap, t.ph = ph, t.pw = pw;
    if constexpr (BL) t.sy = (double)ph / (double)h, t.sx = (double)pw / (double)w;
    if (ST) {
        t.in = nullptr;
        t.in2 = reinterpret_cast<float *>(lds_d + (size_t)SR * HSP);
        t.rowoff = nullptr;
        return t;
    }
    const int HH = halo_rows(r), st = halo_stride(r);
    t.in = reinterpret_cast<float *>(lds_d + (size_t)HH * HSP);
    t.in2 = t.in + (size_t)HH * st;
    t.rowoff = reinterpret_cast<int *>(t.in2 + (kind == KIND_APPLY ? (size_t)GRP * TH * TW : kind == KIND_COEF ? (size_t)HH * st : 0));
    for (int ih = threadIdx.x; ih < HH; ih += NT) {
        const int i = t.ti - r + ih;
        t.rowoff[ih] = i >= 0 && i < h ? clampi(rmap ? rmap[i] : i, 0, ph - 1) * pw : -1;
    }
#pragma unroll
    for (int m = 0; m < NCO; m++) {
        const int jh = (threadIdx.x & 63) + 64 * m, j = t.tj - r + jh;
        if constexpr (BL) {
            bil_tap(clampi(j, 0, w - 1), t.sx, pw, t.co[m], t.co1[m], t.clam[m]);
            if (!(jh < st && j >= 0 && j < w)) t.co[m] = -1;
        } else {
            t.co[m] = jh < st && j >= 0 && j < w ? clampi(cmap ? cmap[j] : j, 0, pw - 1) : -1;
        }
    }
    __syncthreads();
    return t;
}

// ---- the window-sum front end --------------------------------------------------------------------------------------
// What the kernels below call, in the form they are built for (ST: streamed, through the tile's maps; else tiled, staged
// through LDS).  Window sums of a plane, which the tiled form leaves in the halo tile `in` ...
template <bool ST, bool BL = false>
__device__ __forceinline__ void plane_sums(const Tile &t, float *__restrict__ in, const float *__restrict__ pl, double (&s)[RPT])
{
    if constexpr (ST) {
        tile_sums_stream(t, s, [&](int i, int jj) { return (double)t.template ld<BL>(pl, i, jj); });
    } else {
        tile_fill<BL>(t, in, pl);
        tile_sums(t, s, [&](int e) { return (double)in[e]; });
    }
}
// ... of the square of the plane pl that a plane_sums call has left in t.in ...
template <bool ST, bool BL = false>
__device__ __forceinline__ void square_sums(const Tile &t, const float *__restrict__ pl, double (&s)[RPT])
{
    if constexpr (ST) {
        tile_sums_stream(t, s, [&](int i, int jj) { const double v = t.template ld<BL>(pl, i, jj); return v * v; });
    } else {
        tile_sums(t, s, [&](int e) { const double v = t.in[e]; return v * v; });
    }
}
// ... and of its product with a second plane, which goes into t.in2 (exact in fp64: 24 + 24 bits)
template <bool ST, bool BL = false>
__device__ __forceinline__ void product_sums(const Tile &t, const float *__restrict__ pl, const float *__restrict__ pl2,
                                             double (&s)[RPT])
{
    if constexpr (ST) {
        tile_sums_stream(t, s, [&](int i, int jj) { return (double)t.template ld<BL>(pl, i, jj) * (double)t.template ld<BL>(pl2, i, jj); });
    } else {
        tile_fill<BL>(t, t.in2, pl2);
        tile_sums(t, s, [&](int e) { return (double)t.in[e] * (double)t.in2[e]; });
    }
}
// rn[k] = 1 / N of the thread's pixels
__device__ __forceinline__ void recip_counts(const Tile &t, double (&rn)[RPT])
{
#pragma unroll
    for (int k = 0; k < RPT; k++) rn[k] = 1.0 / t.count(k);
}
// f(k, offset in an h x w plane) for those of the thread's pixels that lie in the image.  (No unroll pragma: it would
// unroll the loop here, before the kernel's loop over channels sees it, and the eight offsets then stay live across the
// window sums -- up to 46 more VGPRs.  The constant trip count is unrolled in the kernel all the same.)
template <typename F>
__device__ __forceinline__ void for_pixels(const Tile &t, F f)
{
    const int i0 = t.i0(), j = t.j();
    for (int k = 0; k < RPT; k++) {
        const int i = i0 + k;
        if (i < t.h && j < t.w) f(k, (int64_t)i * t.w + j);
    }
}

// ---- guide statistics ----------------------------------------------------------------------------------------------
// (BL, here and in the three kernels that follow: the low-resolution image is the bilinear sample of the H x W planes,
// taken while the tile is filled; the maps are null)
template <bool ST, bool BL = false>
__global__ __launch_bounds__(NT) void k_guide_stats(const float *__restrict__ x, const int *__restrict__ rmap,
                                                   const int *__restrict__ cmap, const float *__restrict__ eps,
                                                   double *__restrict__ mx, float *__restrict__ inv, int cx, int H, int W, int h,
                                                   int w, int r)
{
    Tile t = make_tile<ST, BL>(r, h, w, rmap, cmap, H, W, KIND_STATS);
    const int b = blockIdx.z;
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w;
    for (int c = 0; c < cx; c++) {
        const float *xp = x + ((int64_t)b * cx + c) * HWf;
        double s1[RPT], s2[RPT];
        plane_sums<ST, BL>(t, t.in, xp, s1);
        square_sums<ST, BL>(t, xp, s2);
        const double e = (double)eps[c];
        for_pixels(t, [&](int k, int64_t q) {
            const double n = t.count(k);
            const double m = s1[k] / n, var = s2[k] / n - m * m;
            const int64_t o = ((int64_t)b * cx + c) * hw + q;
            mx[o] = m;
            inv[o] = (float)(1.0 / (var + e));
        });
    }
}

// ---- coefficients --------------------------------------------------------------------------------------------------
template <bool ST, bool BL = false>
__global__ __launch_bounds__(NT) void k_guide_coef(const float *__restrict__ y, const float *__restrict__ x,
                                                  const int *__restrict__ rmap, const int *__restrict__ cmap,
                                                  const double *__restrict__ mx, const float *__restrict__ inv,
                                                  float *__restrict__ coef, int n0, int cy, int cx, int H, int W, int h, int w, int r)
{
    Tile t = make_tile<ST, BL>(r, h, w, rmap, cmap, H, W, KIND_COEF);
    const int n = n0 + blockIdx.z, b = n / cy;                     // n = image * cy + label
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w;
    const float *yp = y + (int64_t)n * HWf;
    float *cp = coef + (int64_t)blockIdx.z * (cx + 1) * hw;

    double my[RPT], bacc[RPT], rn[RPT], s[RPT];
    recip_counts(t, rn);
    plane_sums<ST, BL>(t, t.in, yp, s);                             // (tiled form: y stays in LDS for the products below)
#pragma unroll
    for (int k = 0; k < RPT; k++) bacc[k] = my[k] = s[k] * rn[k];
    for (int c = 0; c < cx; c++) {
        product_sums<ST, BL>(t, yp, x + ((int64_t)b * cx + c) * HWf, s);
        for_pixels(t, [&](int k, int64_t o) {
            const int64_t g = ((int64_t)b * cx + c) * hw + o;
            const double m = mx[g];
            const float a = (float)((s[k] * rn[k] - my[k] * m) * (double)inv[g]);
            cp[(int64_t)c * hw + o] = a;
            bacc[k] -= (double)a * m;
        });
    }
    for_pixels(t, [&](int k, int64_t o) { cp[(int64_t)cx * hw + o] = (float)bacc[k]; });
}

// ---- apply ---------------------------------------------------------------------------------------------------------
// first index I in [0, n) with map[I] >= v (map is non-decreasing)
__device__ __forceinline__ int lower_bound(const int *__restrict__ map, int n, int v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (map[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool ST>
__global__ __launch_bounds__(NT) void k_guide_apply(const float *__restrict__ coef, const float *__restrict__ x,
                                                   const float *__restrict__ src, float *__restrict__ out,
                                                   const int *__restrict__ rlow, const int *__restrict__ clow, int n0, int cy, int cx,
                                                   int H, int W, int h, int w, int r, float scale)
{
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_APPLY);
    float *M = t.in2;                                               // [GRP][TH][TW] window means (both forms)
    const int n = n0 + blockIdx.z, b = n / cy;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w;
    const float *cp = coef + (int64_t)blockIdx.z * (cx + 1) * hw;
    double rn[RPT];
    recip_counts(t, rn);
    // the full-resolution rows and columns whose low-resolution pixel lies in this tile
    const int I0 = lower_bound(rlow, H, t.ti), I1 = lower_bound(rlow, H, t.ti + TH);
    const int J0 = lower_bound(clow, W, t.tj), J1 = lower_bound(clow, W, t.tj + TW);
    const float *xb = x + (int64_t)b * cx * HWf;
    const float *sp = src ? src + (int64_t)n * HWf : nullptr;
    float *op = out + (int64_t)n * HWf;
    const int np = cx + 1;

    for (int q0 = 0; q0 < np; q0 += GRP) {
        const int nq = min(GRP, np - q0);
        for (int q = 0; q < nq; q++) {
            double s[RPT];
            plane_sums<ST>(t, t.in, cp + (int64_t)(q0 + q) * hw, s);
#pragma unroll
            for (int k = 0; k < RPT; k++) M[(q * TH + wave * RPT + k) * TW + lane] = (float)(s[k] * rn[k]);
        }
        __syncthreads();
        const bool first = q0 == 0, last = q0 + GRP >= np;
        for (int I = I0 + wave; I < I1; I += 4) {
            const int li = clampi(rlow[I] - t.ti, 0, TH - 1);
            for (int J = J0 + lane; J < J1; J += 64) {
                const int lj = clampi(clow[J] - t.tj, 0, TW - 1);
                const int64_t o = (int64_t)I * W + J;
                double acc = first ? 0.0 : (double)op[o];
                for (int q = 0; q < nq; q++) {
                    const double m = M[(q * TH + li) * TW + lj];
                    acc += q0 + q < cx ? m * (double)xb[(int64_t)(q0 + q) * HWf + o] : m;
                }
                if (last) {
                    acc *= (double)scale;
                    if (sp) acc -= (double)sp[o];
                }
                op[o] = (float)acc;
            }
        }
        // (the next group's first write to M comes after the two barriers of its tile_sums)
    }
}

constexpr int npairs(int cx) { return cx * (cx + 1) / 2; }     // elements of the upper triangle of a cx x cx matrix

// ---- full covariance: the forward ------------------------------------------------------------------------------------
// The model the reference kept as commented lines (crf/gaussian_matrix.py:204-212): the guide channels are solved for
// together, through their whole covariance matrix instead of its diagonal.  At the solving resolution:
//   S_cd = mean(x_c x_d) - mx_c mx_d      P = (S + diag(eps))^-1 (symmetric)      A_lc = sum_d cov_ld P_dc
// b_l and out as in the header, so k_guide_apply and the chunks are those of the diagonal model.  P belongs to the image, not to the
// label: the two kernels below take the places of k_guide_stats and k_guide_coef, the channel count a template parameter
// (1 .. PHL_GUIDED_FULL_MAX_CX), so that every matrix element is a register of a constant index.
//   k_guide_stats_full  per (image, tile): mx_c and the window sums of the cx (cx + 1) / 2 products x_c x_d (two halo
//                       tiles, as k_guide_coef) -> S + diag(eps) = L D L^T in fp64 registers, M = L^-1,
//                       P = M^T D^-1 M -> mx (fp64 planes) and the upper triangle of P (fp64 planes, row-major)
//   k_guide_coef_full   per (image x label, tile): the sums of y and y x_c as k_guide_coef, all cx covariances kept ->
//                       A_lc through P in fp64, rounded to fp32 once; b_l from the rounded values
// No pivot search and no loop whose trip count depends on the data: a non-positive pivot (eps <= 0 on a flat window)
// gives inf or nan, as 1 / (var + eps) does in k_guide_stats.
// plane of P_cd, c <= d, among the npairs(cx) of an image
__host__ __device__ constexpr int pair_plane(int c, int d, int cx) { return c * cx - c * (c - 1) / 2 + (d - c); }

// f(std::integral_constant<int, I>) for I = 0 .. N - 1: a loop whose index is a constant in every body
template <typename F, int... I>
__device__ __forceinline__ void static_for_seq(F f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F f) { static_for_seq(f, std::make_integer_sequence<int, N>{}); }

template <bool ST, int CX, bool BL = false>
__global__ __launch_bounds__(NT) void k_guide_stats_full(const float *__restrict__ x, const int *__restrict__ rmap,
                                                        const int *__restrict__ cmap, const float *__restrict__ eps,
                                                        double *__restrict__ mx, double *__restrict__ P, int H, int W, int h, int w,
                                                        int r)
{
    constexpr int NP = npairs(CX);
    Tile t = make_tile<ST, BL>(r, h, w, rmap, cmap, H, W, KIND_COEF);
    const int b = blockIdx.z;
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w;
    const float *xb = x + (int64_t)b * CX * HWf;
    double m[CX][RPT], S[NP][RPT], rn[RPT], s[RPT];
    recip_counts(t, rn);
    // (static_for, not a loop with an unroll pragma: around bodies of this size the pragma is not always honoured, and a
    // channel that is not a constant puts S into scratch)
    static_for<CX>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        plane_sums<ST, BL>(t, t.in, xb + c * HWf, s);
#pragma unroll
        for (int k = 0; k < RPT; k++) m[c][k] = s[k] * rn[k];
        square_sums<ST, BL>(t, xb + c * HWf, s);
#pragma unroll
        for (int k = 0; k < RPT; k++) S[pair_plane(c, c, CX)][k] = s[k] * rn[k];          // mean(x_c x_d) for now
        static_for<CX>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            if constexpr (d > c) {
                product_sums<ST, BL>(t, xb + c * HWf, xb + d * HWf, s);
#pragma unroll
                for (int k = 0; k < RPT; k++) S[pair_plane(c, d, CX)][k] = s[k] * rn[k];
            }
        });
    });
    double e[CX];
#pragma unroll
    for (int c = 0; c < CX; c++) e[c] = (double)eps[c];
    double *mp = mx + (int64_t)b * CX * hw, *pp = P + (int64_t)b * NP * hw;
    for_pixels(t, [&](int k, int64_t q) {
        // a[d][c], c <= d: the lower triangle of S + diag(eps), then L below the diagonal; D and 1 / D beside it
        double a[CX][CX], M[CX][CX], D[CX], rD[CX];
#pragma unroll
        for (int d = 0; d < CX; d++)
#pragma unroll
            for (int c = 0; c <= d; c++) a[d][c] = S[pair_plane(c, d, CX)][k] - m[c][k] * m[d][k] + (c == d ? e[c] : 0.0);
#pragma unroll
        for (int j = 0; j < CX; j++) {
            double dj = a[j][j];
#pragma unroll
            for (int p = 0; p < j; p++) dj -= a[j][p] * a[j][p] * D[p];
            D[j] = dj, rD[j] = 1.0 / dj;
#pragma unroll
            for (int i = j + 1; i < CX; i++) {
                double v = a[i][j];
#pragma unroll
                for (int p = 0; p < j; p++) v -= a[i][p] * a[j][p] * D[p];
                a[i][j] = v * rD[j];
            }
        }
        // M = L^-1, unit lower triangular
#pragma unroll
        for (int j = 0; j < CX; j++) {
            M[j][j] = 1.0;
#pragma unroll
            for (int i = j + 1; i < CX; i++) {
                double v = 0.0;
#pragma unroll
                for (int p = j; p < i; p++) v -= a[i][p] * M[p][j];
                M[i][j] = v;
            }
        }
#pragma unroll
        for (int c = 0; c < CX; c++) {
            mp[c * hw + q] = m[c][k];
#pragma unroll
            for (int d = c; d < CX; d++) {
                double v = 0.0;
#pragma unroll
                for (int p = d; p < CX; p++) v += M[p][c] * M[p][d] * rD[p];
                pp[pair_plane(c, d, CX) * hw + q] = v;
            }
        }
    });
}

template <bool ST, int CX, bool BL = false>
__global__ __launch_bounds__(NT) void k_guide_coef_full(const float *__restrict__ y, const float *__restrict__ x,
                                                       const int *__restrict__ rmap, const int *__restrict__ cmap,
                                                       const double *__restrict__ mx, const double *__restrict__ P,
                                                       float *__restrict__ coef, int n0, int cy, int H, int W, int h, int w, int r)
{
    constexpr int NP = npairs(CX);
    Tile t = make_tile<ST, BL>(r, h, w, rmap, cmap, H, W, KIND_COEF);
    const int n = n0 + blockIdx.z, b = n / cy;                     // n = image * cy + label
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w;
    const float *yp = y + (int64_t)n * HWf, *xb = x + (int64_t)b * CX * HWf;
    const double *mp = mx + (int64_t)b * CX * hw, *pp = P + (int64_t)b * NP * hw;
    float *cp = coef + (int64_t)blockIdx.z * (CX + 1) * hw;

    double my[RPT], rn[RPT], s[RPT], cov[CX][RPT];
    recip_counts(t, rn);
    plane_sums<ST, BL>(t, t.in, yp, s);                             // (tiled form: y stays in LDS for the products below)
#pragma unroll
    for (int k = 0; k < RPT; k++) my[k] = s[k] * rn[k];
    static_for<CX>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        product_sums<ST, BL>(t, yp, xb + c * HWf, s);
#pragma unroll
        for (int k = 0; k < RPT; k++) cov[c][k] = s[k] * rn[k];       // mean(y x_c) for now
    });
    for_pixels(t, [&](int k, int64_t o) {
        double m[CX], cv[CX], p[NP], bacc = my[k];
#pragma unroll
        for (int c = 0; c < CX; c++) m[c] = mp[c * hw + o], cv[c] = cov[c][k] - my[k] * m[c];
#pragma unroll
        for (int i = 0; i < NP; i++) p[i] = pp[i * hw + o];
#pragma unroll
        for (int c = 0; c < CX; c++) {
            double v = 0.0;
#pragma unroll
            for (int d = 0; d < CX; d++) v += cv[d] * p[pair_plane(min(c, d), max(c, d), CX)];
            const float a = (float)v;
            cp[c * hw + o] = a;
            bacc -= (double)a * m[c];
        }
        cp[CX * hw + o] = (float)bacc;
    });
}

// ---- bilinear: FastGuidedFilter(mode='bilinear'), forward ----------------------------------------------------------
// D = F.interpolate(., (h, w), mode='bilinear'), U = F.interpolate(., (H, W), mode='bilinear') (align_corners=False):
//   (mean_A, mean_b) = the model above (either one) on D(y), D(x)      out_l = (sum_c U(mean_A_lc) x_c + U(mean_b_l)) * scale - src_l
// D is taken inside the front end: the BL instances of the statistics and coefficient kernels fill their halo tiles with
// the four-tap samples (fp64 taps and weights from bil_tap, the sample rounded to fp32 once, which is what fp32 torch
// holds as well), so no low-resolution copy of y or x is written and everything after the fill is the nearest kernels'
// code.  U needs the window means of up to four low-resolution pixels, which may lie in four tiles, so the means leave
// k_guide_apply's LDS:
//   k_guide_mean    per (image x label, tile): the window means of the cx + 1 coefficient planes (plane_sums, rounded to
//                   fp32 as k_guide_apply rounds them) -> cx + 1 low-resolution planes
//   k_guide_up      per full-resolution pixel (a thread takes UR rows of one column): the four-tap samples of the mean
//                   planes and the sum over the channels in fp64, * scale - src, one rounding into out
// Labels per chunk: kChunkBytes / (2 (cx + 1) h w sizeof(float)), at least 1, at most B cy and 65535 (Plan::per_forward):
// the coefficient and the mean planes of a chunk stay in the Infinity Cache between the three kernels.
constexpr int UR = 4;               // full-resolution rows per thread of k_guide_up: a workgroup covers 16 x 64 pixels

template <bool ST>
__global__ __launch_bounds__(NT) void k_guide_mean(const float *__restrict__ coef, float *__restrict__ mean, int np, int h, int w,
                                                  int r)
{
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_STATS);
    const int64_t hw = (int64_t)h * w;
    const float *cp = coef + (int64_t)blockIdx.z * np * hw;
    float *mp = mean + (int64_t)blockIdx.z * np * hw;
    double rn[RPT];
    recip_counts(t, rn);
    for (int q = 0; q < np; q++) {
        double s[RPT];
        plane_sums<ST>(t, t.in, cp + (int64_t)q * hw, s);
        for_pixels(t, [&](int k, int64_t o) { mp[(int64_t)q * hw + o] = (float)(s[k] * rn[k]); });
    }
}

__global__ __launch_bounds__(NT) void k_guide_up(const float *__restrict__ mean, const float *__restrict__ x,
                                                const float *__restrict__ src, float *__restrict__ out, int n0, int cy, int cx,
                                                int H, int W, int h, int w, int tilesx, float scale)
{
    const int bx = blockIdx.x % tilesx, by = blockIdx.x / tilesx;
    const int J = bx * 64 + (threadIdx.x & 63), I0 = (by * 4 + (threadIdx.x >> 6)) * UR;
    if (J >= W) return;
    const int n = n0 + blockIdx.z, b = n / cy;
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w;
    const float *mp = mean + (int64_t)blockIdx.z * (cx + 1) * hw;
    const float *xb = x + (int64_t)b * cx * HWf;
    const float *sp = src ? src + (int64_t)n * HWf : nullptr;
    float *op = out + (int64_t)n * HWf;
    const double sy = (double)h / (double)H;
    int j0, j1;
    double lx;
    bil_tap(J, (double)w / (double)W, w, j0, j1, lx);
    for (int k = 0; k < UR && I0 + k < H; k++) {
        int i0, i1;
        double ly;
        bil_tap(I0 + k, sy, h, i0, i1, ly);
        const int64_t o = (int64_t)(I0 + k) * W + J, q0 = (int64_t)i0 * w, q1 = (int64_t)i1 * w;
        double acc = 0.0;
        for (int c = 0; c <= cx; c++) {
            const float *m = mp + (int64_t)c * hw;
            const double u = bil_mix(m[q0 + j0], m[q0 + j1], m[q1 + j0], m[q1 + j1], ly, lx);
            acc += c < cx ? u * (double)xb[(int64_t)c * HWf + o] : u;
        }
        acc *= (double)scale;
        if (sp) acc -= (double)sp[o];
        op[o] = (float)acc;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------
// With g the gradient of out [B][cy][H][W], N = S(1), and the forward's mx_c, my_l, inv_c = 1 / (var_c + eps_c), A_lc
// recomputed (nothing but y, x, eps and g comes in):
//   gAbar_lc[q] = scale sum_{p: lo(p) = q} g_l[p] x_c[p]      gbbar_l[q] = scale sum_{p: lo(p) = q} g_l[p]
//   gA_lc = S(gAbar_lc / N)    gb_l = S(gbbar_l / N)                        (the adjoint of mean is u -> S(u / N))
//   gA'_lc = gA_lc - gb_l mx_c   gcov_lc = gA'_lc inv_c   gvar_c = -inv_c sum_l gA'_lc A_lc   gmy_l = gb_l - sum_c gcov_lc mx_c
//   gmx_c = -sum_l gb_l A_lc - sum_l gcov_lc my_l - 2 mx_c gvar_c
//   U_l0 = S(gmy_l / N)   U_lc = S(gcov_lc / N)
//   gys_l = U_l0 + sum_c xs_c U_lc          gxs_c = sum_l ys_l U_lc + S(gmx_c / N) + 2 xs_c S(gvar_c / N)
//   grad_y = gys at the sampled pixels (0 elsewhere) - g where the subtracted source is y
//   grad_x[p] = scale sum_l g_l[p] mean(A_lc)[lo(p)] + gxs at the sampled pixels        grad_eps_c = sum gvar_c
// Kernels, per chunk of labels (planes are low-resolution, fp32 where a window sum reads them, fp64 where labels are summed):
//   k_grad_gather   the nearest samples ys / xs as planes of their own (skipped at full resolution: y and x are those
//                   planes), so that every tile below has identity maps
//   k_grad_down     gAbar / N and gbbar / N: one thread per low-resolution pixel sums its pre-image rectangle in fp64
//   k_grad_coef     per (label, tile): the forward's sums of ys and ys xs_c again -> my, A in fp64; the sums gA, gb; the
//                   pointwise step; writes gcov_lc / N and gmy_l / N, A_lc (for grad_x) and this label's terms of
//                   gvar_c / N and gmx_c / N
//   k_grad_apply    per (label, tile): U_l0, U_lc -> gys into LDS -> grad_y over the tile's full-resolution pixels;
//                   for grad_x also this label's ys_l U_lc and mean(A_lc)
//   k_grad_reduce   the per-label terms summed over the chunk's labels in index order into fp64 planes [B][cx][h][w]
//   k_grad_direct   sum_l g_l[p] mean(A_lc)[lo(p)] into an fp64 plane [B][cx][H][W], labels in index order
// (chunks follow each other in stream order), and then once:
//   k_grad_finish   gmx_c / N with its - 2 mx_c gvar_c term, and gvar_c / N, as fp32 planes for the tile routine
//   k_grad_x        per (image, tile), channels in a loop: gxs into LDS -> grad_x over the tile's full-resolution pixels
//   k_grad_eps1/2   grad_eps: a fixed-order two-stage fp64 reduction of gvar_c
// No atomics anywhere; every gradient is rounded to fp32 once.
//
// BL, the backward of phl_guided_filter_bilinear (the diagonal model): ys = D(y), xs = D(x) and out_l = scale (sum_c
// U(mean A_lc) x_c + U(mean b_l)) - src_l.  Everything between gA and gys, gxs, gvar above is the same code on the same
// low-resolution planes; the four places that connect the two resolutions take their bilinear form:
//   k_grad_gather<true>   ys / xs = the four-tap samples, bil_tap / bil_mix and the one rounding to fp32 of the forward's
//                         tile fill, so that k_guide_stats and k_grad_coef on these planes (identity maps) recompute
//                         the forward's model bit for bit
//   k_grad_down<true>     gAbar_lc = scale U^T(g_l x_c), gbbar_l = scale U^T(g_l): U's first tap is non-decreasing in the
//                         output index, so the full-resolution rows (columns) that tap a low-resolution row (column)
//                         are one range (up_lower_bound); the thread of a low-resolution pixel sums its rectangle
//                         with the weights of up_weight, rows then columns, fp64
//   scatter_tile<true>    D^T: with H >= 2h the first taps of D are at least 2 apart, so a full-resolution row is a tap
//                         of at most one low-resolution row (down_owner; columns likewise) and D^T is a gather of one
//                         low-resolution pixel with the product of the two axis weights, 0 where there is none
//   k_grad_direct<true>   scale sum_l g_l[p] U(mean A_lc)[p] with the four taps of k_guide_up
// The entry point refuses 2h > H and 2w > W, which the single owner of scatter_tile<true> rests on.
constexpr int NE = 256;             // threads of the pointwise kernels
constexpr int NEB = 128;            // first-stage workgroups per channel of the grad_eps reduction
enum { PART_VAR = 0, PART_MX = 1, PART_YU = 2, NPART = kGradParts };

// U (n low -> N full, sc = (double)n / N) along an axis: the first full index whose first tap is >= v (the first tap is
// non-decreasing in the full index), and the weight of low index i in the sample at full index I (both taps the same
// index at a clamped edge: their sum)
__device__ __forceinline__ int up_lower_bound(int N, double sc, int n, int v)
{
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int a, b;
        double l;
        bil_tap(mid, sc, n, a, b, l);
        if (a < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ double up_weight(int I, double sc, int n, int i)
{
    int a, b;
    double l;
    bil_tap(I, sc, n, a, b, l);
    return (a == i ? 1.0 - l : 0.0) + (b == i ? l : 0.0);
}
// D (N full -> n low, sc = (double)N / n >= 2) along an axis: the first tap of low index i, and the one low index whose
// sample takes full index I with its weight (-1 and 0 where I is nobody's tap).  The first taps are strictly increasing
// and at least 2 apart, so the owner is the last i whose first tap is <= I: an estimate from the inverse map, corrected
// with the taps themselves.
__device__ __forceinline__ int down_first_tap(int i, double sc, int N)
{
    int a, b;
    double l;
    bil_tap(i, sc, N, a, b, l);
    return a;
}
__device__ __forceinline__ int down_owner(int I, double sc, int N, int n, double &wgt)
{
    int i = clampi((int)floor(((double)I + 1.5) / sc - 0.5), 0, n - 1);
    while (i + 1 < n && down_first_tap(i + 1, sc, N) <= I) i++;
    while (i >= 0 && down_first_tap(i, sc, N) > I) i--;
    wgt = 0.0;
    if (i < 0) return -1;
    int a, b;
    double l;
    bil_tap(i, sc, N, a, b, l);
    wgt = (a == I ? 1.0 - l : 0.0) + (b == I ? l : 0.0);
    return i;
}

template <bool BL = false>
__global__ __launch_bounds__(NE) void k_grad_gather(const float *__restrict__ src, float *__restrict__ dst,
                                                   const int *__restrict__ rmap, const int *__restrict__ cmap, int H, int W, int h,
                                                   int w)
{
    const int64_t hw = (int64_t)h * w, q = (int64_t)blockIdx.x * NE + threadIdx.x;
    if (q >= hw) return;
    const int64_t pl = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
    const int i = (int)(q / w), j = (int)(q % w);
    if constexpr (BL) {                                              // Tile::ld<true>: the sample the forward's tiles hold
        int i0, i1, j0, j1;
        double ly, lx;
        bil_tap(i, (double)H / (double)h, H, i0, i1, ly);
        bil_tap(j, (double)W / (double)w, W, j0, j1, lx);
        const float *p0 = src + pl * H * W + (int64_t)i0 * W, *p1 = src + pl * H * W + (int64_t)i1 * W;
        dst[pl * hw + q] = (float)bil_mix(p0[j0], p0[j1], p1[j0], p1[j1], ly, lx);
    } else {
        dst[pl * hw + q] = src[pl * H * W + (int64_t)clampi(rmap[i], 0, H - 1) * W + clampi(cmap[j], 0, W - 1)];
    }
}

template <bool BL = false>
__global__ __launch_bounds__(NE) void k_grad_down(const float *__restrict__ g, const float *__restrict__ x, float *__restrict__ P,
                                                 const int *__restrict__ rlow, const int *__restrict__ clow, int n0, int cy, int cx,
                                                 int H, int W, int h, int w, int r, float scale)
{
    const int64_t hw = (int64_t)h * w, HWf = (int64_t)H * W, q = (int64_t)blockIdx.x * NE + threadIdx.x;
    if (q >= hw) return;
    const int z = blockIdx.y, n = n0 + z, b = n / cy;
    const int i = (int)(q / w), j = (int)(q % w);
    // the full-resolution rows and columns that reach the pixel: its pre-image under the nearest maps, or (BL) those
    // whose taps of U include it, first tap i - 1 or i
    const double sy = (double)h / (double)H, sx = (double)w / (double)W;
    const int I0 = BL ? up_lower_bound(H, sy, h, i - 1) : lower_bound(rlow, H, i);
    const int I1 = BL ? up_lower_bound(H, sy, h, i + 1) : lower_bound(rlow, H, i + 1);
    const int J0 = BL ? up_lower_bound(W, sx, w, j - 1) : lower_bound(clow, W, j);
    const int J1 = BL ? up_lower_bound(W, sx, w, j + 1) : lower_bound(clow, W, j + 1);
    const double k = (double)scale / ((double)win_count(i, r, h) * (double)win_count(j, r, w));
    const float *gp = g + (int64_t)n * HWf;
    for (int c = 0; c <= cx; c++) {
        const float *xp = c < cx ? x + ((int64_t)b * cx + c) * HWf : nullptr;
        double acc = 0.0;
        for (int I = I0; I < I1; I++) {
            const double wy = BL ? up_weight(I, sy, h, i) : 1.0;
            for (int J = J0; J < J1; J++) {
                const int64_t o = (int64_t)I * W + J;
                const double v = xp ? (double)gp[o] * (double)xp[o] : (double)gp[o];
                if constexpr (BL) acc += wy * up_weight(J, sx, w, j) * v; else acc += v;
            }
        }
        P[((int64_t)z * (cx + 1) + c) * hw + q] = (float)(acc * k);
    }
}

template <bool ST>
__global__ __launch_bounds__(NT) void k_grad_coef(const float *__restrict__ ys, const float *__restrict__ xs,
                                                 const float *__restrict__ P, const double *__restrict__ mx,
                                                 const float *__restrict__ inv, float *__restrict__ Q, float *__restrict__ A,
                                                 double *__restrict__ part, int n0, int cy, int cx, int h, int w, int r)
{
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_COEF);
    const int z = blockIdx.z, b = (n0 + z) / cy;
    const int64_t hw = (int64_t)h * w;
    const float *yp = ys + (int64_t)z * hw, *pp = P + (int64_t)z * (cx + 1) * hw;
    float *qp = Q + (int64_t)z * (cx + 1) * hw, *ap = A ? A + (int64_t)z * cx * hw : nullptr;
    double *tp = part ? part + (int64_t)z * NPART * cx * hw : nullptr;

    double my[RPT], gb[RPT], gmy[RPT], rn[RPT], a[RPT], s[RPT];
    recip_counts(t, rn);
    plane_sums<ST>(t, t.in, yp, s);                                 // (tiled form: ys stays in LDS for the products below)
#pragma unroll
    for (int k = 0; k < RPT; k++) my[k] = s[k] * rn[k];
    plane_sums<ST>(t, t.in2, pp + (int64_t)cx * hw, gb);
#pragma unroll
    for (int k = 0; k < RPT; k++) gmy[k] = gb[k];
    for (int c = 0; c < cx; c++) {
        product_sums<ST>(t, yp, xs + ((int64_t)b * cx + c) * hw, s);
#pragma unroll
        for (int k = 0; k < RPT; k++) a[k] = s[k] * rn[k];            // mean(y x_c) for now
        plane_sums<ST>(t, t.in2, pp + (int64_t)c * hw, s);
        for_pixels(t, [&](int k, int64_t o) {
            const int64_t gi = ((int64_t)b * cx + c) * hw + o;
            const double m = mx[gi], iv = (double)inv[gi];
            const double alc = (a[k] - my[k] * m) * iv;
            const double gap = s[k] - gb[k] * m, gcov = gap * iv;
            gmy[k] -= gcov * m;
            qp[(int64_t)c * hw + o] = (float)(gcov * rn[k]);
            if (ap) ap[(int64_t)c * hw + o] = (float)alc;
            if (tp) {
                tp[((int64_t)PART_VAR * cx + c) * hw + o] = -(iv * (gap * alc)) * rn[k];
                tp[((int64_t)PART_MX * cx + c) * hw + o] = -(gb[k] * alc + gcov * my[k]) * rn[k];
            }
        });
    }
    for_pixels(t, [&](int k, int64_t o) { qp[(int64_t)cx * hw + o] = (float)(gmy[k] * rn[k]); });
}

// f(o, value) for every full-resolution pixel of the tile's share: G[li][lj] of the tile's LDS plane at the pixel that is
// the sample (rmapS[i], cmapS[j]) of the tile's low-resolution pixel (i, j), 0 at the others.  The shares partition the
// image: the rows from the sample row of the tile's first row up to that of the next tile's (strictly increasing maps),
// columns likewise -- a sample need not lie in the pre-image of its own low-resolution pixel under the upsampling maps.
// BL: the samples are D's; the value is G at the one low-resolution pixel whose taps include the pixel (down_owner per
// axis), times the product of the two axis weights, and the shares run between the first taps of the tiles' first rows
// and columns (no maps).
template <bool BL = false, typename F>
__device__ __forceinline__ void scatter_tile(const Tile &t, const double *__restrict__ G, const int *__restrict__ rmapS,
                                             const int *__restrict__ cmapS, int H, int W, F f)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (BL) {
        const double sy = (double)H / (double)t.h, sx = (double)W / (double)t.w;
        const int I0 = t.ti == 0 ? 0 : clampi(down_first_tap(t.ti, sy, H), 0, H);
        const int I1 = t.ti + TH >= t.h ? H : clampi(down_first_tap(t.ti + TH, sy, H), 0, H);
        const int J0 = t.tj == 0 ? 0 : clampi(down_first_tap(t.tj, sx, W), 0, W);
        const int J1 = t.tj + TW >= t.w ? W : clampi(down_first_tap(t.tj + TW, sx, W), 0, W);
        for (int I = I0 + wave; I < I1; I += 4) {
            double wy;
            const int i = down_owner(I, sy, H, t.h, wy);
            const bool ri = i >= t.ti && i < t.ti + TH && i < t.h;
            for (int J = J0 + lane; J < J1; J += 64) {
                double wx;
                const int j = down_owner(J, sx, W, t.w, wx);
                const bool hit = ri && j >= t.tj && j < t.tj + TW && j < t.w;
                f((int64_t)I * W + J, hit ? wy * wx * G[(i - t.ti) * TW + (j - t.tj)] : 0.0);
            }
        }
        return;
    }
    const int I0 = t.ti == 0 ? 0 : clampi(rmapS[t.ti], 0, H), I1 = t.ti + TH >= t.h ? H : clampi(rmapS[t.ti + TH], 0, H);
    const int J0 = t.tj == 0 ? 0 : clampi(cmapS[t.tj], 0, W), J1 = t.tj + TW >= t.w ? W : clampi(cmapS[t.tj + TW], 0, W);
    for (int I = I0 + wave; I < I1; I += 4) {
        const int i = lower_bound(rmapS, t.h, I);
        const bool ri = i < t.h && i >= t.ti && i < t.ti + TH && rmapS[i] == I;
        for (int J = J0 + lane; J < J1; J += 64) {
            const int j = lower_bound(cmapS, t.w, J);
            const bool hit = ri && j < t.w && j >= t.tj && j < t.tj + TW && cmapS[j] == J;
            f((int64_t)I * W + J, hit ? G[(i - t.ti) * TW + (j - t.tj)] : 0.0);
        }
    }
}

template <bool ST, bool BL = false>
__global__ __launch_bounds__(NT) void k_grad_apply(const float *__restrict__ Q, const float *__restrict__ A,
                                                  const float *__restrict__ ys, const float *__restrict__ xs,
                                                  const float *__restrict__ g, float *__restrict__ grad_y, float *__restrict__ mA,
                                                  double *__restrict__ part, const int *__restrict__ rmapS,
                                                  const int *__restrict__ cmapS, int n0, int cy, int cx, int H, int W, int h, int w,
                                                  int r, int subtract_is_y, int pstride, int poff)
{
    // part: `pstride` planes a label, this kernel's ys_l U_lc from plane `poff` on
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_APPLY);
    double *G = reinterpret_cast<double *>(t.in2);                  // [TH][TW] gys (both forms; 8-byte aligned)
    const int z = blockIdx.z, n = n0 + z, b = n / cy;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t hw = (int64_t)h * w, HWf = (int64_t)H * W;
    const float *qp = Q + (int64_t)z * (cx + 1) * hw, *yp = ys + (int64_t)z * hw;
    double gys[RPT], s[RPT];
    plane_sums<ST>(t, t.in, qp + (int64_t)cx * hw, gys);
    for (int c = 0; c < cx; c++) {
        const float *xp = xs + ((int64_t)b * cx + c) * hw;
        plane_sums<ST>(t, t.in, qp + (int64_t)c * hw, s);
        for_pixels(t, [&](int k, int64_t o) {
            gys[k] += (double)xp[o] * s[k];
            if (part) part[((int64_t)z * pstride + poff + c) * hw + o] = (double)yp[o] * s[k];
        });
        if (mA) {
            plane_sums<ST>(t, t.in, A + ((int64_t)z * cx + c) * hw, s);
            for_pixels(t, [&](int k, int64_t o) { mA[((int64_t)z * cx + c) * hw + o] = (float)(s[k] / t.count(k)); });
        }
    }
    if (!grad_y) return;
#pragma unroll
    for (int k = 0; k < RPT; k++) G[(wave * RPT + k) * TW + lane] = gys[k];
    __syncthreads();
    const float *gp = g + (int64_t)n * HWf;
    float *op = grad_y + (int64_t)n * HWf;
    scatter_tile<BL>(t, G, rmapS, cmapS, H, W,
                     [&](int64_t o, double v) { op[o] = (float)(subtract_is_y ? v - (double)gp[o] : v); });
}

// acc[sel][b][c] (+)= sum over the chunk's labels of image b, in index order, of part[label][sel][c]; a label has
// `pstride` planes (the diagonal form: NPART * cx; the full form: one selector of `cx` = all its planes)
__global__ __launch_bounds__(NE) void k_grad_reduce(const double *__restrict__ part, double *__restrict__ acc, int n0, int nz, int cy,
                                                   int cx, int B, int nsel, int pstride, int64_t hw)
{
    const int64_t q = (int64_t)blockIdx.x * NE + threadIdx.x;
    if (q >= hw) return;
    const int c = blockIdx.y, b = n0 / cy + blockIdx.z;
    const int na = max(n0, b * cy), nb = min(n0 + nz, (b + 1) * cy);
    for (int sel = 0; sel < nsel; sel++) {
        double s = 0.0;
        for (int n = na; n < nb; n++) s += part[((int64_t)(n - n0) * pstride + (int64_t)sel * cx + c) * hw + q];
        double *d = acc + (((int64_t)sel * B + b) * cx + c) * hw + q;
        *d = na == b * cy ? s : *d + s;
    }
}

// D[b][c][p] (+)= sum over the chunk's labels of image b, in index order, of g_l[p] mean(A_lc)[lo(p)]
// (BL: of g_l[p] U(mean(A_lc))[p], the four taps and the mix of k_guide_up)
template <bool BL = false>
__global__ __launch_bounds__(NE) void k_grad_direct(const float *__restrict__ g, const float *__restrict__ mA, double *__restrict__ D,
                                                   const int *__restrict__ rlow, const int *__restrict__ clow, int n0, int nz, int cy,
                                                   int cx, int H, int W, int h, int w)
{
    const int64_t HWf = (int64_t)H * W, hw = (int64_t)h * w, p = (int64_t)blockIdx.x * NE + threadIdx.x;
    if (p >= HWf) return;
    const int c = blockIdx.y, b = n0 / cy + blockIdx.z;
    const int na = max(n0, b * cy), nb = min(n0 + nz, (b + 1) * cy);
    double s = 0.0;
    if constexpr (BL) {
        int i0, i1, j0, j1;
        double ly, lx;
        bil_tap((int)(p / W), (double)h / (double)H, h, i0, i1, ly);
        bil_tap((int)(p % W), (double)w / (double)W, w, j0, j1, lx);
        const int64_t q0 = (int64_t)i0 * w, q1 = (int64_t)i1 * w;
        for (int n = na; n < nb; n++) {
            const float *m = mA + ((int64_t)(n - n0) * cx + c) * hw;
            s += (double)g[(int64_t)n * HWf + p] * bil_mix(m[q0 + j0], m[q0 + j1], m[q1 + j0], m[q1 + j1], ly, lx);
        }
    } else {
        const int64_t lo = (int64_t)clampi(rlow[p / W], 0, h - 1) * w + clampi(clow[p % W], 0, w - 1);
        for (int n = na; n < nb; n++) s += (double)g[(int64_t)n * HWf + p] * (double)mA[((int64_t)(n - n0) * cx + c) * hw + lo];
    }
    double *d = D + ((int64_t)b * cx + c) * HWf + p;
    *d = na == b * cy ? s : *d + s;
}

__global__ __launch_bounds__(NE) void k_grad_finish(const double *__restrict__ acc, const double *__restrict__ mx,
                                                   float *__restrict__ F, int B, int cx, int64_t hw)
{
    const int64_t q = (int64_t)blockIdx.x * NE + threadIdx.x;
    if (q >= hw) return;
    const int64_t bc = (int64_t)blockIdx.z * cx + blockIdx.y, o = bc * hw + q;
    const double gv = acc[(int64_t)PART_VAR * B * cx * hw + o];
    F[(bc * 2 + 0) * hw + q] = (float)(acc[(int64_t)PART_MX * B * cx * hw + o] - 2.0 * mx[o] * gv);
    F[(bc * 2 + 1) * hw + q] = (float)gv;
}

template <bool ST, bool BL = false>
__global__ __launch_bounds__(NT) void k_grad_x(const float *__restrict__ F, const double *__restrict__ YU,
                                              const float *__restrict__ xs, const double *__restrict__ D, float *__restrict__ grad_x,
                                              const int *__restrict__ rmapS, const int *__restrict__ cmapS, int cx, int H, int W,
                                              int h, int w, int r, float scale)
{
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_APPLY);
    double *G = reinterpret_cast<double *>(t.in2);
    const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i0 = t.ti + wave * RPT, j = t.tj + lane;
    const int64_t hw = (int64_t)h * w, HWf = (int64_t)H * W;
    for (int c = 0; c < cx; c++) {
        const int64_t bc = (int64_t)b * cx + c;
        double s1[RPT], s2[RPT];
        plane_sums<ST>(t, t.in, F + (bc * 2 + 0) * hw, s1);
        plane_sums<ST>(t, t.in, F + (bc * 2 + 1) * hw, s2);
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int i = i0 + k;
            double v = 0.0;
            if (i < h && j < w) {
                const int64_t o = bc * hw + (int64_t)i * w + j;
                v = YU[o] + s1[k] + 2.0 * (double)xs[o] * s2[k];
            }
            G[(wave * RPT + k) * TW + lane] = v;
        }
        __syncthreads();
        const double *dp = D + bc * HWf;
        float *op = grad_x + bc * HWf;
        scatter_tile<BL>(t, G, rmapS, cmapS, H, W, [&](int64_t o, double v) { op[o] = (float)((double)scale * dp[o] + v); });
        // (the next channel's first write to G comes after the barriers of its plane_sums)
    }
}

// grad_eps_c = sum over images and pixels of gvar_c = (gvar_c / N) N: stage 1, NEB workgroups per channel, each thread a
// fixed strided share in index order, then a fixed tree in LDS; stage 2 adds the NEB partial sums in index order
// (gvn: `stride` planes an image; channel c's is plane c, or with `pairs` plane pair_plane(c, c) of the full form's gS)
__global__ __launch_bounds__(NE) void k_grad_eps1(const double *__restrict__ gvn, double *__restrict__ partial, int B, int cx, int h,
                                                 int w, int r, int stride, int pairs)
{
    __shared__ double sh[NE];
    const int c = blockIdx.y, pl = pairs ? pair_plane(c, c, cx) : c;
    const int64_t hw = (int64_t)h * w, total = (int64_t)B * hw;
    double s = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * NE + threadIdx.x; e < total; e += (int64_t)NEB * NE) {
        const int64_t b = e / hw, q = e % hw;
        const double n = (double)win_count((int)(q / w), r, h) * (double)win_count((int)(q % w), r, w);
        s += gvn[(b * stride + pl) * hw + q] * n;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = NE / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)c * NEB + blockIdx.x] = sh[0];
}

__global__ void k_grad_eps2(const double *__restrict__ partial, float *__restrict__ grad_eps, int cx)
{
    const int c = threadIdx.x;
    if (c >= cx) return;
    double s = 0.0;
    for (int k = 0; k < NEB; k++) s += partial[(int64_t)c * NEB + k];
    grad_eps[c] = (float)s;
}

// ---- backward of the full-covariance model -------------------------------------------------------------------------
// With m_c = mx_c, Sig = S (the full covariance's forward above), P = (Sig + diag(eps))^-1, cv_ld = cov_ld, and gA, gb, gA' as above:
//   gcv_ld = sum_c gA'_lc P_cd      gSig_cd = -1/2 sum_l (A_lc gcv_ld + A_ld gcv_lc)      gmy_l = gb_l - sum_d gcv_ld m_d
//   gm_c = -sum_l gb_l A_lc - sum_l gcv_lc my_l - 2 sum_d gSig_cd m_d
//   U_l0 = S(gmy_l / N)   U_lc = S(gcv_lc / N)   V_cd = S(gSig_cd / N)
//   gys_l = U_l0 + sum_c xs_c U_lc          gxs_c = sum_l ys_l U_lc + S(gm_c / N) + 2 sum_d xs_d V_cd
//   grad_y, grad_x from gys, gxs and mean(A) as above          grad_eps_c = sum gSig_cc
// (the diagonal form is the case of a diagonal P: gvar_c = gSig_cc).  U, gys and mean(A) have the diagonal form's shape, so
// backward() runs the diagonal form's sequence with k_guide_stats_full for the statistics and three kernels of its own:
//   k_grad_coef_full    per (label, tile), the channel count a template parameter as in the forward: the window sums of ys,
//                       ys xs_c, gb and gA_c stay in registers; cv, A = cv P, gA', gcv = gA' P, gmy per pixel in fp64 ->
//                       gcv_lc / N and gmy_l / N (the Q planes of k_grad_apply), A_lc (for grad_x), and as fp64 planes this
//                       label's terms of gSig_cd / N (pair_plane order) and of gm_c / N without its gSig term
//   k_grad_finish_full  once: gm_c / N with its - 2 sum_d gSig_cd m_d term and the gSig_cd / N, as fp32 planes
//   k_grad_x_full       per (image, tile): gxs_c (cx + 1 window sums per channel) into LDS -> grad_x as k_grad_x (BL: through
//                       D^T, scatter_tile<true>)
// A label's fp64 planes: [npairs gSig][cx gm][cx ys_l U_lc]; k_grad_reduce sums them into acc [B][npairs + 2 cx][h][w].
template <bool ST, int CX>
__global__ __launch_bounds__(NT) void k_grad_coef_full(const float *__restrict__ ys, const float *__restrict__ xs,
                                                      const float *__restrict__ Pd, const double *__restrict__ mx,
                                                      const double *__restrict__ Pm, float *__restrict__ Q, float *__restrict__ A,
                                                      double *__restrict__ part, int n0, int cy, int h, int w, int r)
{
    constexpr int NP = npairs(CX), NPL = NP + 2 * CX;
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_COEF);
    const int z = blockIdx.z, b = (n0 + z) / cy;
    const int64_t hw = (int64_t)h * w;
    const float *yp = ys + (int64_t)z * hw, *xb = xs + (int64_t)b * CX * hw, *gd = Pd + (int64_t)z * (CX + 1) * hw;
    const double *mp = mx + (int64_t)b * CX * hw, *pp = Pm + (int64_t)b * NP * hw;
    float *qp = Q + (int64_t)z * (CX + 1) * hw, *ap = A ? A + (int64_t)z * CX * hw : nullptr;
    double *tp = part ? part + (int64_t)z * NPL * hw : nullptr;

    double my[RPT], gb[RPT], rn[RPT], s[RPT], cov[CX][RPT], gA[CX][RPT];
    recip_counts(t, rn);
    plane_sums<ST>(t, t.in, yp, s);                                 // (tiled form: ys stays in LDS for the products below)
#pragma unroll
    for (int k = 0; k < RPT; k++) my[k] = s[k] * rn[k];
    static_for<CX>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        product_sums<ST>(t, yp, xb + c * hw, s);
#pragma unroll
        for (int k = 0; k < RPT; k++) cov[c][k] = s[k] * rn[k];       // mean(y x_c) for now
    });
    plane_sums<ST>(t, t.in2, gd + CX * hw, gb);
    static_for<CX>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        plane_sums<ST>(t, t.in2, gd + c * hw, gA[c]);
    });
    for_pixels(t, [&](int k, int64_t o) {
        double m[CX], p[NP], cv[CX], gap[CX], a[CX], gcv[CX], gmy = gb[k];
#pragma unroll
        for (int c = 0; c < CX; c++) m[c] = mp[c * hw + o], cv[c] = cov[c][k] - my[k] * m[c], gap[c] = gA[c][k] - gb[k] * m[c];
#pragma unroll
        for (int i = 0; i < NP; i++) p[i] = pp[i * hw + o];
#pragma unroll
        for (int c = 0; c < CX; c++) {
            double va = 0.0, vg = 0.0;
#pragma unroll
            for (int d = 0; d < CX; d++) {
                const double pcd = p[pair_plane(min(c, d), max(c, d), CX)];
                va += cv[d] * pcd, vg += gap[d] * pcd;
            }
            a[c] = va, gcv[c] = vg;
            gmy -= vg * m[c];
            qp[c * hw + o] = (float)(vg * rn[k]);
            if (ap) ap[c * hw + o] = (float)va;
        }
        qp[CX * hw + o] = (float)(gmy * rn[k]);
        if (tp) {
#pragma unroll
            for (int c = 0; c < CX; c++) {
#pragma unroll
                for (int d = c; d < CX; d++) tp[pair_plane(c, d, CX) * hw + o] = -0.5 * (a[c] * gcv[d] + a[d] * gcv[c]) * rn[k];
                tp[(NP + c) * hw + o] = -(gb[k] * a[c] + gcv[c] * my[k]) * rn[k];
            }
        }
    });
}

// F[b][c] = gm_c / N, c < cx, and F[b][cx + i] = gSig / N of pair i, from acc [B][npl][h][w] (gSig first, then gm's terms)
__global__ __launch_bounds__(NE) void k_grad_finish_full(const double *__restrict__ acc, const double *__restrict__ mx,
                                                        float *__restrict__ F, int cx, int npl, int64_t hw)
{
    const int64_t q = (int64_t)blockIdx.x * NE + threadIdx.x;
    if (q >= hw) return;
    const int b = blockIdx.z, np = npairs(cx);
    const double *ab = acc + (int64_t)b * npl * hw + q, *mb = mx + (int64_t)b * cx * hw + q;
    float *fb = F + (int64_t)b * (cx + np) * hw + q;
    for (int c = 0; c < cx; c++) {
        double v = ab[(int64_t)(np + c) * hw];
        for (int d = 0; d < cx; d++) v -= 2.0 * ab[(int64_t)pair_plane(min(c, d), max(c, d), cx) * hw] * mb[(int64_t)d * hw];
        fb[(int64_t)c * hw] = (float)v;
    }
    for (int i = 0; i < np; i++) fb[(int64_t)(cx + i) * hw] = (float)ab[(int64_t)i * hw];
}

template <bool ST, bool BL = false>
__global__ __launch_bounds__(NT) void k_grad_x_full(const float *__restrict__ F, const double *__restrict__ acc,
                                                   const float *__restrict__ xs, const double *__restrict__ D,
                                                   float *__restrict__ grad_x, const int *__restrict__ rmapS,
                                                   const int *__restrict__ cmapS, int cx, int npl, int H, int W, int h, int w, int r,
                                                   float scale)
{
    Tile t = make_tile<ST>(r, h, w, nullptr, nullptr, h, w, KIND_APPLY);
    double *G = reinterpret_cast<double *>(t.in2);
    const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i0 = t.ti + wave * RPT, j = t.tj + lane;
    const int np = npairs(cx);
    const int64_t hw = (int64_t)h * w, HWf = (int64_t)H * W;
    const float *fb = F + (int64_t)b * (cx + np) * hw, *xb = xs + (int64_t)b * cx * hw;
    const double *yu = acc + ((int64_t)b * npl + np + cx) * hw;      // sum_l ys_l U_lc
    for (int c = 0; c < cx; c++) {
        double v[RPT], s[RPT];
        plane_sums<ST>(t, t.in, fb + (int64_t)c * hw, v);
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const bool in = i0 + k < h && j < w;
            v[k] = in ? v[k] + yu[(int64_t)c * hw + (int64_t)(i0 + k) * w + j] : 0.0;
        }
        for (int d = 0; d < cx; d++) {
            plane_sums<ST>(t, t.in, fb + (int64_t)(cx + pair_plane(min(c, d), max(c, d), cx)) * hw, s);
#pragma unroll
            for (int k = 0; k < RPT; k++)
                if (i0 + k < h && j < w) v[k] += 2.0 * (double)xb[(int64_t)d * hw + (int64_t)(i0 + k) * w + j] * s[k];
        }
#pragma unroll
        for (int k = 0; k < RPT; k++) G[(wave * RPT + k) * TW + lane] = v[k];
        __syncthreads();
        const double *dp = D + ((int64_t)b * cx + c) * HWf;
        float *op = grad_x + ((int64_t)b * cx + c) * HWf;
        scatter_tile<BL>(t, G, rmapS, cmapS, H, W, [&](int64_t o, double v) { op[o] = (float)((double)scale * dp[o] + v); });
        // (the next channel's first write to G comes after the barriers of its plane_sums)
    }
}


// ---- host ----------------------------------------------------------------------------------------------------------
// One argument record from the entry point to the launches, one trait for the two linear models, forward<ST, CX, BL> and
// backward<ST, CX, BL> for every variant, one dispatch over (tiled, CX, BL), one checked front per direction.
inline bool fits_tiled(int r) { return max_lds(r) <= kMaxLds && halo_stride(r) <= 64 * NCO; }

// a label's fp64 planes that the backward sums over labels: NPART per channel, or with the full covariance
// [npairs gSig][cx gm][cx ys_l U_lc]
constexpr int grad_planes(bool full_cov, int cx) { return full_cov ? npairs(cx) + 2 * cx : kGradParts * cx; }

// The tiled form while its LDS fits the radius, else the streamed form; the tile grid; the dynamic LDS of the three
// layouts (one halo tile, two, one + the window means); the labels of a chunk.
struct Plan {
    bool tiled;
    dim3 tiles;
    size_t lds_stats, lds_coef, lds_apply;
    Plan(int re, int h, int w)
        : tiled(fits_tiled(re)), tiles((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH)),
          lds_stats(tiled ? tile_lds(re, 1, false) : stream_lds(false)), lds_coef(tiled ? tile_lds(re, 2, false) : stream_lds(false)),
          lds_apply(tiled ? tile_lds(re, 1, true) : stream_lds(true))
    {
    }
    dim3 grid(unsigned nz) const { return dim3(tiles.x, tiles.y, nz); }
    // labels per chunk: the per-label planes of a chunk (`per` bytes a label) stay within kChunkBytes (and gridDim.y / z)
    static int64_t chunk(int64_t nimg, int64_t per) { return max((int64_t)1, min(min(nimg, (int64_t)65535), (int64_t)kChunkBytes / per)); }
    // `per` of the forward (the cx + 1 coefficient planes; bilinear: the cx + 1 window-mean planes beside them) and of the
    // backward (ys unless full resolution, P and Q, A and mA for grad_x, the `planes` = grad_planes() fp64 terms for
    // grad_x / grad_eps; the bilinear backwards hold the planes of the nearest form below full resolution): forward(),
    // backward() and the three queries all come here
    static int64_t per_forward(int cx, int64_t hw, bool bilinear) { return (bilinear ? 2 : 1) * (int64_t)(cx + 1) * hw * (int64_t)sizeof(float); }
    static int64_t per_backward(int cx, int64_t hw, int planes, bool full, bool need_x, bool need_xe)
    {
        return hw * (int64_t)((full ? 0 : 4) + 8 * (cx + 1) + (need_x ? 8 * cx : 0) + (need_xe ? 8 * planes : 0));
    }
};

struct Args {
    const char *who;                                // the entry point, for the messages
    const float *y, *x, *third;                     // third: the forward's src (may be null), the backward's g
    float *out, *grad_y, *grad_x, *grad_eps;        // the forward's out; the backward's gradients, null where not asked for
    int B, cy, cx, H, W, h, w, r;                   // r as the caller gave it; past the checks min(r, max(h, w))
    const int *row_of_low, *col_of_low, *low_of_row, *low_of_col;      // the nearest index maps; all null: bilinear sampling
    const float *eps;
    float scale;
    int subtract_is_y;
    hipStream_t st;
    int64_t hw() const { return (int64_t)h * w; }
    int64_t HWf() const { return (int64_t)H * W; }
    int64_t nimg() const { return (int64_t)B * cy; }
};

// The two linear models, in every place where their host paths differ.  Model<0> below is the diagonal one, a model per
// guide channel, the channel count a run-time argument of its kernels.  Model<CX>, CX = 1 .. PHL_GUIDED_FULL_MAX_CX, is the
// full covariance of CX = cx channels.  The members that launch take the tile's source planes (`x`, H x W) beside the
// record: the backward's statistics run on the gathered samples, whatever the sampling, with BL = false.
template <int CX>
struct Model {
    static constexpr int NP = npairs(CX), NPL = grad_planes(true, CX);
    using Stat = double;                                                      // beside mx: the upper triangle of P, fp64
    static int stat_planes(int) { return NP; }
    static size_t lds_stats(const Plan &p) { return p.lds_coef; }            // products of two channels: two halo tiles
    static int label_planes(int) { return NPL; }                             // grad_planes(); ys_l U_lc from yu_plane on
    static int yu_plane(int) { return NP + CX; }
    static int f_planes(int) { return CX + NP; }                             // fp32 planes of an image in F
    template <bool ST, bool BL> static auto stats_k() { return k_guide_stats_full<ST, CX, BL>; }
    template <bool ST, bool BL> static auto coef_k() { return k_guide_coef_full<ST, CX, BL>; }
    template <bool ST> static auto grad_coef_k() { return k_grad_coef_full<ST, CX>; }
    template <bool ST, bool BL> static auto grad_x_k() { return k_grad_x_full<ST, BL>; }
    template <bool ST, bool BL>
    static void stats(const Args &a, const Plan &p, const float *x, int H, int W, double *mx, Stat *P)
    {
        stats_k<ST, BL>()<<<p.grid((unsigned)a.B), dim3(NT), lds_stats(p), a.st>>>(x, a.row_of_low, a.col_of_low, a.eps, mx, P, H, W, a.h, a.w, a.r);
    }
    template <bool ST, bool BL>
    static void coef(const Args &a, const Plan &p, int64_t n0, unsigned nz, const double *mx, const Stat *P, float *coef)
    {
        coef_k<ST, BL>()<<<p.grid(nz), dim3(NT), p.lds_coef, a.st>>>(
            a.y, a.x, a.row_of_low, a.col_of_low, mx, P, coef, (int)n0, a.cy, a.H, a.W, a.h, a.w, a.r);
    }
    template <bool ST>
    static void grad_coef(const Args &a, const Plan &p, int64_t n0, unsigned nz, const float *ys, const float *xs, const float *Pd,
                          const double *mx, const Stat *P, float *Q, float *A, double *part)
    {
        grad_coef_k<ST>()<<<p.grid(nz), dim3(NT), p.lds_coef, a.st>>>(ys, xs, Pd, mx, P, Q, A, part, (int)n0, a.cy, a.h, a.w, a.r);
    }
    // one selector of NPL "channels"; without grad_x nothing reads past the gSig planes
    static void reduce(const Args &a, unsigned nblo, unsigned nb, const double *part, double *acc, int64_t n0, unsigned nz, bool need_x)
    {
        k_grad_reduce<<<dim3(nblo, (unsigned)(need_x ? NPL : NP), nb), dim3(NE), 0, a.st>>>(
            part, acc, (int)n0, (int)nz, a.cy, NPL, a.B, 1, NPL, a.hw());
    }
    template <bool ST, bool BL>
    static void finish_x(const Args &a, const Plan &p, unsigned nblo, const double *acc, const double *mx, float *F, const float *xs, const double *D)
    {
        k_grad_finish_full<<<dim3(nblo, 1, (unsigned)a.B), dim3(NE), 0, a.st>>>(acc, mx, F, CX, NPL, a.hw());
        grad_x_k<ST, BL>()<<<p.grid((unsigned)a.B), dim3(NT), p.lds_apply, a.st>>>(
            F, acc, xs, D, a.grad_x, a.row_of_low, a.col_of_low, CX, NPL, a.H, a.W, a.h, a.w, a.r, a.scale);
    }
    static void eps1(const Args &a, const double *acc, double *epart)       // gvar_c = gSig_cc: plane pair_plane(c, c) of NPL
    {
        k_grad_eps1<<<dim3(NEB, (unsigned)CX), dim3(NE), 0, a.st>>>(acc, epart, a.B, CX, a.h, a.w, a.r, NPL, 1);
    }
};

template <>
struct Model<0> {
    using Stat = float;                                                       // beside mx: inv = 1 / (var + eps), fp32
    static int stat_planes(int cx) { return cx; }
    static size_t lds_stats(const Plan &p) { return p.lds_stats; }
    static int label_planes(int cx) { return grad_planes(false, cx); }       // [NPART][cx]; ys_l U_lc is part PART_YU
    static int yu_plane(int cx) { return PART_YU * cx; }
    static int f_planes(int cx) { return 2 * cx; }
    template <bool ST, bool BL> static auto stats_k() { return k_guide_stats<ST, BL>; }
    template <bool ST, bool BL> static auto coef_k() { return k_guide_coef<ST, BL>; }
    template <bool ST> static auto grad_coef_k() { return k_grad_coef<ST>; }
    template <bool ST, bool BL> static auto grad_x_k() { return k_grad_x<ST, BL>; }
    template <bool ST, bool BL>
    static void stats(const Args &a, const Plan &p, const float *x, int H, int W, double *mx, Stat *inv)
    {
        stats_k<ST, BL>()<<<p.grid((unsigned)a.B), dim3(NT), lds_stats(p), a.st>>>(
            x, a.row_of_low, a.col_of_low, a.eps, mx, inv, a.cx, H, W, a.h, a.w, a.r);
    }
    template <bool ST, bool BL>
    static void coef(const Args &a, const Plan &p, int64_t n0, unsigned nz, const double *mx, const Stat *inv, float *coef)
    {
        coef_k<ST, BL>()<<<p.grid(nz), dim3(NT), p.lds_coef, a.st>>>(
            a.y, a.x, a.row_of_low, a.col_of_low, mx, inv, coef, (int)n0, a.cy, a.cx, a.H, a.W, a.h, a.w, a.r);
    }
    template <bool ST>
    static void grad_coef(const Args &a, const Plan &p, int64_t n0, unsigned nz, const float *ys, const float *xs, const float *Pd,
                          const double *mx, const Stat *inv, float *Q, float *A, double *part)
    {
        grad_coef_k<ST>()<<<p.grid(nz), dim3(NT), p.lds_coef, a.st>>>(ys, xs, Pd, mx, inv, Q, A, part, (int)n0, a.cy, a.cx, a.h, a.w, a.r);
    }
    // NPART selectors of cx channels; without grad_x nothing reads the PART_YU planes
    static void reduce(const Args &a, unsigned nblo, unsigned nb, const double *part, double *acc, int64_t n0, unsigned nz, bool need_x)
    {
        k_grad_reduce<<<dim3(nblo, (unsigned)a.cx, nb), dim3(NE), 0, a.st>>>(
            part, acc, (int)n0, (int)nz, a.cy, a.cx, a.B, need_x ? NPART : 2, NPART * a.cx, a.hw());
    }
    template <bool ST, bool BL>
    static void finish_x(const Args &a, const Plan &p, unsigned nblo, const double *acc, const double *mx, float *F, const float *xs, const double *D)
    {
        k_grad_finish<<<dim3(nblo, (unsigned)a.cx, (unsigned)a.B), dim3(NE), 0, a.st>>>(acc, mx, F, a.B, a.cx, a.hw());
        grad_x_k<ST, BL>()<<<p.grid((unsigned)a.B), dim3(NT), p.lds_apply, a.st>>>(
            F, acc + (size_t)PART_YU * a.B * a.cx * a.hw(), xs, D, a.grad_x, a.row_of_low, a.col_of_low, a.cx, a.H, a.W, a.h, a.w, a.r,
            a.scale);
    }
    static void eps1(const Args &a, const double *acc, double *epart)       // gvar_c: plane c of part PART_VAR = 0
    {
        k_grad_eps1<<<dim3(NEB, (unsigned)a.cx), dim3(NE), 0, a.st>>>(acc, epart, a.B, a.cx, a.h, a.w, a.r, a.cx, 0);
    }
};

// The forward of every variant.  Nearest: the statistics once, then per chunk of labels the coefficients and
// k_guide_apply.  BL: the first two fill their tiles with the four-tap samples, and k_guide_mean and k_guide_up take the
// place of k_guide_apply.
template <bool ST, int CX, bool BL>
int forward(const Args &a, const Plan &p)
{
    using M = Model<CX>;
    const int cx = a.cx;
    const int64_t hw = a.hw(), nimg = a.nimg();
    if (int rc = phl_allow_lds(M::template stats_k<ST, BL>(), M::lds_stats(p))) return rc;
    if (int rc = phl_allow_lds(M::template coef_k<ST, BL>(), p.lds_coef)) return rc;
    if (int rc = BL ? phl_allow_lds(k_guide_mean<ST>, p.lds_stats) : phl_allow_lds(k_guide_apply<ST>, p.lds_apply)) return rc;

    const int64_t chunk = Plan::chunk(nimg, Plan::per_forward(cx, hw, BL));
    phl_temps tmp(a.st);
    double *mx = tmp.get<double>((size_t)a.B * cx * hw);
    auto *sp = tmp.get<typename M::Stat>((size_t)a.B * M::stat_planes(cx) * hw);
    float *coef = tmp.get<float>((size_t)chunk * (cx + 1) * hw), *mean = BL ? tmp.get<float>((size_t)chunk * (cx + 1) * hw) : nullptr;
    const int tilesx = (a.W + 63) / 64, tilesy = (a.H + 4 * UR - 1) / (4 * UR);        // of k_guide_up
    int &rc = tmp.rc;
    if (rc == PHL_OK) {
        M::template stats<ST, BL>(a, p, a.x, a.H, a.W, mx, sp);
        phl_launched(rc, "the guided filter's statistics");
    }
    for (int64_t n0 = 0; n0 < nimg && rc == PHL_OK; n0 += chunk) {
        const unsigned nz = (unsigned)min(chunk, nimg - n0);
        M::template coef<ST, BL>(a, p, n0, nz, mx, sp, coef);
        if constexpr (BL) {
            k_guide_mean<ST><<<p.grid(nz), dim3(NT), p.lds_stats, a.st>>>(coef, mean, cx + 1, a.h, a.w, a.r);
            k_guide_up<<<dim3((unsigned)tilesx * (unsigned)tilesy, 1, nz), dim3(NT), 0, a.st>>>(
                mean, a.x, a.third, a.out, (int)n0, a.cy, cx, a.H, a.W, a.h, a.w, tilesx, a.scale);
        } else {
            k_guide_apply<ST><<<p.grid(nz), dim3(NT), p.lds_apply, a.st>>>(
                coef, a.x, a.third, a.out, a.low_of_row, a.low_of_col, (int)n0, a.cy, cx, a.H, a.W, a.h, a.w, a.r, a.scale);
        }
        phl_launched(rc, "the guided filter's chunk kernels");
    }
    return tmp.release();
}

// The backward of every variant.  BL (no maps): the four pieces that connect the two resolutions in their bilinear form
// (k_grad_gather, k_grad_down, scatter_tile in k_grad_apply and the x kernel, k_grad_direct).  The statistics then run on
// the stored samples xs with identity maps: the BL = false kernel forms its window sums in the order of the forward's
// BL = true one, whose only difference is the four-tap tile fill that k_grad_gather<true> repeats, so mx and inv / P
// are the forward's bit for bit.
template <bool ST, int CX, bool BL>
int backward(const Args &a, const Plan &p)
{
    using M = Model<CX>;
    const int cx = a.cx, cy = a.cy, npl = M::label_planes(cx);
    const float *g = a.third;
    const bool full = !BL && a.h == a.H && a.w == a.W;          // strictly increasing maps onto the same size: the identity
    const bool need_x = a.grad_x != nullptr, need_xe = need_x || a.grad_eps != nullptr, need_apply = need_x || a.grad_y != nullptr;
    const int64_t hw = a.hw(), HWf = a.HWf(), nimg = a.nimg();
    const unsigned nblo = (unsigned)((hw + NE - 1) / NE), nbfull = (unsigned)((HWf + NE - 1) / NE);
    if (int rc = phl_allow_lds(M::template stats_k<ST, false>(), M::lds_stats(p))) return rc;
    if (int rc = phl_allow_lds(M::template grad_coef_k<ST>(), p.lds_coef)) return rc;
    if (int rc = phl_allow_lds(k_grad_apply<ST, BL>, p.lds_apply)) return rc;
    if (int rc = phl_allow_lds(M::template grad_x_k<ST, BL>(), p.lds_apply)) return rc;

    const int64_t chunk = Plan::chunk(nimg, Plan::per_backward(cx, hw, npl, full, need_x, need_xe));
    const size_t nstat = (size_t)a.B * cx * hw;
    phl_temps tmp(a.st);
    double *mx = tmp.get<double>(nstat);
    auto *sp = tmp.get<typename M::Stat>((size_t)a.B * M::stat_planes(cx) * hw);
    float *xsb = full ? nullptr : tmp.get<float>(nstat);
    float *ysb = full ? nullptr : tmp.get<float>((size_t)chunk * hw);
    float *Pd = tmp.get<float>((size_t)chunk * (cx + 1) * hw), *Q = tmp.get<float>((size_t)chunk * (cx + 1) * hw);
    float *A = need_x ? tmp.get<float>((size_t)chunk * cx * hw) : nullptr, *mA = need_x ? tmp.get<float>((size_t)chunk * cx * hw) : nullptr;
    double *part = need_xe ? tmp.get<double>((size_t)chunk * npl * hw) : nullptr;
    double *acc = need_xe ? tmp.get<double>((size_t)a.B * npl * hw) : nullptr;
    float *F = need_x ? tmp.get<float>((size_t)a.B * M::f_planes(cx) * hw) : nullptr;
    double *D = need_x ? tmp.get<double>((size_t)a.B * cx * HWf) : nullptr;
    double *epart = a.grad_eps ? tmp.get<double>((size_t)cx * NEB) : nullptr;
    int &rc = tmp.rc;
    const float *xs = full ? a.x : xsb;
    if (rc == PHL_OK) {
        if (!full)
            k_grad_gather<BL><<<dim3(nblo, (unsigned)cx, (unsigned)a.B), dim3(NE), 0, a.st>>>(
                a.x, xsb, a.row_of_low, a.col_of_low, a.H, a.W, a.h, a.w);
        if constexpr (BL)
            M::template stats<ST, false>(a, p, xsb, a.h, a.w, mx, sp);
        else
            M::template stats<ST, false>(a, p, a.x, a.H, a.W, mx, sp);
        phl_launched(rc, "the guided filter's statistics / k_grad_gather");
    }
    for (int64_t n0 = 0; n0 < nimg && rc == PHL_OK; n0 += chunk) {
        const unsigned nz = (unsigned)min(chunk, nimg - n0);
        const unsigned nb = (unsigned)((n0 + nz - 1) / cy - n0 / cy + 1);          // images the chunk touches
        const float *ys = full ? a.y + n0 * HWf : ysb;
        if (!full) k_grad_gather<BL><<<dim3(nblo, nz, 1), dim3(NE), 0, a.st>>>(a.y + n0 * HWf, ysb, a.row_of_low, a.col_of_low, a.H, a.W, a.h, a.w);
        k_grad_down<BL><<<dim3(nblo, nz), dim3(NE), 0, a.st>>>(
            g, a.x, Pd, a.low_of_row, a.low_of_col, (int)n0, cy, cx, a.H, a.W, a.h, a.w, a.r, a.scale);
        M::template grad_coef<ST>(a, p, n0, nz, ys, xs, Pd, mx, sp, Q, A, part);
        if (need_apply)
            k_grad_apply<ST, BL><<<p.grid(nz), dim3(NT), p.lds_apply, a.st>>>(
                Q, A, ys, xs, g, a.grad_y, mA, need_x ? part : nullptr, a.row_of_low, a.col_of_low, (int)n0, cy, cx, a.H, a.W, a.h, a.w,
                a.r, a.subtract_is_y, npl, M::yu_plane(cx));
        if (need_xe) M::reduce(a, nblo, nb, part, acc, n0, nz, need_x);
        if (need_x)
            k_grad_direct<BL><<<dim3(nbfull, (unsigned)cx, nb), dim3(NE), 0, a.st>>>(
                g, mA, D, a.low_of_row, a.low_of_col, (int)n0, (int)nz, cy, cx, a.H, a.W, a.h, a.w);
        phl_launched(rc, "the guided filter backward's chunk kernels");
    }
    if (need_x && rc == PHL_OK) {
        M::template finish_x<ST, BL>(a, p, nblo, acc, mx, F, xs, D);
        phl_launched(rc, "k_grad_finish / k_grad_x");
    }
    if (a.grad_eps && rc == PHL_OK) {
        M::eps1(a, acc, epart);
        k_grad_eps2<<<dim3(1), dim3(64), 0, a.st>>>(epart, a.grad_eps, cx);
        phl_launched(rc, "k_grad_eps");
    }
    return tmp.release();
}

// (tiled, cx of the full covariance or 0, bilinear) -> f(ST, CX, BL) as integral constants: every instantiation of
// forward() and backward() comes from here
template <typename F>
int dispatch(bool tiled, int CX, bool BL, F f)
{
    static_assert(PHL_GUIDED_FULL_MAX_CX == 4, "one instantiation per channel count");
    int rc = PHL_ERR_INVALID;
    dispatch_bool(!tiled, [&](auto st) {
        dispatch_bool(BL, [&](auto bl) { dispatch_int<0, 1, 2, 3, 4>(CX, [&](auto cx) { rc = f(st, cx, bl); }); });
    });
    return rc;
}

// The arguments the forward and the backward share (`need`: out or g).  PHL_OK also for zero elements, which the
// caller then tests for.
int check_guided_args(const Args &a, const void *need, const char *need_name, bool maps)
{
    if (a.B < 0 || a.cy < 0 || a.cx < 1 || a.H < 0 || a.W < 0 || a.h < 0 || a.w < 0 || a.r < 0 || a.h > a.H || a.w > a.W ||
        !isfinite(a.scale)) {
        phl_set_error("%s: bad arguments (B=%d cy=%d cx=%d H=%d W=%d h=%d w=%d r=%d scale=%g)", a.who, a.B, a.cy, a.cx, a.H, a.W, a.h,
                      a.w, a.r, (double)a.scale);
        return PHL_ERR_INVALID;
    }
    if (a.B == 0 || a.cy == 0 || a.H == 0 || a.W == 0) return PHL_OK;
    if (a.h == 0 || a.w == 0) {
        phl_set_error("%s: empty solving resolution %d x %d for a %d x %d image", a.who, a.h, a.w, a.H, a.W);
        return PHL_ERR_INVALID;
    }
    if (!a.y || !a.x || !need || !a.eps || (maps && (!a.row_of_low || !a.col_of_low || !a.low_of_row || !a.low_of_col))) {
        phl_set_error("%s: null y / x / %s / eps / index map", a.who, need_name);
        return PHL_ERR_INVALID;
    }
    const int64_t HWf = a.HWf(), lim = INT64_MAX / 64;      // byte counts of the fp64 temporaries stay in int64
    const int64_t nimg = a.nimg();
    if (HWf > INT32_MAX || nimg > INT32_MAX || HWf > lim / nimg || HWf > lim / ((int64_t)a.B * a.cx) || (a.h + TH - 1) / TH > 65535 ||
        a.B > 65535 || max(a.H, a.W) > (1 << 30)) {
        phl_set_error("%s: %d x %d x (%d | %d) x %d x %d elements are too many", a.who, a.B, a.cy, a.cx, a.cy, a.H, a.W);
        return PHL_ERR_TOO_LARGE;
    }
    if (a.cx > PHL_GUIDED_MAX_CX) {
        phl_set_error("%s: %d guide channels, at most %d", a.who, a.cx, PHL_GUIDED_MAX_CX);
        return PHL_ERR_UNSUPPORTED;
    }
    return PHL_OK;
}

// What every entry point checks, in this order: the shared arguments; nothing to do (zero elements, no gradient asked
// for: PHL_OK); the flags word (`known`: the bits this entry point takes); the channels of the full covariance; the
// bilinear backward's ratio; aliasing.  Then the window is clipped and the variant dispatched.  `bilinear`: no index maps.
int checked(Args a, bool grad, bool bilinear, bool full_cov, unsigned flags = 0, unsigned known = 0)
{
    if (int rc = check_guided_args(a, grad ? (const void *)a.third : a.out, grad ? "g" : "out", !bilinear)) return rc;
    if (a.B == 0 || a.cy == 0 || a.H == 0 || a.W == 0 || (grad && !a.grad_y && !a.grad_x && !a.grad_eps)) return PHL_OK;
    if (flags & ~known) {
        phl_set_error("%s: unknown flags 0x%x%s", a.who, flags,
                      grad ? " (the full-covariance backward is phl_guided_filter_bilinear_full_grad)" : "");
        return PHL_ERR_UNSUPPORTED;
    }
    full_cov = full_cov || (flags & PHL_GUIDED_BILINEAR_FULL_COV) != 0;
    if (full_cov && a.cx > PHL_GUIDED_FULL_MAX_CX) {
        phl_set_error("%s: %d guide channels with the full covariance, at most %d (PHL_GUIDED_FULL_MAX_CX)", a.who, a.cx,
                      PHL_GUIDED_FULL_MAX_CX);
        return PHL_ERR_UNSUPPORTED;
    }
    if (grad && bilinear && (2 * (int64_t)a.h > a.H || 2 * (int64_t)a.w > a.W)) {       // below a ratio of 2 two samples of D may share a tap
        phl_set_error("%s: %d x %d is more than half of %d x %d", a.who, a.h, a.w, a.H, a.W);
        return PHL_ERR_UNSUPPORTED;
    }
    // the forward's out is no input; no gradient is an input or another gradient
    const void *ins[4] = {a.y, a.x, a.third, grad ? a.eps : nullptr}, *outs[3] = {grad ? a.grad_y : a.out, a.grad_x, a.grad_eps};
    for (int o = 0; o < 3; o++)
        for (int i = 0; i < 4; i++)
            if (outs[o] && (outs[o] == ins[i] || (i < o && outs[o] == outs[i]))) {
                phl_set_error(grad ? "%s: a gradient aliases an input or another gradient" : "%s: out aliases an input", a.who);
                return PHL_ERR_INVALID;
            }
    a.r = min(a.r, max(a.h, a.w));            // a window beyond the image on both axes sums the same pixels
    const Plan p(a.r, a.h, a.w);
    return dispatch(p.tiled, full_cov ? a.cx : 0, bilinear, [&](auto st, auto cx, auto bl) {
        constexpr bool ST = decltype(st)::value, BL = decltype(bl)::value;
        constexpr int CX = decltype(cx)::value;
        return grad ? backward<ST, CX, BL>(a, p) : forward<ST, CX, BL>(a, p);
    });
}

int checked_forward(const Args &a, bool bilinear, bool full_cov, unsigned flags = 0)
{
    return checked(a, false, bilinear, full_cov, flags, bilinear ? PHL_GUIDED_BILINEAR_FULL_COV : 0);
}
int checked_backward(const Args &a, bool bilinear, bool full_cov, unsigned flags = 0) { return checked(a, true, bilinear, full_cov, flags); }

}  // namespace

extern "C" {

int phl_guided_filter_max_r(void)
{
    int r = 0;
    while (fits_tiled(r + 1)) r++;
    return r;
}

int phl_guided_filter_grad_max_r(void) { return phl_guided_filter_max_r(); }     // the same two LDS layouts as the forward

int phl_guided_filter_labels_per_chunk(int B, int cy, int cx, int h, int w, int full, int needs)
{
    if (B < 1 || cy < 1 || cx < 1 || h < 1 || w < 1 || needs < -1 || needs > 7) return 0;
    const int64_t hw = (int64_t)h * w, nimg = (int64_t)B * cy;
    const bool need_x = (needs & 2) != 0, need_xe = (needs & 6) != 0;
    return (int)Plan::chunk(nimg, needs < 0 ? Plan::per_forward(cx, hw, false)
                                            : Plan::per_backward(cx, hw, grad_planes(false, cx), full != 0, need_x, need_xe));
}

int phl_guided_filter_full_grad_labels_per_chunk(int B, int cy, int cx, int h, int w, int full, int needs)
{
    if (B < 1 || cy < 1 || cx < 1 || cx > PHL_GUIDED_FULL_MAX_CX || h < 1 || w < 1 || needs < 0 || needs > 7) return 0;
    const bool need_x = (needs & 2) != 0, need_xe = (needs & 6) != 0;
    return (int)Plan::chunk((int64_t)B * cy, Plan::per_backward(cx, (int64_t)h * w, grad_planes(true, cx), full != 0, need_x, need_xe));
}

int phl_guided_filter_bilinear_labels_per_chunk(int B, int cy, int cx, int h, int w)
{
    if (B < 1 || cy < 1 || cx < 1 || h < 1 || w < 1) return 0;
    return (int)Plan::chunk((int64_t)B * cy, Plan::per_forward(cx, (int64_t)h * w, true));
}

int phl_guided_filter(const float *y, const float *x, const float *src, float *out, int B, int cy, int cx, int H, int W, int h, int w,
                      int r, const int *row_of_low, const int *col_of_low, const int *low_of_row, const int *low_of_col,
                      const float *eps, float scale, phl_stream stream)
{
    return checked_forward({"phl_guided_filter", y, x, src, out, nullptr, nullptr, nullptr, B, cy, cx, H, W, h, w, r, row_of_low,
                            col_of_low, low_of_row, low_of_col, eps, scale, 0, (hipStream_t)stream}, false, false);
}

int phl_guided_filter_full(const float *y, const float *x, const float *src, float *out, int B, int cy, int cx, int H, int W, int h,
                           int w, int r, const int *row_of_low, const int *col_of_low, const int *low_of_row, const int *low_of_col,
                           const float *eps, float scale, phl_stream stream)
{
    return checked_forward({"phl_guided_filter_full", y, x, src, out, nullptr, nullptr, nullptr, B, cy, cx, H, W, h, w, r, row_of_low,
                            col_of_low, low_of_row, low_of_col, eps, scale, 0, (hipStream_t)stream}, false, true);
}

int phl_guided_filter_bilinear(const float *y, const float *x, const float *src, float *out, int B, int cy, int cx, int H, int W, int h,
                               int w, int r, const float *eps, float scale, unsigned flags, phl_stream stream)
{
    return checked_forward({"phl_guided_filter_bilinear", y, x, src, out, nullptr, nullptr, nullptr, B, cy, cx, H, W, h, w, r, nullptr,
                            nullptr, nullptr, nullptr, eps, scale, 0, (hipStream_t)stream}, true, false, flags);
}

int phl_guided_filter_grad(const float *y, const float *x, const float *g, float *grad_y, float *grad_x, float *grad_eps, int B, int cy,
                           int cx, int H, int W, int h, int w, int r, const int *row_of_low, const int *col_of_low,
                           const int *low_of_row, const int *low_of_col, const float *eps, float scale, int subtract_is_y,
                           phl_stream stream)
{
    return checked_backward({"phl_guided_filter_grad", y, x, g, nullptr, grad_y, grad_x, grad_eps, B, cy, cx, H, W, h, w, r, row_of_low,
                             col_of_low, low_of_row, low_of_col, eps, scale, subtract_is_y, (hipStream_t)stream}, false, false);
}

int phl_guided_filter_full_grad(const float *y, const float *x, const float *g, float *grad_y, float *grad_x, float *grad_eps, int B,
                                int cy, int cx, int H, int W, int h, int w, int r, const int *row_of_low, const int *col_of_low,
                                const int *low_of_row, const int *low_of_col, const float *eps, float scale, int subtract_is_y,
                                phl_stream stream)
{
    return checked_backward({"phl_guided_filter_full_grad", y, x, g, nullptr, grad_y, grad_x, grad_eps, B, cy, cx, H, W, h, w, r,
                             row_of_low, col_of_low, low_of_row, low_of_col, eps, scale, subtract_is_y, (hipStream_t)stream}, false, true);
}

// (non-zero flags: PHL_ERR_UNSUPPORTED; the full covariance has the entry point below)
int phl_guided_filter_bilinear_grad(const float *y, const float *x, const float *g, float *grad_y, float *grad_x, float *grad_eps,
                                    int B, int cy, int cx, int H, int W, int h, int w, int r, const float *eps, float scale,
                                    int subtract_is_y, unsigned flags, phl_stream stream)
{
    return checked_backward({"phl_guided_filter_bilinear_grad", y, x, g, nullptr, grad_y, grad_x, grad_eps, B, cy, cx, H, W, h, w, r,
                             nullptr, nullptr, nullptr, nullptr, eps, scale, subtract_is_y, (hipStream_t)stream}, true, false, flags);
}

int phl_guided_filter_bilinear_full_grad(const float *y, const float *x, const float *g, float *grad_y, float *grad_x, float *grad_eps,
                                         int B, int cy, int cx, int H, int W, int h, int w, int r, const float *eps, float scale,
                                         int subtract_is_y, phl_stream stream)
{
    return checked_backward({"phl_guided_filter_bilinear_full_grad", y, x, g, nullptr, grad_y, grad_x, grad_eps, B, cy, cx, H, W, h, w,
                             r, nullptr, nullptr, nullptr, nullptr, eps, scale, subtract_is_y, (hipStream_t)stream}, true, true);
}

}  // extern "C"
