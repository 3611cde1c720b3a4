// phl_costvol_nchw.hip -- the stereo cost volume in the layout the channel-major consumers read
// (CRFasRNN's default W, phl_nchw_softmax_compat, phl_nchw_expected_value: logits [B][L][H][W]), and the
// winner-takes-all disparity of the same sweep without the volume.
//
// Reference: crf/depth.py:31-34 (disparity_estimate = argmin over the last axis of disparity_badness) and
// crf/dataloader.py:54-57,83 (planar_sweep_algorithm: logits = -1 * disparity_badness, permuted to [L, H, W]).
// The mathematics and the staging are phl_costvol_common.h's.
//
// One workgroup (512 threads) makes a TY x TX = 8 x 64 pixel tile for DC = 8 consecutive disparities:
//   0. the image rows it needs go to LDS as zero-padded float4 pixels, read through the caller's element strides;
//   1. raw costs: a thread owns one staged (row, column) and its 8 disparities -> craw[row][k][column];
//   2. horizontal window sums: a thread owns one (row, k) and 8 adjacent columns, a running sum in registers that is
//      restarted every 8 columns -> hs[row][k][x] (over the dead image stage);
//   3. vertical window sums: a thread owns one (k, 4 adjacent columns), a running float4 sum down the tile's 8 rows.
// Step 3 hands each float4 to the caller's sink: k_cost_volume_nchw stores it (16 lanes x 16 bytes = 256 contiguous
// bytes of one (k, y) row, four such rows per wave instruction), k_disparity_wta folds it into a per-thread running
// (min, argmin) and walks all disparity blocks of its tile; both run the same device function, so the second is the
// argmin of the first bit for bit.
#include "phl_costvol_common.h"

namespace {

constexpr int TX = PHL_COSTVOL_NCHW_TX, TY = PHL_COSTVOL_NCHW_TY, DC = PHL_COSTVOL_NCHW_DC;
constexpr int NT = 512, SEG = 8;                // SEG: columns per horizontal running sum
constexpr int HS = TX + 4;                      // row stride of hs in floats: 16-byte rows, 4 banks apart
static_assert(TX % SEG == 0 && SEG % 4 == 0 && TX % 4 == 0 && (TX / 4) * DC <= NT && TX * TY <= NT, "thread maps");

template <int R>
struct geo {
    static constexpr int ROWS = TY + 2 * R, COLS = TX + 2 * R, W2 = COLS + DC;
    static constexpr int NQ = (SEG + 2 * R + 3) / 4;            // float4 loads of one segment's raw costs
    static constexpr int CS = TX - SEG + 4 * NQ;                // row stride of craw: the last segment's loads stay inside
    static constexpr size_t stage_bytes = sizeof(float4) * (size_t)ROWS * (COLS + W2);
    static constexpr size_t hs_bytes = sizeof(float) * (size_t)ROWS * DC * HS;
    static constexpr size_t a_bytes = stage_bytes > hs_bytes ? stage_bytes : hs_bytes;
    static constexpr size_t craw_bytes = sizeof(float) * (size_t)ROWS * DC * CS;
    static constexpr size_t lds_bytes = a_bytes + craw_bytes + sizeof(int) * COLS;
    static_assert(CS >= COLS && CS % 4 == 0, "craw rows");
    static_assert(lds_bytes <= 160 * 1024, "LDS of one workgroup");
    static_assert(lds_bytes >= 2 * sizeof(float) * DC * TY * TX, "the WTA's final exchange lies over the tile's LDS");
};

__device__ __forceinline__ float4 add_sub(float4 s, float4 in, float4 out)
{
    return make_float4(s.x + in.x - out.x, s.y + in.y - out.y, s.z + in.z - out.z, s.w + in.w - out.w);
}

// The window sums of tile (x0, y0) of image pair `b` for disparities d0 .. d0+DC-1.  sink(k, xq, oy, s): the four sums
// of row y0 + oy, columns x0 + 4*xq .. +3, disparity d0 + k; called by threads 0 .. (TX/4)*DC-1 for every oy < TY,
// inside the image or not.  Ends with a barrier: the LDS may be staged again.
template <int R, int CRIT, typename Sink>
__device__ __forceinline__ void tile_window_sums(float *lds, const images &im, int b, int x0, int y0, int d0, Sink &&sink)
{
    using G = geo<R>;
    constexpr int ROWS = G::ROWS, COLS = G::COLS, W2 = G::W2, CS = G::CS;
    float4 *i1s = reinterpret_cast<float4 *>(lds);                // [ROWS][COLS] img1 pixel at reflected (row, col)
    float4 *i2s = i1s + ROWS * COLS;                              // [ROWS][W2]   img2 pixel, actual columns base2 .., 0 left of the image
    float *hs = lds;                                              // [ROWS][DC][HS] horizontal sums, over the two above
    float *craw = lds + G::a_bytes / sizeof(float);               // [ROWS][DC][CS] raw costs
    int *xr = reinterpret_cast<int *>(craw + ROWS * DC * CS);     // [COLS] reflected column as index into a row of i2s
    stage_images<R, TX, TY, DC, NT>(im, b, x0, y0, d0, i1s, i2s, xr);
    // 1: raw costs, lanes along the staged columns
    for (int e = threadIdx.x; e < ROWS * COLS; e += NT) {
        const int rr = e / COLS, xx = e - rr * COLS;
        const float4 a = i1s[e];
        const float4 *brow = i2s + rr * W2 + xr[xx];
        float *c = craw + rr * DC * CS + xx;
#pragma unroll
        for (int k = 0; k < DC; k++) c[k * CS] = raw_cost<CRIT>(a, brow[-k]);
    }
    __syncthreads();
    // 2: horizontal running sums of SEG columns each (the image stage is dead: hs lies over it)
    for (int e = threadIdx.x; e < ROWS * DC * (TX / SEG); e += NT) {
        const int rk = e / (TX / SEG), seg = e - rk * (TX / SEG);
        float c[4 * G::NQ];
        const float4 *src = reinterpret_cast<const float4 *>(craw + rk * CS + seg * SEG);
#pragma unroll
        for (int q = 0; q < G::NQ; q++) {
            const float4 v = src[q];
            c[4 * q] = v.x, c[4 * q + 1] = v.y, c[4 * q + 2] = v.z, c[4 * q + 3] = v.w;
        }
        float o[SEG];
        float s = c[0];
#pragma unroll
        for (int t = 1; t <= 2 * R; t++) s += c[t];
        o[0] = s;
#pragma unroll
        for (int x = 1; x < SEG; x++) {
            s = s + c[x + 2 * R] - c[x - 1];
            o[x] = s;
        }
        float4 *dst = reinterpret_cast<float4 *>(hs + rk * HS + seg * SEG);
#pragma unroll
        for (int q = 0; q < SEG / 4; q++) dst[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
    __syncthreads();
    // 3: vertical running sums, four columns per thread
    if (threadIdx.x < (TX / 4) * DC) {
        const int xq = threadIdx.x % (TX / 4), k = threadIdx.x / (TX / 4);
        const float4 *col = reinterpret_cast<const float4 *>(hs + k * HS) + xq;
        constexpr int RS = DC * HS / 4;                           // one staged row down, in float4
        float4 s = col[0];
#pragma unroll
        for (int t = 1; t <= 2 * R; t++) {
            const float4 v = col[t * RS];
            s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
        }
        sink(k, xq, 0, s);
#pragma unroll
        for (int oy = 1; oy < TY; oy++) {
            s = add_sub(s, col[(oy + 2 * R) * RS], col[(oy - 1) * RS]);
            sink(k, xq, oy, s);
        }
    }
    __syncthreads();
}

template <int R, int CRIT>
__global__ __launch_bounds__(NT) void k_cost_volume_nchw(images im, int L, int tiles_x, int tiles_y, int dblocks, int negate,
                                                         float *__restrict__ out, int64_t out_bs, int64_t out_ls, int64_t out_ys)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    t /= tiles_y;
    const int db = t % dblocks, b = t / dblocks;
    const int x0 = tx * TX, y0 = ty * TY, d0 = db * DC;
    tile_window_sums<R, CRIT>(lds, im, b, x0, y0, d0, [&](int k, int xq, int oy, float4 s) {
        const int gk = d0 + k, gy = y0 + oy, gx = x0 + 4 * xq;
        if (gk >= L || gy >= im.h || gx >= im.w) return;
        if (negate) s = make_float4(-s.x, -s.y, -s.z, -s.w);      // (a cost of exactly 0 becomes -0.0, as -1 * 0.0 does)
        float *p = out + b * out_bs + gk * out_ls + gy * out_ys + gx;
        if (gx + 3 < im.w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            *reinterpret_cast<float4 *>(p) = s;                   // 16 lanes: 256 contiguous bytes of row (gk, gy)
        } else {                                                  // a row off the 16-byte grid, or the image's last columns
            p[0] = s.x;
            if (gx + 1 < im.w) p[1] = s.y;
            if (gx + 2 < im.w) p[2] = s.z;
            if (gx + 3 < im.w) p[3] = s.w;
        }
    });
}

template <int R, int CRIT>
__global__ __launch_bounds__(NT) void k_disparity_wta(images im, int L, int tiles_x, int tiles_y, int32_t *__restrict__ disp,
                                                      float *__restrict__ cost, int64_t o_bs, int64_t o_ys)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int x0 = tx * TX, y0 = ty * TY;
    // thread (k, xq) of step 3 keeps the minimum over its disparities k, k + DC, k + 2 DC, ... : strict < on increasing
    // disparity, so the smallest of equal costs stays
    float best[TY][4];
    int arg[TY][4];
#pragma unroll
    for (int oy = 0; oy < TY; oy++)
#pragma unroll
        for (int j = 0; j < 4; j++) best[oy][j] = INFINITY, arg[oy][j] = 0;
    for (int d0 = 0; d0 < L; d0 += DC) {
        tile_window_sums<R, CRIT>(lds, im, b, x0, y0, d0, [&](int k, int, int oy, float4 s) {
            const int gk = d0 + k;
            if (gk >= L) return;
            const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
            for (int j = 0; j < 4; j++)             // (oy is a constant once step 3 is unrolled: the arrays stay in registers)
                if (v[j] < best[oy][j]) best[oy][j] = v[j], arg[oy][j] = gk;
        });
    }
    // the DC partial minima of a pixel meet in LDS (the last tile_window_sums ended with a barrier)
    float *rc = lds;                                  // [DC][TY][TX]
    int *ri = reinterpret_cast<int *>(lds + DC * TY * TX);
    if (threadIdx.x < (TX / 4) * DC) {
        const int xq = threadIdx.x % (TX / 4), k = threadIdx.x / (TX / 4);
#pragma unroll
        for (int oy = 0; oy < TY; oy++) {
            const int at = (k * TY + oy) * TX + 4 * xq;
            *reinterpret_cast<float4 *>(rc + at) = make_float4(best[oy][0], best[oy][1], best[oy][2], best[oy][3]);
            *reinterpret_cast<int4 *>(ri + at) = make_int4(arg[oy][0], arg[oy][1], arg[oy][2], arg[oy][3]);
        }
    }
    __syncthreads();
    if (threadIdx.x < TX * TY) {
        const int x = threadIdx.x % TX, oy = threadIdx.x / TX;
        const int gx = x0 + x, gy = y0 + oy;
        if (gx < im.w && gy < im.h) {
            float m = rc[oy * TX + x];
            int a = ri[oy * TX + x];
#pragma unroll
            for (int k = 1; k < DC; k++) {
                const float c = rc[(k * TY + oy) * TX + x];
                const int i = ri[(k * TY + oy) * TX + x];
                if (c < m || (c == m && i < a)) m = c, a = i;     // equal costs: the smaller disparity, as np.argmin
            }
            const int64_t at = b * o_bs + gy * o_ys + gx;         // 64 lanes: 256 contiguous bytes of row gy
            disp[at] = a;
            if (cost) cost[at] = m;
        }
    }
}

struct request {
    images im;
    int batch, L;
    unsigned flags;
    float *out;
    int64_t out_bs, out_ls, out_ys;
    int32_t *disp;
    float *cost;
    int tiles_x, tiles_y, dblocks, grid;
};

template <int R, int CRIT>
int launch(const request &q, hipStream_t st)
{
    constexpr size_t lds = geo<R>::lds_bytes;
    if (q.disp) {
        if (const int rc = phl_allow_lds(k_disparity_wta<R, CRIT>, lds)) return rc;
        k_disparity_wta<R, CRIT><<<dim3((unsigned)q.grid), dim3(NT), lds, st>>>(q.im, q.L, q.tiles_x, q.tiles_y, q.disp, q.cost,
                                                                                 q.out_bs, q.out_ys);
    } else {
        if (const int rc = phl_allow_lds(k_cost_volume_nchw<R, CRIT>, lds)) return rc;
        k_cost_volume_nchw<R, CRIT><<<dim3((unsigned)q.grid), dim3(NT), lds, st>>>(
            q.im, q.L, q.tiles_x, q.tiles_y, q.dblocks, (q.flags & PHL_COSTVOL_NEGATE) != 0, q.out, q.out_bs, q.out_ls, q.out_ys);
    }
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

typedef __int128 wide;
const wide I64_MAX = (wide)INT64_MAX;
constexpr int INDEX_MAX = (1 << 30) - 128;      // h, w, max_disp: reflect() doubles a length, a tile reaches TX + 16 past it

wide mag(int64_t v) { return v < 0 ? -(wide)v : (wide)v; }

// byte range [lo, hi) that an image of these strides spans around its base address
void image_span(const request &q, wide &lo, wide &hi)
{
    const int64_t ext[4] = {q.batch - 1, q.im.h - 1, q.im.w - 1, q.im.C - 1}, str[4] = {q.im.bs, q.im.ys, q.im.xs, q.im.cs};
    lo = 0, hi = 0;
    for (int i = 0; i < 4; i++) (str[i] < 0 ? lo : hi) += (wide)ext[i] * str[i];
    lo *= 4, hi = hi * 4 + 4;
}

bool overlaps(const void *p, wide bytes, const void *img, wide lo, wide hi)
{
    const wide a = (wide)(uintptr_t)p, b = (wide)(uintptr_t)img;
    return a < b + hi && b + lo < a + bytes;
}

// The argument checks of both entry points, all before the first HIP call.  PHL_OK with q.grid == 0: nothing to launch.
int check(const char *name, request &q, int window, int criterion, bool wta)
{
    const images &im = q.im;
    if (const int rc = check_supported(name, im.C, window, criterion)) return rc;
    if (q.flags & ~PHL_COSTVOL_NEGATE) {
        phl_set_error("%s: supports flags within PHL_COSTVOL_NEGATE; got flags=%#x", name, q.flags);
        return PHL_ERR_UNSUPPORTED;
    }
    q.grid = 0;
    if (q.batch < 0 || im.h < 0 || im.w < 0 || q.L < 0) {
        phl_set_error("%s: negative size (batch=%d h=%d w=%d max_disp=%d)", name, q.batch, im.h, im.w, q.L);
        return PHL_ERR_INVALID;
    }
    if (wta && q.L == 0) {
        phl_set_error("%s: max_disp = 0, an argmin over nothing", name);
        return PHL_ERR_INVALID;
    }
    if (q.batch == 0 || im.h == 0 || im.w == 0 || q.L == 0) return PHL_OK;
    if (!im.img1 || !im.img2 || (wta ? !q.disp : !q.out)) {
        phl_set_error("%s: NULL image or output", name);
        return PHL_ERR_INVALID;
    }
    // what one output row, plane and item span, in elements (x stride 1)
    const wide rows = (wide)(im.h - 1) * mag(q.out_ys) + im.w;
    const wide item = wta ? rows : (wide)(q.L - 1) * mag(q.out_ls) + rows;
    if (q.out_ys < im.w || (!wta && q.out_ls < rows) || (q.batch > 1 && q.out_bs < item)) {
        phl_set_error("%s: output strides smaller than what they step over (rows of %d, %d rows%s): rows would overlap", name,
                      im.w, im.h, wta ? "" : ", max_disp planes");
        return PHL_ERR_INVALID;
    }
    const wide out_elems = (wide)(q.batch - 1) * mag(q.out_bs) + item;
    wide lo, hi;
    image_span(q, lo, hi);
    const void *outs[3] = {q.out, q.disp, q.cost};
    for (const void *o : outs)
        if (o && (overlaps(o, out_elems * 4, im.img1, lo, hi) || overlaps(o, out_elems * 4, im.img2, lo, hi))) {
            phl_set_error("%s: an output lies inside an image", name);
            return PHL_ERR_INVALID;
        }
    if (q.cost && overlaps(q.cost, out_elems * 4, q.disp, 0, out_elems * 4)) {
        phl_set_error("%s: cost_dev overlaps disp_dev", name);
        return PHL_ERR_INVALID;
    }
    q.tiles_x = (im.w - 1) / TX + 1, q.tiles_y = (im.h - 1) / TY + 1, q.dblocks = (q.L - 1) / DC + 1;
    const wide grid = (wide)q.tiles_x * q.tiles_y * q.batch * (wta ? 1 : q.dblocks);
    if (out_elems * 4 > I64_MAX || hi > I64_MAX || -lo > I64_MAX || grid > INT32_MAX || q.L > INDEX_MAX ||
        im.w > INDEX_MAX || im.h > INDEX_MAX) {
        phl_set_error("%s: too large (the byte offsets leave int64 or the %d x %d x %d tiles leave a grid of 2^31 - 1)", name, TX,
                      TY, DC);
        return PHL_ERR_TOO_LARGE;
    }
    q.grid = (int)grid;
    return PHL_OK;
}

// checks, then launches what they left to launch
int run(const char *name, request &q, int window, int criterion, bool wta, phl_stream stream)
{
    if (const int rc = check(name, q, window, criterion, wta)) return rc;
    if (!q.grid) return PHL_OK;
    return dispatch(window, criterion, [&](auto r, auto c) { return launch<decltype(r)::value, decltype(c)::value>(q, (hipStream_t)stream); });
}

}  // namespace

extern "C" int phl_cost_volume_nchw(const float *img1, const float *img2, int batch, int h, int w, int channels, int64_t img_bs,
                                    int64_t img_ys, int64_t img_xs, int64_t img_cs, int max_disp, int window, int criterion,
                                    unsigned flags, float *out, int64_t out_bs, int64_t out_ls, int64_t out_ys, phl_stream stream)
{
    request q = {{img1, img2, img_bs, img_ys, img_xs, img_cs, h, w, channels}, batch, max_disp, flags, out, out_bs, out_ls, out_ys,
                 nullptr, nullptr, 0, 0, 0, 0};
    return run("phl_cost_volume_nchw", q, window, criterion, false, stream);
}

extern "C" int phl_disparity_wta(const float *img1, const float *img2, int batch, int h, int w, int channels, int64_t img_bs,
                                 int64_t img_ys, int64_t img_xs, int64_t img_cs, int max_disp, int window, int criterion,
                                 int32_t *disp, float *cost, int64_t o_bs, int64_t o_ys, phl_stream stream)
{
    request q = {{img1, img2, img_bs, img_ys, img_xs, img_cs, h, w, channels}, batch, max_disp, 0u, nullptr, o_bs, 0, o_ys,
                 disp, cost, 0, 0, 0, 0};
    return run("phl_disparity_wta", q, window, criterion, true, stream);
}
