// phl_costvol.hip -- the unary cost volume E_0 of the stereo CRF, produced on the device in the layout the lattice
// filter reads (pixel-major [h*w][L] fp32).  The mathematics and the staging are phl_costvol_common.h's.
//
// One workgroup makes a TY x TX pixel tile for DC consecutive disparities: the image rows it needs go to LDS once,
// every thread then owns one (row, disparity) and forms the horizontal window sums in registers, the vertical sums are
// read back from LDS, and a wavefront stores 128 contiguous bytes per pixel.
#include "phl_costvol_common.h"

namespace {

constexpr int TX = 16, TY = 16, DC = 32;   // threads = (TY + 2R) rows x DC disparities

template <int R, int CRIT>
__global__ __launch_bounds__((TY + 2 * R) * DC) void k_cost_volume(const float *__restrict__ img1, const float *__restrict__ img2, int h,
                                                                   int w, int C, int L, float *__restrict__ out, int64_t out_rs)
{
    constexpr int ROWS = TY + 2 * R, COLS = TX + 2 * R, W2 = COLS + DC;   // staged extents
    constexpr int NT = ROWS * DC;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float4 *i1s = reinterpret_cast<float4 *>(lds);    // [ROWS][COLS]  img1 pixel (<= 4 channels) at reflected (row, col)
    float4 *i2s = i1s + ROWS * COLS;                  // [ROWS][W2]    img2 pixel, actual columns base2 .. base2+W2-1, 0 left of the image
    float *hs = reinterpret_cast<float *>(i2s + ROWS * W2);      // [ROWS][TX][DC]    horizontal window sums
    int *xr = reinterpret_cast<int *>(hs + ROWS * TX * DC);      // [COLS] reflected column of each tile column, as index into a row of i2s
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, d0 = blockIdx.z * DC;
    const images im = {img1, img2, 0, (int64_t)w * C, C, 1, h, w, C};       // dense [h][w][C]
    stage_images<R, TX, TY, DC, NT>(im, 0, x0, y0, d0, i1s, i2s, xr);
    // phase 1: thread = (row, disparity); cost of the row's COLS columns -> horizontal running window sums
    {
        const int k = threadIdx.x % DC, rr = threadIdx.x / DC;
        float c[COLS];
        const float4 *arow = i1s + rr * COLS;
        const float4 *brow = i2s + rr * W2 - k;
#pragma unroll
        for (int xx = 0; xx < COLS; xx++) c[xx] = raw_cost<CRIT>(arow[xx], brow[xr[xx]]);
        float s = c[0];
#pragma unroll
        for (int t = 1; t <= 2 * R; t++) s += c[t];
        hs[(rr * TX + 0) * DC + k] = s;
#pragma unroll
        for (int x = 1; x < TX; x++) {
            s = s + c[x + 2 * R] - c[x - 1];
            hs[(rr * TX + x) * DC + k] = s;
        }
    }
    __syncthreads();
    // phase 2: thread = (column, disparity); vertical running window sums, 128 contiguous bytes per pixel per wave half
    if (threadIdx.x < TX * DC) {
        const int k = threadIdx.x % DC, x = threadIdx.x / DC;
        const int gx = x0 + x, gk = d0 + k;
        if (gx < w && gk < L) {
            float s = hs[(0 * TX + x) * DC + k];
#pragma unroll
            for (int t = 1; t <= 2 * R; t++) s += hs[(t * TX + x) * DC + k];
            out[((int64_t)y0 * w + gx) * out_rs + gk] = s;
            for (int oy = 1; oy < TY && y0 + oy < h; oy++) {
                s = s + hs[((oy + 2 * R) * TX + x) * DC + k] - hs[((oy - 1) * TX + x) * DC + k];
                out[((int64_t)(y0 + oy) * w + gx) * out_rs + gk] = s;
            }
        }
    }
}

}  // namespace

extern "C" int phl_cost_volume(const float *img1, const float *img2, int h, int w, int channels, int max_disp, int window,
                               int criterion, float *out, int64_t out_rs, phl_stream stream)
{
    if (const int rc = check_supported("phl_cost_volume", channels, window, criterion)) return rc;
    if (h < 1 || w < 1 || max_disp < 0 || !img1 || !img2 || (max_disp > 0 && !out) || out_rs < max_disp) {
        phl_set_error("phl_cost_volume: bad arguments");
        return PHL_ERR_INVALID;
    }
    if (max_disp == 0) return PHL_OK;
    return dispatch(window, criterion, [&](auto r, auto c) -> int {
        constexpr int R = decltype(r)::value, CRIT = decltype(c)::value, ROWS = TY + 2 * R, COLS = TX + 2 * R, W2 = COLS + DC;
        const size_t lds = sizeof(float) * (4 * (size_t)ROWS * COLS + 4 * (size_t)ROWS * W2 + COLS + (size_t)ROWS * TX * DC);
        if (const int rc = phl_allow_lds(k_cost_volume<R, CRIT>, lds)) return rc;
        const dim3 grid((unsigned)((w + TX - 1) / TX), (unsigned)((h + TY - 1) / TY), (unsigned)((max_disp + DC - 1) / DC));
        k_cost_volume<R, CRIT><<<grid, dim3(ROWS * DC), lds, (hipStream_t)stream>>>(img1, img2, h, w, channels, max_disp, out, out_rs);
        PHL_HIP(hipGetLastError());
        return PHL_OK;
    });
}
