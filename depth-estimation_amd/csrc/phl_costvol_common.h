// What the stereo sweep's kernels share (phl_costvol.hip: k_cost_volume, pixel-major [h*w][L]; phl_costvol_nchw.hip:
// k_cost_volume_nchw and k_disparity_wta, channel-major [B][L][H][W]).  Internal: everything sits in an anonymous
// namespace, so each translation unit gets its own copy.
//
// Reference (numpy + scipy on the CPU): crf/depth.py:36-53
//   disparity_badness(img1, img2, window_size, criterion):
//     cost[y,x,k] = sum_ch criterion(img1[y,x,ch], img2[y,x-k,ch])      img2 zero for x-k < 0  (:45-50)
//     out[y,x,k]  = sum over the ws x ws window of cost[.,.,k]           (:51-52)
//   with scipy.ndimage's default border rule 'reflect' (d c b a | a b c d | d c b a) on the COST array, not the images.
// criterion: AD |a-b| (:26-27), SD (a-b)^2 (:24-25), nprod -a*b (:28-29).
//
// Every kernel stages the image rows of its tile in LDS once (stage_images), forms the raw costs from them and then
// separable RUNNING window sums, restarted every tile: a window enters with one add and leaves with one subtract, the
// add before the subtract, ~4 adds per output instead of ws^2.  The kernels' only HBM traffic of size is the result;
// they are VALU-bound (the raw costs).  Tile shapes, LDS layouts and the thread maps of the sums differ per layout and
// are described in each file.
#pragma once
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "phl_internal.h"

namespace {

constexpr int CMAX = 4;         // channels of a staged pixel (one float4)

struct images {
    const float *img1, *img2;
    int64_t bs, ys, xs, cs;     // element strides: batch, row, column, channel (the same for both images)
    int h, w, C;
};

__device__ __forceinline__ int reflect(int i, int n)
{
    // scipy 'reflect': -1 -> 0, -2 -> 1, n -> n-1, n+1 -> n-2 (period 2n)
    if (i >= 0 && i < n) return i;
    if (i < 0 && i >= -n) return -i - 1;          // one fold: the common border case, no division
    if (i >= n && i < 2 * n) return 2 * n - 1 - i;
    const int p = 2 * n;                          // windows larger than the image
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

__device__ __forceinline__ float4 ld_pixel(const float *p, int64_t cs, int C)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // channels padded with zeros: every criterion gives 0 on (0, 0)
    v.x = p[0];
    if (C > 1) v.y = p[cs];
    if (C > 2) v.z = p[2 * cs];
    if (C > 3) v.w = p[3 * cs];
    return v;
}

template <int CRIT> __device__ __forceinline__ float crit(float a, float b);
template <> __device__ __forceinline__ float crit<0>(float a, float b) { return fabsf(a - b); }
template <> __device__ __forceinline__ float crit<1>(float a, float b) { return (a - b) * (a - b); }
template <> __device__ __forceinline__ float crit<2>(float a, float b) { return -1.0f * a * b; }

template <int CRIT>
__device__ __forceinline__ float raw_cost(float4 a, float4 b)
{
    return ((crit<CRIT>(a.x, b.x) + crit<CRIT>(a.y, b.y)) + crit<CRIT>(a.z, b.z)) + crit<CRIT>(a.w, b.w);
}

// Step 0 of every kernel: what the TY x TX pixel tile at (x0, y0) of image pair `b` reads for window radius R and
// disparities d0 .. d0+DC-1, that is ROWS x COLS = (TY + 2R) x (TX + 2R) staged pixels, by the workgroup's NT threads.
//   i1s [ROWS][COLS]       img1 pixel at the reflected (row, column)
//   i2s [ROWS][COLS + DC]  img2 pixel at the reflected row, actual columns base2 .. base2+COLS+DC-1, 0 outside the image
//   xr  [COLS]             column xx at disparity d0 + k pairs with i2s[row][xr[xx] - k]
// Ends with a barrier.
template <int R, int TX, int TY, int DC, int NT>
__device__ __forceinline__ void stage_images(const images &im, int b, int x0, int y0, int d0, float4 *i1s, float4 *i2s, int *xr)
{
    constexpr int ROWS = TY + 2 * R, COLS = TX + 2 * R, W2 = COLS + DC;
    const int h = im.h, w = im.w, C = im.C;
    const float *img1 = im.img1 + b * im.bs, *img2 = im.img2 + b * im.bs;
    // the tile's reflected columns fall on a contiguous range of actual columns, at most COLS wide
    int cmin = w;
    for (int xx = 0; xx < COLS; xx++) cmin = min(cmin, reflect(x0 - R + xx, w));         // tiny, uniform over the workgroup
    const int base2 = cmin - (d0 + DC - 1);           // leftmost img2 column any (column, disparity) pair reads
    for (int xx = threadIdx.x; xx < COLS; xx += NT) xr[xx] = reflect(x0 - R + xx, w) - d0 - base2;
    for (int e = threadIdx.x; e < ROWS * COLS; e += NT) {
        const int rr = e / COLS, xx = e - rr * COLS;
        const int y = reflect(y0 - R + rr, h), x = reflect(x0 - R + xx, w);
        i1s[e] = ld_pixel(img1 + y * im.ys + x * im.xs, im.cs, C);
    }
    for (int e = threadIdx.x; e < ROWS * W2; e += NT) {
        const int rr = e / W2, cc = e - rr * W2;
        const int y = reflect(y0 - R + rr, h), x = base2 + cc;
        i2s[e] = (x >= 0 && x < w) ? ld_pixel(img2 + y * im.ys + x * im.xs, im.cs, C) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
}

// The supported set of all three entry points, checked before anything else: an image without channels has no data, and
// its NULL pointer is not the caller's mistake.
inline int check_supported(const char *name, int channels, int window, int criterion)
{
    if (channels >= 1 && channels <= CMAX && window >= 1 && window % 2 == 1 && window <= 17 && criterion >= 0 && criterion <= 2)
        return PHL_OK;
    phl_set_error("%s: supports 1..%d channels, odd windows up to 17, criterion 0 (AD) / 1 (SD) / 2 (nprod); got c=%d ws=%d crit=%d",
                  name, CMAX, channels, window, criterion);
    return PHL_ERR_UNSUPPORTED;
}

// f(std::integral_constant<int, R>(), std::integral_constant<int, CRIT>()) for the run-time (window / 2, criterion) of
// a supported request: the kernels are instantiated for R = 0..8 by CRIT = 0..2 here and nowhere else.
template <int CRIT, class F>
int dispatch_radius(int R, F &&f)
{
    using std::integral_constant;
    constexpr integral_constant<int, CRIT> c;
    switch (R) {
        case 0: return f(integral_constant<int, 0>(), c);
        case 1: return f(integral_constant<int, 1>(), c);
        case 2: return f(integral_constant<int, 2>(), c);
        case 3: return f(integral_constant<int, 3>(), c);
        case 4: return f(integral_constant<int, 4>(), c);
        case 5: return f(integral_constant<int, 5>(), c);
        case 6: return f(integral_constant<int, 6>(), c);
        case 7: return f(integral_constant<int, 7>(), c);
        default: return f(integral_constant<int, 8>(), c);
    }
}

template <class F>
int dispatch(int window, int criterion, F &&f)
{
    switch (criterion) {
        case 0: return dispatch_radius<0>(window / 2, f);
        case 1: return dispatch_radius<1>(window / 2, f);
        default: return dispatch_radius<2>(window / 2, f);
    }
}

}  // namespace
