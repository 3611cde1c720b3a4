// What the channel-major ([B][L][n], n = H * W) translation units share: phl_nchw.hip (the mean-field step),
// phl_nchw_expect.hip (the expected label), phl_nchw_scalar.hip (the upsampler head's unaries) and phl_nchw_conf.hip (the
// unaries from logits and a confidence).  Internal: everything sits in an anonymous namespace, so each translation unit
// gets its own copy.
//
// The pixel layout of the streaming kernels (every kernel of the last three files): a workgroup of NT = 256 threads owns
// WGP = 1024 consecutive pixels of one image -- tile t of the ceil(n / WGP) tiles of image b is workgroup b * tiles + t --
// and a thread owns PX = 4 of them, which it walks through the L planes.
//   VEC   n % 4 == 0 and every pointer 16-byte aligned: the pixels are 4 t .. 4 t + 3 of the tile, one float4 per plane,
//         which lies inside the image or outside
//   else  the pixels are t, t + 256, t + 512, t + 768, one dword each: a wave still reads 256 contiguous bytes per plane
// k_nchw_tile's 64-pixel LDS tile (phl_nchw.hip) is another layout; that file shares the host side only, and so does
// phl_nchw_train.hip (the training step and its backward, the same tile with Q in float64).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <initializer_list>
#include <type_traits>

#include "phl_internal.h"

namespace {

constexpr int NT = 256;                // threads of a workgroup
constexpr int PX = 4;                  // pixels of a thread
constexpr int WGP = NT * PX;           // pixels of a workgroup
static_assert(WGP == PHL_NCHW_EXPECT_PIXELS && WGP == PHL_NCHW_SCALAR_PIXELS, "include/phl.h documents the workgroup's pixel count");

// The thread's place in workgroup-sized tile blk of the B * tiles: b = its image, q = its first pixel, ok[j] = pixel j
// lies inside the image; false: the thread has no pixel.
template <bool VEC>
__device__ __forceinline__ bool thread_pixels(int64_t n, int tiles, unsigned blk, int &b, int64_t &q, bool (&ok)[PX])
{
    b = blk / tiles;
    const int tile = blk - b * tiles;
    q = (int64_t)tile * WGP + (VEC ? PX * (int)threadIdx.x : (int)threadIdx.x);
#pragma unroll
    for (int j = 0; j < PX; j++) ok[j] = VEC ? q < n : q + j * NT < n;      // VEC: n % 4 == 0
    return ok[0];
}

// The thread's four pixels of one plane, p = the address of the first.  VEC: one float4, unguarded (thread_pixels said
// that the thread has a pixel).  Dwords: a pixel outside the image loads as 0.f and is not stored.
template <bool VEC>
__device__ __forceinline__ void load_px(const float *p, const bool (&ok)[PX], float (&v)[PX])
{
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < PX; j++) v[j] = ok[j] ? p[j * NT] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_px(float *p, const bool (&ok)[PX], const float (&v)[PX])
{
    if (VEC) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < PX; j++)
            if (ok[j]) p[j * NT] = v[j];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// tiles of px pixels in an image of n, and the grid of one workgroup per tile and image
inline int nchw_tiles(int64_t n, int px = WGP) { return (int)((n + px - 1) / px); }
inline dim3 nchw_grid(int B, int tiles) { return dim3((unsigned)((int64_t)B * tiles)); }

// float4 accesses along the pixel axis: n % 4 == 0 and every pointer 16-byte aligned (null counts as aligned)
inline bool nchw_vec(int64_t n, std::initializer_list<const void *> ptrs)
{
    bool vec = n % 4 == 0;
    for (const void *p : ptrs) vec = vec && phl_al16(p);
    return vec;
}

// B * L * n * 4 bytes leave int64, or the workgroups of px pixels leave the grid (px = 0: the grid does not grow with
// the image).  B, L >= 1 and <= 2^31 - 1: their product stays in int64.
inline bool nchw_too_large(int B, int L, int64_t n, int px)
{
    return n > (INT64_MAX / 4) / ((int64_t)B * L) || (px && (n + px - 1) / px > INT32_MAX / (int64_t)B);
}

// f(std::bool_constant<VEC>(), std::bool_constant<HASG>()) for the run-time pair, and what it returns.  A kernel without
// the second parameter passes false and ignores it.
template <class F>
auto nchw_dispatch(bool vec, bool has_g, F &&f)
{
    using std::false_type;
    using std::true_type;
    if (vec && has_g) return f(true_type(), true_type());
    if (vec) return f(true_type(), false_type());
    if (has_g) return f(false_type(), true_type());
    return f(false_type(), false_type());
}

// printf into a buffer that lives to the end of the caller's statement: the `sizes` text of nchw_check
struct nchw_text {
    char s[128];
    __attribute__((format(printf, 2, 3))) nchw_text(const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(s, sizeof s, fmt, ap);
        va_end(ap);
    }
};

// The argument checks of an entry point, in the order include/phl.h states: the sizes (`bad`, evaluated by the caller;
// `sizes` is their text for the messages), zero elements (`empty`: PHL_OK whatever the pointers), a null among
// `required` (`required_names` for the message), `result` being one of `inputs` (nulls among them are harmless), too
// many elements.  true: there is nothing to launch and the entry point returns status.
inline bool nchw_check(const char *who, const char *sizes, bool bad, bool empty, std::initializer_list<const void *> required,
                       const char *required_names, std::initializer_list<const void *> inputs, const void *result,
                       const char *result_name, int B, int L, int64_t n, int px, int &status)
{
    bool null = false, alias = false;
    for (const void *p : required) null = null || !p;
    for (const void *p : inputs) alias = alias || p == result;
    status = PHL_ERR_INVALID;
    if (bad) phl_set_error("%s: bad arguments (%s)", who, sizes);
    else if (empty) status = PHL_OK;
    else if (null) phl_set_error("%s: null %s", who, required_names);
    else if (alias) phl_set_error("%s: %s aliases an input", who, result_name);
    else if (nchw_too_large(B, L, n, px)) {
        phl_set_error("%s: too many elements (%s)", who, sizes);
        status = PHL_ERR_TOO_LARGE;
    } else status = PHL_OK;
    return empty || status != PHL_OK;
}

}  // namespace
