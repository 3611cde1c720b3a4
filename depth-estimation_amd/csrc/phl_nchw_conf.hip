// phl_nchw_conf.hip -- the unary energies of a CRFasRNN call from logits and a per-pixel confidence, and their backward.
//
// Reference (crf/crf_module.py:95-97, CRFasRNN.forward): E0 = -logits * confidence on [B, L, H, W] logits and a [B, 1, H, W]
// confidence -- a negation and a broadcast product, two passes over the volume; under autograd the temporary -logits
// lives until the backward (the confidence needs it), which then writes gE0 * (-logits) as another volume and reduces it
// over the labels in fp32.  Here
//
//     E0[b, a, p]          = -(logits[b, a, p] * conf[b, p])
//     grad_conf[b, p]      = -sum_a logits[b, a, p] * gE0[b, a, p]
//     grad_logits[b, a, p] = -(conf[b, p] * gE0[b, a, p])
//
//   k_conf_unaries        the layout of phl_nchw_common.h: a thread loads the confidences of its four pixels once and
//                         walks the L planes, BLK = 8 planes in flight.  One read of the logits, one write of E0.
//   k_conf_grad           the same walk over gE0 -- and over the logits where grad_conf is asked for, the confidences
//                         where grad_logits is.  A part that is not asked for is compiled out (NEEDC / NEEDL), so the
//                         other part's instructions, and bits, are the same with and without it.
//
// Arithmetic.  An fp32 product is correctly rounded and the negation is exact: E0 and grad_logits are the bits of torch's
// (-logits) * confidence and -(gE0 * confidence) on finite inputs, signed zeros included (-(x * y) == (-x) * y in IEEE
// arithmetic).  grad_conf: the product of two fp32 numbers is exact in float64 (48 bits), the sum runs in float64 in label
// order a = 0 .. L-1 and is rounded to fp32 once.  No LDS, no atomics, no scratch: a repeated call gives the same bits.
#include "phl_nchw_common.h"

static_assert(WGP == PHL_NCHW_CONF_PIXELS, "include/phl.h documents the workgroup's pixel count");

namespace {

constexpr int BLK = 8;                 // label planes in flight

// planes a0 .. a0 + BLK - 1 of E0; lp / op: the thread's first pixel in plane 0.  FULL: all BLK planes exist.
template <bool VEC, bool FULL>
__device__ __forceinline__ void unaries_block(const float *lp, float *op, int a0, int L, int64_t n, const bool (&ok)[PX],
                                              const float (&c)[PX])
{
    float x[BLK][PX];
#pragma unroll
    for (int i = 0; i < BLK; i++)
        if (FULL || a0 + i < L) load_px<VEC>(lp + (int64_t)(a0 + i) * n, ok, x[i]);      // (a0 + i: wave-uniform)
#pragma unroll
    for (int i = 0; i < BLK; i++) {
        if (FULL || a0 + i < L) {
            float e[PX];
#pragma unroll
            for (int j = 0; j < PX; j++) e[j] = -(x[i][j] * c[j]);
            store_px<VEC>(op + (int64_t)(a0 + i) * n, ok, e);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void k_conf_unaries(const float *__restrict__ logits, const float *__restrict__ conf,
                                                     float *__restrict__ E0, int L, int64_t n, int tiles)
{
    int b;
    int64_t q;
    bool ok[PX];
    if (!thread_pixels<VEC>(n, tiles, blockIdx.x, b, q, ok)) return;
    float c[PX];
    load_px<VEC>(conf + (int64_t)b * n + q, ok, c);
    const int64_t base = (int64_t)b * L * n + q;
    int a0 = 0;
    for (; a0 + BLK <= L; a0 += BLK) unaries_block<VEC, true>(logits + base, E0 + base, a0, L, n, ok, c);
    if (a0 < L) unaries_block<VEC, false>(logits + base, E0 + base, a0, L, n, ok, c);
}

// planes a0 .. a0 + BLK - 1 of the backward: acc[j] += logits * gE0 in float64 (NEEDC), grad_logits = -(c * gE0) (NEEDL)
template <bool VEC, bool NEEDC, bool NEEDL, bool FULL>
__device__ __forceinline__ void grad_block(const float *lp, const float *gp, float *zp, int a0, int L, int64_t n,
                                           const bool (&ok)[PX], const float (&c)[PX], double (&acc)[PX])
{
    float x[BLK][PX], g[BLK][PX];
#pragma unroll
    for (int i = 0; i < BLK; i++) {
        if (FULL || a0 + i < L) {
            const float *ga = gp + (int64_t)(a0 + i) * n;
            if (!NEEDC) {
                load_px<VEC>(ga, ok, g[i]);
            } else if (VEC) {
                load_px<VEC>(lp + (int64_t)(a0 + i) * n, ok, x[i]);
                load_px<VEC>(ga, ok, g[i]);
            } else {                                             // dwords: the two loads of a pixel under one guard
                const float *la = lp + (int64_t)(a0 + i) * n;
#pragma unroll
                for (int j = 0; j < PX; j++) {
                    x[i][j] = ok[j] ? la[j * NT] : 0.f;
                    g[i][j] = ok[j] ? ga[j * NT] : 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < BLK; i++) {
        if (FULL || a0 + i < L) {
            if (NEEDC) {
#pragma unroll
                for (int j = 0; j < PX; j++) acc[j] += (double)x[i][j] * (double)g[i][j];      // exact product, label order
            }
            if (NEEDL) {
                float z[PX];
#pragma unroll
                for (int j = 0; j < PX; j++) z[j] = -(c[j] * g[i][j]);
                store_px<VEC>(zp + (int64_t)(a0 + i) * n, ok, z);
            }
        }
    }
}

template <bool VEC, bool NEEDC, bool NEEDL>
__global__ __launch_bounds__(NT) void k_conf_grad(const float *__restrict__ logits, const float *__restrict__ conf,
                                                  const float *__restrict__ gE0, float *__restrict__ grad_conf,
                                                  float *__restrict__ grad_logits, int L, int64_t n, int tiles)
{
    int b;
    int64_t q;
    bool ok[PX];
    if (!thread_pixels<VEC>(n, tiles, blockIdx.x, b, q, ok)) return;
    float c[PX] = {0.f, 0.f, 0.f, 0.f};
    if (NEEDL) load_px<VEC>(conf + (int64_t)b * n + q, ok, c);
    double acc[PX] = {0.0, 0.0, 0.0, 0.0};
    const int64_t base = (int64_t)b * L * n + q;
    const float *lp = NEEDC ? logits + base : nullptr;
    float *zp = NEEDL ? grad_logits + base : nullptr;
    int a0 = 0;
    for (; a0 + BLK <= L; a0 += BLK) grad_block<VEC, NEEDC, NEEDL, true>(lp, gE0 + base, zp, a0, L, n, ok, c, acc);
    if (a0 < L) grad_block<VEC, NEEDC, NEEDL, false>(lp, gE0 + base, zp, a0, L, n, ok, c, acc);
    if (NEEDC) {
        float r[PX];
#pragma unroll
        for (int j = 0; j < PX; j++) r[j] = (float)-acc[j];
        store_px<VEC>(grad_conf + (int64_t)b * n + q, ok, r);
    }
}

}  // namespace

extern "C" {

int phl_nchw_confidence_unaries(const float *logits, const float *conf, float *E0, int B, int L, int64_t n, phl_stream stream)
{
    const char *who = "phl_nchw_confidence_unaries";
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0,
                   {logits, conf, E0}, "logits / conf / E0", {logits, conf}, E0, "E0", B, L, n, WGP, rc))
        return rc;
    const int tiles = nchw_tiles(n);
    nchw_dispatch(nchw_vec(n, {logits, conf, E0}), false, [&](auto vec, auto) {
        k_conf_unaries<decltype(vec)::value><<<nchw_grid(B, tiles), dim3(NT), 0, (hipStream_t)stream>>>(logits, conf, E0, L, n, tiles);
    });
    phl_launched(rc, who);
    return rc;
}

int phl_nchw_confidence_unaries_grad(const float *logits, const float *conf, const float *gE0, float *grad_conf,
                                     float *grad_logits, int B, int L, int64_t n, phl_stream stream)
{
    const char *who = "phl_nchw_confidence_unaries_grad";
    int rc;
    // two outputs through the one-result check: `first` is an output that exists (null: both are missing), and it stands
    // among the inputs where the other output clashes with an input or with it
    const float *first = grad_conf ? grad_conf : grad_logits, *second = grad_conf ? grad_logits : nullptr;
    const bool clash = second && (second == logits || second == conf || second == gE0 || second == first);
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0,
                   {logits, conf, gE0, first}, "logits / conf / gE0, or both of grad_conf and grad_logits",
                   {logits, conf, gE0, clash ? first : nullptr}, first, "grad_conf / grad_logits", B, L, n, WGP, rc))
        return rc;
    const int tiles = nchw_tiles(n);
    nchw_dispatch(nchw_vec(n, {logits, conf, gE0, grad_conf, grad_logits}), grad_conf != nullptr, [&](auto vec, auto need_c) {
        constexpr bool V = decltype(vec)::value, C = decltype(need_c)::value;
        const dim3 grid = nchw_grid(B, tiles);
        hipStream_t st = (hipStream_t)stream;
        if (!C || grad_logits) k_conf_grad<V, C, true><<<grid, dim3(NT), 0, st>>>(logits, conf, gE0, grad_conf, grad_logits, L, n, tiles);
        else k_conf_grad<V, true, false><<<grid, dim3(NT), 0, st>>>(logits, conf, gE0, grad_conf, grad_logits, L, n, tiles);
    });
    phl_launched(rc, who);
    return rc;
}

}  // extern "C"
