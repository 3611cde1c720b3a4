// phl_nchw_expect.hip -- the expected label of a channel-major column, and its backward: the end of the CRFasRNN heads.
//
// Reference (crf/mb_stereo_crf.py:62-66, logits2average_depth): probs = softmax(logits, dim=1); (probs * labels).sum(1)
// on [B, L, H, W] tensors -- a 2-3 pass softmax over a strided dimension, a broadcast product and a sum, to produce one
// plane.  Here
//
//     out[b, p] = sum_a labels[a] * softmax_a( sign * (X[b, a, p] + G[b, a, p]) )          (G optional, sign = +-1)
//
// is ONE kernel that reads X and G once and writes the plane; with sign = -1 it takes the mean-field loop's E0 and G as
// they are, so the logits of the last iteration never exist in memory either (phl_nchw.hip, k_nchw_logits).
//
//   k_nchw_expect        a thread walks the label planes of its four pixels once (the layout of phl_nchw_common.h),
//                        BLK = 8 planes in flight.  Per pixel it keeps the running maximum m, the sum s of exp(z - m)
//                        and the label-weighted sum t (online softmax): the maximum of the eight new values is taken
//                        first, s and t are rescaled by exp(m - m') where it rose -- one exp per element plus at most
//                        one per block.  m starts from the first block's maximum (no exp(-inf - -inf)).  It ends with
//                        t / s.
//   k_nchw_expect_grad   gZ[b, a, p] = sign * g[b, p] * q_a * (labels[a] - d), the gradient of X and of G alike.  Pass 1
//                        is the forward's code (m, s, d); pass 2 reads X and G again and writes gZ = exp(z - m) * (w *
//                        (labels[a] - d)), w = sign * g / s.  Nothing but the forward's inputs is needed.
//
// Arithmetic.  An online softmax subtracts another maximum than a two-pass one and multiplies exponentials: in fp32 the
// roundings of x + g, of z - m (half an ulp of up to 60 or so: 4e-6 of the term), of m - m' and of expf are as large as
// the two-pass form's, but they are others, so neither form is the more accurate one, element by element (an fp32 build
// of this file, emulated operation by operation on the CPU over the GPU test's cases, ranged from 0.3 to 3 times the fp32
// torch form's error and missed the test's factor of 2 in 2 of its 27 groups).  The kernels are expected to wait for
// memory rather than for the vector unit (f64 runs at the full vector rate on gfx950; about 30 f64 operations per 4 or 8
// bytes of traffic).  Measured at 1110 x 1390: the forward with G runs at 0.96 of the copy rate at 231 labels
// and 0.80 at 64, so there it does wait for memory; forward + backward at two thirds, not yet taken apart.  Between the
// fp32 loads and the fp32 stores everything is float64: z = x + g and z - m are exact, exp, s, t, d and the backward's exp(z - m) * w * (labels[a] - d)
// are float64, and every output is rounded to fp32 once -- the fp32 number nearest to the float64 result, which no fp32
// chain can beat.  m itself stays fp32 (any value near the maximum serves).  No LDS, no atomics, every sum in a fixed
// order: a repeated call gives the same bits.
#include <math.h>

#include "phl_nchw_common.h"

namespace {

constexpr int BLK = 8;                 // label planes in flight

// x[i][j], g[i][j] of planes a0 .. a0 + BLK - 1 and lab[i] their labels; planes beyond L are left alone.  xp / gp: the
// thread's first pixel in plane 0.  FULL: all BLK planes exist.
template <bool VEC, bool HASG, bool FULL>
__device__ __forceinline__ void load_block(const float *xp, const float *gp, const float *labels, int a0, int L, int64_t n,
                                           const bool (&ok)[PX], float (&x)[BLK][PX], float (&g)[BLK][PX], float (&lab)[BLK])
{
#pragma unroll
    for (int i = 0; i < BLK; i++) {
        const int a = a0 + i;                                    // wave-uniform
        if (FULL || a < L) {
            const float *xa = xp + (int64_t)a * n, *ga = HASG ? gp + (int64_t)a * n : nullptr;
            // dwords of x and g: load_px's by hand, the two loads of a pixel under ONE guard (as two load_px calls, each
            // guarded load in a branch of its own, these kernels took 1.33 times as long)
            if (VEC || !HASG) {
                load_px<VEC>(xa, ok, x[i]);
                if (HASG) load_px<VEC>(ga, ok, g[i]);
            } else {
#pragma unroll
                for (int j = 0; j < PX; j++) {
                    x[i][j] = ok[j] ? xa[j * NT] : 0.f;
                    g[i][j] = ok[j] ? ga[j * NT] : 0.f;
                }
            }
            lab[i] = labels ? labels[a] : (float)a;
        }
    }
}

// z = sign * (x + g), exact
template <bool HASG>
__device__ __forceinline__ double zval(float x, float g, bool neg)
{
    const double z = HASG ? (double)x + (double)g : (double)x;
    return neg ? -z : z;
}

// exp(z - m) for z <= m (or a rounding above it).  z = -inf gives 0, also while m is still -inf.
__device__ __forceinline__ double exp_rel(double z, float m)
{
    return z == -INFINITY ? 0.0 : exp(z - (double)m);
}

template <bool VEC, bool HASG, bool FULL>
__device__ __forceinline__ void stats_block(const float *xp, const float *gp, const float *labels, int a0, int L, int64_t n,
                                            bool neg, const bool (&ok)[PX], float (&m)[PX], double (&s)[PX], double (&t)[PX])
{
    float x[BLK][PX], g[BLK][PX], lab[BLK];
    load_block<VEC, HASG, FULL>(xp, gp, labels, a0, L, n, ok, x, g, lab);
#pragma unroll
    for (int j = 0; j < PX; j++) {
        float bm = -INFINITY;                                    // the block's maximum, rounded to fp32: any value near it serves
#pragma unroll
        for (int i = 0; i < BLK; i++)
            if (FULL || a0 + i < L) bm = fmaxf(bm, (float)zval<HASG>(x[i][j], g[i][j], neg));
        if (a0 == 0) {
            m[j] = bm;
        } else if (bm > m[j]) {
            const double r = exp_rel((double)m[j], bm);
            s[j] *= r;
            t[j] *= r;
            m[j] = bm;
        }
        double bs = 0.0, bt = 0.0;
#pragma unroll
        for (int i = 0; i < BLK; i++) {
            if (FULL || a0 + i < L) {
                const double e = exp_rel(zval<HASG>(x[i][j], g[i][j], neg), m[j]);
                bs += e;
                bt = __builtin_fma((double)lab[i], e, bt);
            }
        }
        s[j] += bs;
        t[j] += bt;
    }
}

// m, s and d = t / s of the thread's columns
template <bool VEC, bool HASG>
__device__ __forceinline__ void column_stats(const float *xp, const float *gp, const float *labels, int L, int64_t n, bool neg,
                                             const bool (&ok)[PX], float (&m)[PX], double (&s)[PX], double (&d)[PX])
{
    double t[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) {
        m[j] = 0.f;                                              // (set by the first block)
        s[j] = t[j] = 0.0;
    }
    int a0 = 0;
    for (; a0 + BLK <= L; a0 += BLK) stats_block<VEC, HASG, true>(xp, gp, labels, a0, L, n, neg, ok, m, s, t);
    if (a0 < L) stats_block<VEC, HASG, false>(xp, gp, labels, a0, L, n, neg, ok, m, s, t);
    // one label: d is that label by construction (not by (lab * e) / e rounding back), so the backward's labels[a] - d is 0
    const double only = (double)(labels ? labels[0] : 0.f);
#pragma unroll
    for (int j = 0; j < PX; j++) d[j] = (L == 1 && s[j] > 0.0) ? only : t[j] / s[j];
}

template <bool VEC, bool HASG>
__global__ __launch_bounds__(NT) void k_nchw_expect(const float *__restrict__ X, const float *__restrict__ G,
                                                    const float *__restrict__ labels, float *__restrict__ out, int L, int64_t n,
                                                    int tiles, int negate)
{
    int b;
    int64_t q;
    bool ok[PX];
    if (!thread_pixels<VEC>(n, tiles, blockIdx.x, b, q, ok)) return;
    const int64_t base = (int64_t)b * L * n + q;
    float m[PX], r[PX];
    double s[PX], d[PX];
    column_stats<VEC, HASG>(X + base, HASG ? G + base : nullptr, labels, L, n, negate != 0, ok, m, s, d);
#pragma unroll
    for (int j = 0; j < PX; j++) r[j] = (float)d[j];
    store_px<VEC>(out + (int64_t)b * n + q, ok, r);
}

template <bool VEC, bool HASG, bool FULL>
__device__ __forceinline__ void grad_block(const float *xp, const float *gp, const float *labels, float *zp, int a0, int L,
                                           int64_t n, bool neg, const bool (&ok)[PX], const float (&m)[PX],
                                           const double (&w)[PX], const double (&d)[PX])
{
    float x[BLK][PX], g[BLK][PX], lab[BLK];
    load_block<VEC, HASG, FULL>(xp, gp, labels, a0, L, n, ok, x, g, lab);
#pragma unroll
    for (int i = 0; i < BLK; i++) {
        if (FULL || a0 + i < L) {
            float r[PX];
#pragma unroll
            for (int j = 0; j < PX; j++)
                r[j] = (float)(exp_rel(zval<HASG>(x[i][j], g[i][j], neg), m[j]) * (w[j] * ((double)lab[i] - d[j])));
            store_px<VEC>(zp + (int64_t)(a0 + i) * n, ok, r);
        }
    }
}

template <bool VEC, bool HASG>
__global__ __launch_bounds__(NT) void k_nchw_expect_grad(const float *__restrict__ X, const float *__restrict__ G,
                                                         const float *__restrict__ labels, const float *__restrict__ gout,
                                                         float *__restrict__ gZ, int L, int64_t n, int tiles, int negate)
{
    int b;
    int64_t q;
    bool ok[PX];
    if (!thread_pixels<VEC>(n, tiles, blockIdx.x, b, q, ok)) return;
    const int64_t base = (int64_t)b * L * n + q;
    const float *xp = X + base, *gp = HASG ? G + base : nullptr;
    const bool neg = negate != 0;
    float m[PX], g[PX];
    double s[PX], d[PX], w[PX];
    column_stats<VEC, HASG>(xp, gp, labels, L, n, neg, ok, m, s, d);
    load_px<VEC>(gout + (int64_t)b * n + q, ok, g);
#pragma unroll
    for (int j = 0; j < PX; j++) w[j] = (double)(neg ? -g[j] : g[j]) / s[j];
    int a0 = 0;
    for (; a0 + BLK <= L; a0 += BLK) grad_block<VEC, HASG, true>(xp, gp, labels, gZ + base, a0, L, n, neg, ok, m, w, d);
    if (a0 < L) grad_block<VEC, HASG, false>(xp, gp, labels, gZ + base, a0, L, n, neg, ok, m, w, d);
}

}  // namespace

extern "C" {

int phl_nchw_expected_value(const float *X, const float *G, const float *labels, float *out, int B, int L, int64_t n, int negate,
                            phl_stream stream)
{
    const char *who = "phl_nchw_expected_value";
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0, {X, out},
                   "X / out", {X, G, labels}, out, "out", B, L, n, WGP, rc))
        return rc;
    const int tiles = nchw_tiles(n);
    nchw_dispatch(nchw_vec(n, {X, G, out}), G != nullptr, [&](auto vec, auto has_g) {
        k_nchw_expect<decltype(vec)::value, decltype(has_g)::value>
            <<<nchw_grid(B, tiles), dim3(NT), 0, (hipStream_t)stream>>>(X, G, labels, out, L, n, tiles, negate);
    });
    phl_launched(rc, who);
    return rc;
}

int phl_nchw_expected_value_grad(const float *X, const float *G, const float *labels, const float *gout, float *gZ, int B, int L,
                                 int64_t n, int negate, phl_stream stream)
{
    const char *who = "phl_nchw_expected_value_grad";
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0,
                   {X, gout, gZ}, "X / gout / gZ", {X, G, labels, gout}, gZ, "gZ", B, L, n, WGP, rc))
        return rc;
    const int tiles = nchw_tiles(n);
    nchw_dispatch(nchw_vec(n, {X, G, gout, gZ}), G != nullptr, [&](auto vec, auto has_g) {
        k_nchw_expect_grad<decltype(vec)::value, decltype(has_g)::value>
            <<<nchw_grid(B, tiles), dim3(NT), 0, (hipStream_t)stream>>>(X, G, labels, gout, gZ, L, n, tiles, negate);
    });
    phl_launched(rc, who);
    return rc;
}

}  // extern "C"
