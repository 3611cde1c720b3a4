// phl_blur.hip -- the separable Gaussian of the guided filter (crf/guided.py: box_filter, gaussian_blur, GaussianBlur):
// a cascade of K normalised box passes along one axis, and the sigma-gradient of the 3-pass cascade.
//
// One box pass along an axis of length h, r >= 1 (the reference's cumsum form, quirks kept):
//   B_r(x)[i] = sum(x[j], j = max(0, i-r+1) .. min(h-1, i+r)) / c(i),   c(i) = min(i, r) + min(h-1-i, r) + 1
// The contiguous tensor is viewed as [outer, h, inner]; a "line" is one (outer, inner) pair.
//
// k_box_cascade streams each line ONCE through all K passes.  Step t feeds input position t into pass 1; pass p emits
// its output for position t - p r (its window (t - 2r, t] is complete), and that value is the input of pass p + 1 at the
// same step.  Every pass keeps its window sum in fp64 (adding the entering and subtracting the leaving sample); the value
// that leaves is read back: for pass 1 from global memory (2r rows back, an L2 hit), for passes 2..K from a per-lane ring
// of the last 2r values in LDS ([slot][lane]: conflict-free, each lane only touches its own column, no barrier).  A pass
// output is rounded to fp32 once, before it enters the next pass (the ring and the sum see the same fp32 value, so the
// sum never drifts), and the last pass is rounded once into the output.
//
// A workgroup is one wave: 64 lines x one chunk [i0, i1) of h.  It starts K (r-1) samples below i0 and recomputes that
// halo instead of synchronising with the neighbouring chunk; outputs below i0 are discarded.  Two access forms:
//   inner >= 2  lanes run across inner (coalesced rows), 8 steps of loads are issued ahead of their use
//   inner == 1  lines are contiguous: blocks of SB steps of the 64 lines are staged through padded LDS tiles with
//               coalesced segment loads and stores (no lane-per-line global access)
//
// GRAD (K = 3): the same stream over v and g runs the four cascades g, g fl, v, v fl with fl = (i - i0) / sigma (local
// coordinates: f = i / sigma = fl + i0 / sigma and every f-term of the gradient is shift invariant, so the cancellation
// between f B(g) and B(g f) is bounded by the chunk, not by the line length), writes grad_x = B(g) when asked, and sums
//   D f - B(g) v,   D = v fl B(g) - v B(g fl) + g fl B(v) - g B(v fl)      (= -grad_f of the reference)
// per workgroup in fp64 into one partial; k_sum_partials<1> (phl_reduce.h) adds the partials in a fixed order:
// grad_sigma = sum / sigma.
#include <math.h>

#include "phl_reduce.h"

namespace {

constexpr int SB = 16;              // steps per staged block (inner == 1 form)
constexpr int TP = SB + 1;          // padded tile row: lane l reads word l * 17 + s, 32 distinct banks per lane group
constexpr int CB = 8;               // steps of loads issued ahead (inner >= 2 form)

template <bool ROWS, int K, bool GRAD>
__global__ __launch_bounds__(64) void k_box_cascade(const float *__restrict__ x, const float *__restrict__ gin,
                                                    float *__restrict__ out, double *__restrict__ partial, int64_t outer,
                                                    int64_t h, int64_t inner, int64_t ncb, int r, int64_t T, double inv_sigma)
{
    constexpr int NCH = GRAD ? 4 : 1;           // cascades per line
    constexpr int NIN = GRAD ? 2 : 1;           // input arrays (v, g)
    extern __shared__ float lds[];
    const int lane = threadIdx.x;
    const int64_t gi = blockIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * T, i1 = min(h, i0 + T);
    const int r2 = 2 * r;
    const int64_t ts = max((int64_t)0, i0 - (int64_t)K * (r - 1));
    const int64_t te = i1 - 1 + (int64_t)K * r;

    float *ring = lds;                          // [(K-1) * NCH][2r][64]
    float *tiles = lds + (size_t)(K - 1) * NCH * r2 * 64;

    // line -> element (line, i) at base + i * stride
    int64_t base, stride, o0 = 0;
    bool ok;
    if (ROWS) {
        o0 = gi * 64;
        ok = o0 + lane < outer;
        base = (ok ? o0 + lane : 0) * h;
        stride = 1;
    } else {
        const int64_t o = gi / ncb, j = (gi % ncb) * 64 + lane;
        ok = j < inner;
        base = o * h * inner + (ok ? j : 0);
        stride = inner;
    }
    const float *src[2] = {x, gin};             // forward: x;  GRAD: v = x, g = gin

    for (int e = lane; e < (K - 1) * NCH * r2 * 64; e += 64) ring[e] = 0.f;   // own column only (e % 64 == lane)

    double S[NCH][K];
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int p = 0; p < K; p++) S[c][p] = 0.0;
    const double inv_mid = 1.0 / (double)(r2 + 1);
    auto rcp = [&](int64_t q) -> double {
        const int64_t c = min(q, (int64_t)r) + min(h - 1 - q, (int64_t)r) + 1;
        return c == r2 + 1 ? inv_mid : 1.0 / (double)c;
    };
    int slot = 0;
    double acc = 0.0;

    // one step: input at position t (and the values leaving pass 1), returns the cascade output(s) for t - K r
    auto step = [&](int64_t t, const float (&in)[NIN], const float (&lv)[NIN], double (&res)[NCH]) {
        double cur[NCH];
        if (GRAD) {
            const double fl_in = (double)(t - i0) * inv_sigma, fl_lv = (double)(t - r2 - i0) * inv_sigma;
            const double g = in[1], gl = lv[1], v = in[0], vl = lv[0];
            S[0][0] += g - gl;
            S[1][0] += g * fl_in - gl * fl_lv;
            S[2][0] += v - vl;
            S[3][0] += v * fl_in - vl * fl_lv;
        } else {
            S[0][0] += (double)in[0] - (double)lv[0];
        }
        {
            const int64_t q = t - r;
            const bool inside = q >= 0 && q < h;
            const double w = inside ? rcp(q) : 0.0;
#pragma unroll
            for (int c = 0; c < NCH; c++) cur[c] = S[c][0] * w;
        }
#pragma unroll
        for (int p = 1; p < K; p++) {
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                float *rs = ring + ((size_t)(c * (K - 1) + p - 1) * r2 + slot) * 64 + lane;
                const float vin = (float)cur[c];
                const float old = *rs;
                *rs = vin;
                S[c][p] += (double)vin - (double)old;
            }
            const int64_t q = t - (int64_t)(p + 1) * r;
            const bool inside = q >= 0 && q < h;
            const double w = inside ? rcp(q) : 0.0;
#pragma unroll
            for (int c = 0; c < NCH; c++) cur[c] = S[c][p] * w;
        }
        if (++slot == r2) slot = 0;
#pragma unroll
        for (int c = 0; c < NCH; c++) res[c] = cur[c];
    };
    // GRAD epilogue at output position q (inside [i0, i1)): the sigma term, and B(g) as grad_x
    auto grad_term = [&](int64_t q, const double *res, float vq, float gq) {
        const double fl = (double)(q - i0) * inv_sigma, f = (double)q * inv_sigma;
        const double v = vq, g = gq;
        const double D = v * fl * res[0] - v * res[1] + g * fl * res[2] - g * res[3];
        acc += D * f - res[0] * v;
    };

    if (!ROWS) {
        for (int64_t tb = ts; tb <= te; tb += CB) {
            float in[CB][NIN], lv[CB][NIN], vo[CB], go[CB];
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const int64_t t = tb + s, tl = t - r2, q = t - (int64_t)K * r;
                const bool tin = ok && t <= te && t < h, tlv = ok && tl >= ts && tl < h;
                const bool qin = GRAD && ok && t <= te && q >= i0 && q < i1;
#pragma unroll
                for (int a = 0; a < NIN; a++) {
                    in[s][a] = tin ? src[a][base + t * stride] : 0.f;
                    lv[s][a] = tlv ? src[a][base + tl * stride] : 0.f;
                }
                if (GRAD) {
                    vo[s] = qin ? x[base + q * stride] : 0.f;
                    go[s] = qin ? gin[base + q * stride] : 0.f;
                }
            }
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const int64_t t = tb + s, q = t - (int64_t)K * r;
                if (t > te) break;
                double res[NCH];
                step(t, in[s], lv[s], res);
                if (q >= i0 && ok) {
                    if (GRAD) grad_term(q, res, vo[s], go[s]);
                    if (out) out[base + q * stride] = (float)res[0];
                }
            }
        }
    } else {
        // tiles: [NIN] input, [NIN] leaving, GRAD: v and g at the output position; [1] output.  Each [64][TP].
        float *t_in = tiles, *t_lv = tiles + NIN * 64 * TP, *t_q = tiles + 2 * NIN * 64 * TP;
        float *t_out = tiles + (2 * NIN + (GRAD ? 2 : 0)) * 64 * TP;
        for (int64_t tb = ts; tb <= te; tb += SB) {
#pragma unroll 4
            for (int k = 0; k < SB; k++) {
                const int qf = k * 64 + lane, l = qf / SB, s = qf % SB;
                const int64_t line = o0 + l, t = tb + s, tl = t - r2, q = t - (int64_t)K * r;
                const bool lok = line < outer;
                const int64_t lb = (lok ? line : 0) * h;
#pragma unroll
                for (int a = 0; a < NIN; a++) {
                    t_in[(a * 64 + l) * TP + s] = lok && t <= te && t < h ? src[a][lb + t] : 0.f;
                    t_lv[(a * 64 + l) * TP + s] = lok && tl >= ts && tl < h ? src[a][lb + tl] : 0.f;
                    if (GRAD) t_q[(a * 64 + l) * TP + s] = lok && t <= te && q >= i0 && q < i1 ? src[a][lb + q] : 0.f;
                }
            }
            __syncthreads();
            for (int s = 0; s < SB; s++) {
                const int64_t t = tb + s, q = t - (int64_t)K * r;
                if (t > te) break;
                float in[NIN], lv[NIN];
#pragma unroll
                for (int a = 0; a < NIN; a++) {
                    in[a] = t_in[(a * 64 + lane) * TP + s];
                    lv[a] = t_lv[(a * 64 + lane) * TP + s];
                }
                double res[NCH];
                step(t, in, lv, res);
                if (GRAD && q >= i0 && ok) grad_term(q, res, t_q[lane * TP + s], t_q[(64 + lane) * TP + s]);
                t_out[lane * TP + s] = (float)res[0];
            }
            __syncthreads();
            if (out) {
#pragma unroll 4
                for (int k = 0; k < SB; k++) {
                    const int qf = k * 64 + lane, l = qf / SB, s = qf % SB;
                    const int64_t line = o0 + l, t = tb + s, q = t - (int64_t)K * r;
                    if (line < outer && t <= te && q >= i0 && q < i1) out[line * h + q] = t_out[l * TP + s];
                }
            }
        }
    }
    if (GRAD) {
        acc = wave_sum_d(acc);
        if (lane == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}

// ---- geometry ----------------------------------------------------------------------------------------------------
struct Geom {
    bool rows;
    int64_t groups, ncb, T, chunks;
};
inline Geom geom(int64_t outer, int64_t h, int64_t inner, int r, int K)
{
    Geom g;
    g.rows = inner == 1;
    g.ncb = g.rows ? 1 : (inner + 63) / 64;
    g.groups = g.rows ? (outer + 63) / 64 : outer * g.ncb;
    // about 4096 workgroups when the lines alone do not make them; a chunk at least 4 K r (and 64) long, so that the
    // recomputed halo stays a fraction of the chunk
    const int64_t want = (4096 + g.groups - 1) / g.groups;
    const int64_t minT = max((int64_t)64, (int64_t)4 * K * r);
    g.chunks = max((int64_t)1, min(want, h / minT));
    g.T = (h + g.chunks - 1) / g.chunks;
    g.chunks = (h + g.T - 1) / g.T;
    return g;
}
inline size_t cascade_lds(bool rows, int K, bool grad, int r)
{
    const size_t nch = grad ? 4 : 1, nin = grad ? 2 : 1;
    const size_t rings = (size_t)(K - 1) * nch * 2 * (size_t)r * 64 * sizeof(float);
    const size_t tiles = rows ? (2 * nin + (grad ? 2 : 0) + 1) * 64 * TP * sizeof(float) : 0;
    return rings + tiles;
}
constexpr size_t kFusedLds = 64 << 10;       // forward: fused while two workgroups fit a CU; above, K single passes
constexpr size_t kGradLds = 160 << 10;       // sigma-gradient: up to a whole CU's LDS (r <= 40 / 32, see phl.h)

int check_sizes(const char *who, int64_t outer, int64_t h, int64_t inner, int r)
{
    if (outer < 0 || h < 0 || inner < 0 || r < 1) {
        phl_set_error("%s: bad arguments (outer=%lld h=%lld inner=%lld r=%d)", who, (long long)outer, (long long)h,
                      (long long)inner, r);
        return PHL_ERR_INVALID;
    }
    if (outer == 0 || h == 0 || inner == 0) return PHL_OK;
    const int64_t lim = INT64_MAX / 4;       // byte offsets stay in int64
    if (h > lim / outer || inner > lim / (outer * h) || (inner == 1 ? (outer + 63) / 64 : outer * ((inner + 63) / 64)) > INT32_MAX) {
        phl_set_error("%s: %lld x %lld x %lld elements are too many", who, (long long)outer, (long long)h, (long long)inner);
        return PHL_ERR_TOO_LARGE;
    }
    return PHL_OK;
}

template <bool ROWS, int K, bool GRAD>
int launch_one(const float *x, const float *g, float *out, double *partial, int64_t outer, int64_t h, int64_t inner, int r,
               double inv_sigma, const Geom &gm, hipStream_t st)
{
    const size_t lds = cascade_lds(ROWS, K, GRAD, r);
    auto kern = k_box_cascade<ROWS, K, GRAD>;
    if (int rc = phl_allow_lds(kern, lds)) return rc;
    kern<<<dim3((unsigned)gm.groups, (unsigned)gm.chunks), dim3(64), lds, st>>>(x, g, out, partial, outer, h, inner, gm.ncb, r,
                                                                             gm.T, inv_sigma);
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

template <bool ROWS>
int launch_fwd(int K, const float *x, float *out, int64_t outer, int64_t h, int64_t inner, int r, const Geom &gm, hipStream_t st)
{
    switch (K) {
    case 1: return launch_one<ROWS, 1, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    case 2: return launch_one<ROWS, 2, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    case 3: return launch_one<ROWS, 3, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    case 4: return launch_one<ROWS, 4, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    case 5: return launch_one<ROWS, 5, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    case 6: return launch_one<ROWS, 6, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    case 7: return launch_one<ROWS, 7, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    default: return launch_one<ROWS, 8, false>(x, nullptr, out, nullptr, outer, h, inner, r, 0.0, gm, st);
    }
}

}  // namespace

extern "C" {

int phl_box_blur_fused_max_r(int inner_is_one, int passes, int grad)
{
    int r = 0;
    const bool rows = inner_is_one != 0;
    if (passes < 1 || passes > 8) return 0;
    if (passes == 1) return INT32_MAX;
    while (cascade_lds(rows, passes, grad != 0, r + 1) <= (grad ? kGradLds : kFusedLds)) r++;
    return r;
}

int phl_box_blur(const float *src, float *dst, int64_t outer, int64_t h, int64_t inner, int r, int passes, phl_stream stream)
{
    if (int rc = check_sizes("phl_box_blur", outer, h, inner, r)) return rc;
    if (passes < 1 || passes > 8) { phl_set_error("phl_box_blur: passes must be 1..8, got %d", passes); return PHL_ERR_INVALID; }
    if (outer == 0 || h == 0 || inner == 0) return PHL_OK;
    if (!src || !dst || src == dst) { phl_set_error("phl_box_blur: null or identical src / dst"); return PHL_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    const int re = (int)min((int64_t)r, h);          // r >= h: every window is the whole line, as with r = h
    const bool rows = inner == 1;
    if (cascade_lds(rows, passes, false, re) <= kFusedLds) {
        const Geom gm = geom(outer, h, inner, re, passes);
        return rows ? launch_fwd<true>(passes, src, dst, outer, h, inner, re, gm, st)
                    : launch_fwd<false>(passes, src, dst, outer, h, inner, re, gm, st);
    }
    // above the fused limit: one pass per launch through two temporaries (stream-ordered allocations)
    const Geom gm = geom(outer, h, inner, re, 1);
    const size_t count = (size_t)outer * h * inner;
    phl_temps tmp(st);
    float *t[2] = {passes >= 2 ? tmp.get<float>(count) : nullptr, passes >= 3 ? tmp.get<float>(count) : nullptr};
    const float *in = src;
    int &rc = tmp.rc;
    for (int p = 0; p < passes && rc == PHL_OK; p++) {
        float *o = p == passes - 1 ? dst : t[p % 2];
        rc = rows ? launch_fwd<true>(1, in, o, outer, h, inner, re, gm, st) : launch_fwd<false>(1, in, o, outer, h, inner, re, gm, st);
        in = o;
    }
    return tmp.release();
}

int phl_box_blur_grad(const float *v, const float *g, int64_t outer, int64_t h, int64_t inner, int r, double sigma,
                      float *grad_x, float *grad_sigma, phl_stream stream)
{
    if (int rc = check_sizes("phl_box_blur_grad", outer, h, inner, r)) return rc;
    if (!(sigma > 0.0) || !isfinite(sigma) || (!grad_x && !grad_sigma)) {
        phl_set_error("phl_box_blur_grad: needs sigma > 0 and grad_x or grad_sigma");
        return PHL_ERR_INVALID;
    }
    const bool empty = outer == 0 || h == 0 || inner == 0;
    if (!empty && (!v || !g || (grad_x && (grad_x == v || grad_x == g)))) {
        phl_set_error("phl_box_blur_grad: null v / g, or grad_x aliases them");
        return PHL_ERR_INVALID;
    }
    const int re = empty ? 1 : (int)min((int64_t)r, h);
    const bool rows = inner == 1;
    if (grad_sigma && cascade_lds(rows, 3, true, re) > kGradLds) {
        phl_set_error("phl_box_blur_grad: r = %d above the fused limit %d", re, phl_box_blur_fused_max_r(rows, 3, 1));
        return PHL_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!grad_sigma) return phl_box_blur(g, grad_x, outer, h, inner, r, 3, stream);
    if (empty) {
        PHL_HIP(hipMemsetAsync(grad_sigma, 0, sizeof(float), st));
        return PHL_OK;
    }
    const Geom gm = geom(outer, h, inner, re, 3);
    const int64_t nparts = gm.groups * gm.chunks;
    phl_temps tmp(st);
    double *partial = tmp.get<double>((size_t)nparts);
    int &rc = tmp.rc;
    if (rc == PHL_OK)
        rc = rows ? launch_one<true, 3, true>(v, g, grad_x, partial, outer, h, inner, re, 1.0 / sigma, gm, st)
                  : launch_one<false, 3, true>(v, g, grad_x, partial, outer, h, inner, re, 1.0 / sigma, gm, st);
    if (rc == PHL_OK) {
        k_sum_partials<1><<<dim3(1), dim3(256), 0, st>>>(partial, nparts, 1.0 / sigma, grad_sigma);
        phl_launched(rc, "k_sum_partials");
    }
    return tmp.release();
}

}  // extern "C"
