// phl_compat_grad.hip -- the backward of the fused compatibility + softmax step (CRF training).
//
// Forward (phl_meanfield.hip / phl_compat_wide.hip):  Q = softmax(-E),  E = E0 + X Mu,  X = W Q_prev.
// With the upstream gradient gQ:
//   s[p]  = sum_c gQ[p,c] Q[p,c]
//   dE    = Q (s - gQ)            (logits mode, where the step returns -E: dE = -g_out)
//   gE0   = dE
//   gX    = dE Mu^T               [n,L] x [L,L]: the shape of the forward product, no row epilogue
//   gMu   = X^T dE                [L,L], a reduction over all n pixels
//   Potts family (Mu = alpha J + beta I): gX = alpha rowsum(dE) 1 + beta dE, a streaming pass
//
//   k_softmax_neg_grad   dE (and, for the Potts family, gX) in one pass over Q and gQ: a wave per pixel row
//   k_compat_grad_x      gX = scale dE Mu^T on the f32-input matrix cores (exact f32, v_mfma_f32_16x16x4_f32)
//   k_compat_grad_mu     one fp32 slab of X^T dE per pixel range, on the same matrix cores
//   k_compat_grad_mu_sum the slabs summed in a fixed order in fp64 into [L,L]: deterministic bit for bit, no atomics
//
// All kernels: fp32 rows with unit channel stride and row strides % 4 == 0, 16-byte aligned, L % 4 == 0, L <= 512,
// any n.  Every access is a 16-byte piece of a row (L % 4 == 0: a piece is wholly inside the row or wholly outside).
#include <math.h>

#include "phl_reduce.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// NV float4 per lane: rows up to NV * 256 labels.  Q == nullptr (LOGITS): dE = -gQ.  UNIFORM: gX = alpha rowsum(dE) +
// beta dE from the same registers (one read of Q and gQ, two writes).  The row sums and dE itself are formed in fp64 and
// rounded once (the pass is bound by its bytes: the fp64 arithmetic is free), so dE carries half an ulp, not the
// rounding of an f32 dot product -- the products behind it start from the most accurate operand there is.
template <int NV, bool LOGITS, bool UNIFORM>
__global__ __launch_bounds__(256) void k_softmax_neg_grad(const float *__restrict__ Q, int64_t q_rs,
                                                          const float *__restrict__ gQ, int64_t g_rs, float alpha, float beta,
                                                          float *__restrict__ dE, int64_t d_rs, float *__restrict__ gX,
                                                          int64_t x_rs, int64_t n, int L)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t p = wave; p < n; p += nw) {
        float4 g[NV], q[NV];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int c = (j * 64 + lane) * 4;
            if (c < L) {
                g[j] = *reinterpret_cast<const float4 *>(gQ + p * g_rs + c);
                if (!LOGITS) {
                    q[j] = *reinterpret_cast<const float4 *>(Q + p * q_rs + c);
                    s += ((double)g[j].x * q[j].x + (double)g[j].y * q[j].y) + ((double)g[j].z * q[j].z + (double)g[j].w * q[j].w);
                }
            }
        }
        if (!LOGITS) s = wave_sum_d(s);
        double rs = 0.0;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int c = (j * 64 + lane) * 4;
            if (c < L) {
                if (LOGITS) g[j] = make_float4(-g[j].x, -g[j].y, -g[j].z, -g[j].w);
                else g[j] = make_float4((float)(q[j].x * (s - g[j].x)), (float)(q[j].y * (s - g[j].y)),
                                        (float)(q[j].z * (s - g[j].z)), (float)(q[j].w * (s - g[j].w)));
                *reinterpret_cast<float4 *>(dE + p * d_rs + c) = g[j];
                if (UNIFORM) rs += ((double)g[j].x + g[j].y) + ((double)g[j].z + g[j].w);
            }
        }
        if (UNIFORM) {
            const float base = (float)(alpha * wave_sum_d(rs));
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const int c = (j * 64 + lane) * 4;
                if (c < L)
                    *reinterpret_cast<float4 *>(gX + p * x_rs + c) =
                        make_float4(base + beta * g[j].x, base + beta * g[j].y, base + beta * g[j].z, base + beta * g[j].w);
            }
        }
    }
}

__device__ __forceinline__ float4 load4_if(bool ok, const float *p)
{
    return ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------------------
// k_compat_grad_x: gX[p,c] = scale sum_k dE[p,k] Mu[c,k].  Computed transposed, as the forward product (labels = MFMA
// rows, pixels = MFMA columns), so that a lane ends with four consecutive labels of a pixel (16-byte stores).
// A wave owns 64 pixels x 64 labels (4 x 4 tiles of 16x16, 64 accumulator registers); a workgroup is four waves, NLW of
// them side by side along the labels (NLW = 1, 2, 4 for L <= 64, 128, 512) on the same pixels, whose dE rows the
// workgroup shares through L1.  Both operands are k-contiguous rows, so the 16x16x4 maps take them straight from global
// memory: lane (i, g) reads the 16 bytes k = k0 + 4g .. +3 of its row (pixel / label 16t + i) and feeds component u to
// MFMA u of the k step, which contracts k = k0 + 4g' + u over the four k-slots g' -- A and B agree on the k order, so
// the sum is that of the product.  The next 16 k are loaded before the current step's 64 MFMAs.
__global__ __launch_bounds__(256) void k_compat_grad_x(const float *__restrict__ dE, int64_t de_rs, const float *__restrict__ Mu,
                                                       float scale, float *__restrict__ gX, int64_t gx_rs, int64_t n, int L,
                                                       int nlw)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int lw = wave % nlw, pw = wave / nlw;
    const int64_t p0 = ((int64_t)blockIdx.x * (4 / nlw) + pw) * 64;
    const int c0 = ((int)blockIdx.y * nlw + lw) * 64;
    if (c0 >= L || p0 >= n) return;               // wave-uniform; the kernel has no barrier

    const float *brow[4], *arow[4];
    bool bok[4], aok[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int64_t p = p0 + 16 * t + i;
        bok[t] = p < n;
        brow[t] = dE + (bok[t] ? p : 0) * de_rs + 4 * g;
        const int c = c0 + 16 * t + i;
        aok[t] = c < L;
        arow[t] = Mu + (int64_t)(aok[t] ? c : 0) * L + 4 * g;
    }
    f32x4 acc[4][4];                              // [pixel tile][label tile]
#pragma unroll
    for (int pt = 0; pt < 4; pt++)
#pragma unroll
        for (int lt = 0; lt < 4; lt++) acc[pt][lt] = (f32x4)0.f;

    float4 a[4], b[4], an[4], bn[4];
    auto load = [&](int k, float4(&A)[4], float4(&B)[4]) {
        const bool kok = k + 4 * g < L;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            A[t] = load4_if(aok[t] && kok, arow[t] + k);
            B[t] = load4_if(bok[t] && kok, brow[t] + k);
        }
    };
    load(0, a, b);
    for (int k = 0; k < L; k += 16) {
        const bool more = k + 16 < L;
        if (more) load(k + 16, an, bn);
#define PHL_GX_MF(comp)                                                                                                  \
    _Pragma("unroll") for (int lt = 0; lt < 4; lt++) _Pragma("unroll") for (int pt = 0; pt < 4; pt++)                    \
        acc[pt][lt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[lt].comp, b[pt].comp, acc[pt][lt], 0, 0, 0);
        PHL_GX_MF(x) PHL_GX_MF(y) PHL_GX_MF(z) PHL_GX_MF(w)
#undef PHL_GX_MF
        if (more) {
#pragma unroll
            for (int t = 0; t < 4; t++) { a[t] = an[t]; b[t] = bn[t]; }
        }
    }
    // lane (i, g), register r of accumulator (pt, lt): label c0 + 16 lt + 4 g + r of pixel p0 + 16 pt + i
#pragma unroll
    for (int pt = 0; pt < 4; pt++) {
        const int64_t p = p0 + 16 * pt + i;
        if (p >= n) continue;
#pragma unroll
        for (int lt = 0; lt < 4; lt++) {
            const int c = c0 + 16 * lt + 4 * g;
            if (c < L) {
                const f32x4 v = acc[pt][lt] * scale;
                *reinterpret_cast<float4 *>(gX + p * gx_rs + c) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_compat_grad_mu: slab[r][k][c] = sum over the pixels p of range r of X[p,k] dE[p,c].  The contraction runs over
// pixels, so a k step of the 16x16x4 MFMA is four pixels: lane (i, g) reads the 16-byte piece 4i .. 4i+3 of row p + g of
// X (labels r0 + 4i + a) and of dE (labels c0 + 4i + b), and component a (b) is row (column) i of A tile a (B tile b):
// tile (a, b) collects gMu[r0 + 4m + a][c0 + 4j + b] at its (m, j).  One 16-byte load per operand and four pixels feeds
// 16 MFMAs, and a lane ends with gMu[r0 + 4(4g + rr) + a][c0 + 4i .. 4i + 3] in register rr of tiles (a, 0..3): 16-byte
// stores.  A wave owns 64 x 64 outputs (64 accumulator registers); a workgroup is the slab of NWR x NWC waves (NWC =
// ceil(L / 64) covering every column, NWR = min(NWC, 16 / NWC) row bands of 64): the whole [L,L] for L <= 256, so X and
// dE are read once.  Above 256 labels a slab is 128 label rows (NSLABS = 3 at 344 labels, 4 at 512): the [L,L] of a range
// does not fit one workgroup's registers (at 512 labels it is twice a CU's whole register file), so each slab's workgroup reads the range's dE rows (X only its own columns).  Those
// workgroups are placed on ONE XCD (REMAP: workgroups are dealt round-robin over the 8 XCDs, so the slabs of range r get
// ids of equal id % 8) and start together: they stream the same dE rows in step through that XCD's L2, and HBM serves dE
// about once.  Eight pixels are loaded ahead of the current eight's 32 MFMAs.
__global__ __launch_bounds__(1024) void k_compat_grad_mu(const float *__restrict__ X, int64_t x_rs, const float *__restrict__ dE,
                                                         int64_t de_rs, int64_t n, int L, int64_t chunk, int nwc, int S,
                                                         int nslabs, int remap, float *__restrict__ slabs)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int wr = wave / nwc, wc = wave % nwc;
    const int b = (int)blockIdx.x;                // -> (range, slab); remap: blocks b = 8 j + x of XCD x, j = nslabs q + slab
    const int slab = remap ? (b >> 3) % nslabs : b % nslabs;
    const int64_t range = remap ? (b & 7) + 8 * (int64_t)((b >> 3) / nslabs) : b / nslabs;
    const int r0 = slab * S + 64 * wr, c0 = 64 * wc;
    if (r0 >= L) return;                          // wave-uniform; the kernel has no barrier
    const int64_t pb = range * chunk, pe = min(n, pb + chunk);
    const bool xok = r0 + 4 * i < L, dok = c0 + 4 * i < L;
    const float *xp = X + r0 + 4 * i, *dp = dE + c0 + 4 * i;

    f32x4 acc[4][4];                              // [a: row component][b: column component]
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = (f32x4)0.f;

    float4 x[2], d[2], xn[2], dn[2];
    auto load = [&](int64_t p, float4(&XV)[2], float4(&DV)[2]) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int64_t q = p + 4 * s + g;
            const bool ok = q < pe;
            XV[s] = load4_if(ok && xok, xp + (ok ? q : 0) * x_rs);
            DV[s] = load4_if(ok && dok, dp + (ok ? q : 0) * de_rs);
        }
    };
    if (pb < pe) load(pb, x, d);
    for (int64_t p = pb; p < pe; p += 8) {
        const bool more = p + 8 < pe;
        if (more) load(p + 8, xn, dn);
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const float xa[4] = {x[s].x, x[s].y, x[s].z, x[s].w}, db[4] = {d[s].x, d[s].y, d[s].z, d[s].w};
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[a], db[b], acc[a][b], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int s = 0; s < 2; s++) { x[s] = xn[s]; d[s] = dn[s]; }
        }
    }
    if (!dok) return;
    float *out = slabs + range * L * L;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int row = r0 + 4 * (4 * g + rr) + a;
            if (row < L)
                *reinterpret_cast<float4 *>(out + (int64_t)row * L + c0 + 4 * i) =
                    make_float4(acc[a][0][rr], acc[a][1][rr], acc[a][2][rr], acc[a][3][rr]);
        }
}

// gMu[e] = (accumulate ? gMu[e] : 0) + scale * sum_{r = 0 .. R-1} slab[r][e], the sum in fp64 in range order, one
// rounding at the end.  R = 0: gMu is zeroed (or left as it is).
__global__ __launch_bounds__(256) void k_compat_grad_mu_sum(const float *__restrict__ slabs, int R, int64_t LL, float scale,
                                                            int accumulate, float *__restrict__ gMu)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= LL) return;
    double s = 0.0;
    for (int r = 0; r < R; r++) s += (double)slabs[(int64_t)r * LL + e];
    s *= (double)scale;
    if (accumulate) s += (double)gMu[e];
    gMu[e] = (float)s;
}

inline unsigned grad_rows_grid(int64_t n)
{
    int64_t b = (n + 3) / 4;
    if (b > 256 * 8) b = 256 * 8;
    return (unsigned)(b < 1 ? 1 : b);
}

// the slab geometry of k_compat_grad_mu for L labels: waves per row band (NWC), row bands per slab (NWR), slabs
struct MuGeom {
    int nwc, nwr, S, nslabs;
};
inline MuGeom mu_geom(int L)
{
    MuGeom m;
    m.nwc = (L + 63) / 64;
    m.nwr = min(m.nwc, 16 / m.nwc);
    m.S = 64 * m.nwr;
    m.nslabs = (L + m.S - 1) / m.S;
    return m;
}
// pixel ranges: enough workgroups for the 256 CUs (one per CU at 16 waves; smaller slabs: more of them), at least 64
// pixels each (short f32 chains: the ranges meet in fp64), and no more than 64 MiB of slabs (16 Mi floats); with more
// than one slab a multiple of 8 from 8 ranges on (every XCD then holds whole ranges: see REMAP above)
inline int64_t mu_ranges(int64_t n, int L)
{
    const MuGeom m = mu_geom(L);
    const int64_t occ = 256 * (int64_t)max(1, 16 / (m.nwc * m.nwr)) / m.nslabs;
    const int64_t mem = ((int64_t)16 << 20) / ((int64_t)L * L);
    int64_t r = (n + 63) / 64;
    r = min(r, min(occ, mem));
    if (m.nslabs > 1 && r >= 8) r = r / 8 * 8;
    return r < 1 ? 1 : r;
}
inline bool grad_l_ok(int L) { return L >= 4 && L <= 512 && L % 4 == 0; }

}  // namespace

extern "C" {

int phl_softmax_neg_grad(const float *Q, int64_t q_rs, const float *gQ, int64_t g_rs, float *dE, int64_t d_rs, int64_t n, int L,
                         phl_stream stream)
{
    return phl_uniform_compat_grad(Q, q_rs, gQ, g_rs, 0.f, 0.f, dE, d_rs, nullptr, 0, n, L, stream);
}

int phl_uniform_compat_grad(const float *Q, int64_t q_rs, const float *gQ, int64_t g_rs, float alpha, float beta, float *dE,
                            int64_t d_rs, float *gX, int64_t x_rs, int64_t n, int L, phl_stream stream)
{
    if (n < 0 || L < 1 || (n > 0 && (!gQ || !dE))) { phl_set_error("phl_uniform_compat_grad: bad arguments"); return PHL_ERR_INVALID; }
    if (!grad_l_ok(L) || !phl_rows16(gQ, g_rs) || !phl_rows16(dE, d_rs) || (Q && !phl_rows16(Q, q_rs)) || (gX && !phl_rows16(gX, x_rs))) {
        phl_set_error("phl_uniform_compat_grad / phl_softmax_neg_grad: needs L %% 4 == 0, L <= 512 and 16-byte aligned rows (L=%d)", L);
        return PHL_ERR_UNSUPPORTED;
    }
    if (n == 0) return PHL_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = grad_rows_grid(n);
#define PHL_SG(NV_, LG_, UN_)                                                                                             \
    k_softmax_neg_grad<NV_, LG_, UN_><<<dim3(grid), dim3(256), 0, st>>>(Q, q_rs, gQ, g_rs, alpha, beta, dE, d_rs, gX, x_rs, n, L)
#define PHL_SG_NV(NV_)                                                                                                    \
    do {                                                                                                                  \
        if (!Q && gX) PHL_SG(NV_, true, true);                                                                            \
        else if (!Q) PHL_SG(NV_, true, false);                                                                            \
        else if (gX) PHL_SG(NV_, false, true);                                                                            \
        else PHL_SG(NV_, false, false);                                                                                   \
    } while (0)
    if (L <= 256) PHL_SG_NV(1);
    else PHL_SG_NV(2);
#undef PHL_SG_NV
#undef PHL_SG
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

int phl_compat_grad_x(const float *dE, int64_t de_rs, const float *Mu, float scale, float *gX, int64_t gx_rs, int64_t n, int L,
                      phl_stream stream)
{
    if (n < 0 || L < 1 || (n > 0 && (!dE || !Mu || !gX))) { phl_set_error("phl_compat_grad_x: bad arguments"); return PHL_ERR_INVALID; }
    if (!grad_l_ok(L) || !phl_rows16(dE, de_rs) || !phl_rows16(gX, gx_rs) || !phl_al16(Mu)) {
        phl_set_error("phl_compat_grad_x: needs L %% 4 == 0, L <= 512 and 16-byte aligned rows (L=%d)", L);
        return PHL_ERR_UNSUPPORTED;
    }
    if (n == 0) return PHL_OK;
    const int nlw = L <= 64 ? 1 : L <= 128 ? 2 : 4;
    const int64_t px_per_wg = 64 * (4 / nlw);
    const dim3 grid((unsigned)((n + px_per_wg - 1) / px_per_wg), (unsigned)((L + 64 * nlw - 1) / (64 * nlw)));
    k_compat_grad_x<<<grid, dim3(256), 0, (hipStream_t)stream>>>(dE, de_rs, Mu, scale, gX, gx_rs, n, L, nlw);
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

size_t phl_compat_mu_grad_workspace_bytes(int64_t n, int L)
{
    if (!grad_l_ok(L) || n < 0) return 0;
    return (size_t)mu_ranges(n, L) * (size_t)L * (size_t)L * sizeof(float);
}

int phl_compat_mu_grad(const float *X, int64_t x_rs, const float *dE, int64_t de_rs, float scale, int64_t n, int L, void *workspace,
                       float *gMu, int accumulate, phl_stream stream)
{
    if (n < 0 || L < 1 || !gMu || !workspace || (n > 0 && (!X || !dE))) { phl_set_error("phl_compat_mu_grad: bad arguments"); return PHL_ERR_INVALID; }
    if (!grad_l_ok(L) || !phl_rows16(X, x_rs) || !phl_rows16(dE, de_rs) || !phl_al16(workspace)) {
        phl_set_error("phl_compat_mu_grad: needs L %% 4 == 0, L <= 512 and 16-byte aligned rows (L=%d)", L);
        return PHL_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const MuGeom m = mu_geom(L);
    const int64_t R = mu_ranges(n, L);
    int64_t chunk = (n + R - 1) / R;
    chunk = (chunk + 7) / 8 * 8;                  // whole 8-pixel steps (the last range ends at n)
    float *slabs = static_cast<float *>(workspace);
    if (n > 0)
        k_compat_grad_mu<<<dim3((unsigned)(m.nslabs * R)), dim3(64 * m.nwr * m.nwc), 0, st>>>(
            X, x_rs, dE, de_rs, n, L, chunk, m.nwc, m.S, m.nslabs, m.nslabs > 1 && R % 8 == 0 ? 1 : 0, slabs);
    const int64_t LL = (int64_t)L * L;
    k_compat_grad_mu_sum<<<dim3((unsigned)((LL + 255) / 256)), dim3(256), 0, st>>>(slabs, n > 0 ? (int)R : 0, LL, scale,
                                                                                   accumulate, gMu);
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

}  // extern "C"
