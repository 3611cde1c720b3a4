// phl_nchw.hip -- the non-W half of one mean-field iteration for channel-major (NCHW) data, fused.
//
// Reference (crf/crf_module.py:66-79, 97-103): per iteration  Y = Mu(Q);  E = E0 + W(Y);  Q = softmax(-E, dim=1)  on
// [B, L, H, W] tensors, Mu a 1x1 convolution over the label channels.  Around W that is a library convolution, an add,
// a negation and a 2-3 pass softmax over a strided dimension: about seven sweeps over an L-plane tensor.  Here the
// piece between two W calls is ONE kernel -- softmax first, then the product (the dual of k_compat_softmax, which is
// product first, then softmax, on pixel-major rows):
//
//     Y[b, c, p] = sum_a M[a, c] * softmax_a( -(E0[b, a, p] + G[b, a, p]) )            (G optional)
//
// E0 and G are read once, Y is written once, Q and E never exist in memory.
//
//   k_nchw_tile     L <= 256: a workgroup owns TP = 64 consecutive pixels of one image and all L labels of them.  The
//                   [L][TP] block of -(E0 + G) is staged in LDS (64 KiB at 256 labels: two workgroups per CU), the column
//                   softmax runs there (four threads per pixel, max-subtracted, expf, one 1.0f / s per pixel), then
//                     PRODUCT, L > 32   Y^T = M^T Q^T on v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fma chain).  M^T
//                                       is operand A, read from global memory / L2 as it is (lane l: M[a = k + l/32]
//                                       [c = 32 ct + l%32], 128 contiguous bytes per k); the softmaxed tile is operand B,
//                                       read from LDS (lane l: Q[a = k + l/32][pixel 32 h + l%32]: one ds_read_b32, the two
//                                       lane halves on rows of their own, no bank conflict at a row stride of TP).  Wave w
//                                       owns pixel half w & 1 and the label tiles (w >> 1) + 2 i: at most four 32x32
//                                       accumulators, 64 registers.
//                     PRODUCT, L <= 32  the same fma chain on the VALU: one label tile would leave half the waves without
//                                       work and pad 32 labels; at L = 18 the step needs ~1.5 fma per byte moved.
//                     UNIFORM           Y = alpha * colsum(Q) + beta * Q (M = alpha J + beta I, the Potts family), the
//                                       column sum computed, no product.
//                     SOFTMAX           Y = Q.
//                   The result goes back into the LDS block and is stored the way the input was loaded: along the pixel
//                   axis, 256 contiguous bytes per label plane and wave quarter -- float4 accesses when n % 4 == 0 and all
//                   pointers are 16-byte aligned (then every plane base and every tile base is), dwords otherwise.  The
//                   last tile of an image may be shorter than TP: its missing pixels are computed on zeros and not stored.
//                   256 < L <= 512, PRODUCT only (phl_nchw_softmax_compat_wide): the same body on a tile of WIDE_TP = 32
//                   pixels -- 64 KiB at 512 labels, again two workgroups per CU; eight threads per pixel in the softmax;
//                   wave w owns the label tiles w + 4 i of the one pixel half, still at most four accumulators; 128
//                   contiguous bytes per label plane and row in and out; operand B's two lane halves fall on banks 0-31
//                   of rows of their own.  M is read from L2 twice as often per pixel as on the 64-pixel tile.  The
//                   product is summed in two levels, an fma chain per block of WIDE_KB = 32 labels and the blocks added in
//                   order (64 more registers): one chain over 341 labels rounds three to four times as much where Q is
//                   spread, and W amplifies what the labels of a pixel do not share.  The blocks are taken in an order
//                   rotated by the workgroup's index (wide_product).
//   k_nchw_stream   L > 256 (UNIFORM up to 1024, SOFTMAX any): a thread per pixel walks its column in memory, three
//                   reading passes (max, sum, quotient) and for UNIFORM a fourth over its own output.
//   k_nchw_logits   out = -(E0 + G): what CRFasRNN returns after the last iteration.
// No atomics, every sum in a fixed order: a repeated call gives the same bits.  The host side (tile counts, the float4
// predicate, the VEC dispatch, the argument checks) is phl_nchw_common.h's, shared with the other channel-major files.
#include <math.h>

#include "phl_nchw_common.h"

namespace {

constexpr int TP = 64;                 // pixels of a tile; its NT = 256 threads: 4 per pixel in the softmax, 4 waves in the product
constexpr int WIDE_TP = 32;            // pixels of the wide product's tile: 8 threads per pixel in the softmax
constexpr int VALU_MAX_L = 32;         // the product runs on the VALU up to here, on the matrix cores above
constexpr int TILE_MAX_L = 256;        // k_nchw_tile's range on TP pixels
constexpr int WIDE_MAX_L = 512;        // ... and on WIDE_TP pixels (the product on the matrix cores only)
constexpr int WIDE_KB = 32;            // labels of a block of the wide product's two-level sum (a power of two)
constexpr int WIDE_GS = 4;             // k steps (of two labels) whose loads of M are in flight together; 2 WIDE_GS divides WIDE_KB
enum { T_MFMA = 0, T_VALU = 1, T_UNIFORM = 2, T_SOFTMAX = 3 };

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline size_t tile_lds_bytes(int L, int tp) { return ((size_t)((L + 1) & ~1) * tp + 3 * NT) * sizeof(float); }

// red[part][TPX]: the partials of pixel p, combined pairwise in a fixed order -- (r0 . r1) . (r2 . r3) for four of them
template <int PARTS, int TPX, class Op>
__device__ __forceinline__ float combine_parts(const float *red, int p, Op op)
{
    float v[PARTS];
#pragma unroll
    for (int i = 0; i < PARTS; i++) v[i] = red[i * TPX + p];
#pragma unroll
    for (int w = 1; w < PARTS; w *= 2)
#pragma unroll
        for (int i = 0; i < PARTS; i += 2 * w) v[i] = op(v[i], v[i + w]);
    return v[0];
}

// The product of the wide tile for a wave that owns NTL label tiles, ct0 + 4 i: acc[i] = its 32 labels x 32 pixels of
// M^T Q^T.  Three things differ from the 64-pixel tile's loop.
//   The sum has two levels: the fma chain of a block of WIDE_KB labels runs in acc, and acc goes into sum at the end of
//   every block -- at 341 labels one chain's rounding is ~5 u of Y (u = 2^-24) where Q is spread, the blocks' ~1.3 u.
//   The blocks are taken in a rotated order, first = a function of the workgroup's index alone (so a repeated call gives
//   the same bits): workgroups start together and run the same program, and with one order they all ask L2 for the same
//   few rows of M at the same time.  Workgroups b, b + 8, b + 16, .. tend to share an L2 (speed only; nothing relies on it),
//   hence b / 8.
//   The loads of M of WIDE_GS k steps are issued together, before their MFMAs: one k step at a time leaves a wave waiting
//   for L2 once per four MFMAs.
// Rows of M and of S beyond the end are read clamped, and the rows of M count as 0.
template <int NTL>
__device__ __forceinline__ void wide_product(const float *__restrict__ M, const float *S, int L, int La, int ct0, int j, int kh,
                                             f32x16 (&acc)[4])
{
    f32x16 sum[NTL];
    const float *Mc[NTL];
    bool cin[NTL];
#pragma unroll
    for (int i = 0; i < NTL; i++) {
        const int c = 32 * (ct0 + 4 * i) + j;
        cin[i] = c < L;
        Mc[i] = M + (cin[i] ? c : L - 1);
        sum[i] = acc[i];                                         // zeros
    }
    const int nblk = (La + WIDE_KB - 1) / WIDE_KB, first = (int)((blockIdx.x >> 3) % (unsigned)nblk);
    for (int bi = 0; bi < nblk; bi++) {
        const int blk = first + bi < nblk ? first + bi : first + bi - nblk;
        const int kend = (blk + 1) * WIDE_KB < La ? (blk + 1) * WIDE_KB : La;
        for (int k0 = blk * WIDE_KB; k0 < kend; k0 += 2 * WIDE_GS) {
            float av[WIDE_GS][NTL], bv[WIDE_GS];
#pragma unroll
            for (int s = 0; s < WIDE_GS; s++) {
                const int a = k0 + 2 * s + kh, ar = a < L ? a : L - 1;
#pragma unroll
                for (int i = 0; i < NTL; i++) {
                    const float v = Mc[i][ar * L];
                    av[s][i] = (a < L && cin[i]) ? v : 0.f;
                }
            }
#pragma unroll
            for (int s = 0; s < WIDE_GS; s++) {
                const int a = k0 + 2 * s + kh;
                bv[s] = S[(a < La ? a : La - 1) * WIDE_TP + j];
            }
#pragma unroll
            for (int s = 0; s < WIDE_GS; s++)
#pragma unroll
                for (int i = 0; i < NTL; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][i], bv[s], acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NTL; i++) {                          // the block's chain is done
            sum[i] += acc[i];
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < NTL; i++) acc[i] = sum[i];
}

template <int MODE, bool VEC, int TPX = TP>
__global__ __launch_bounds__(NT) void k_nchw_tile(const float *__restrict__ E0, const float *__restrict__ G,
                                                  const float *__restrict__ M, float alpha, float beta,
                                                  float *__restrict__ out, int L, int64_t n, int tiles)
{
    // S [La][TPX]: the tile, La = L rounded up to the MFMA's k step; then three [PARTS][TPX] arrays of per-pixel partials
    static_assert(TPX == TP || (TPX == WIDE_TP && MODE == T_MFMA), "the wide tile is the matrix-core product's");
    constexpr int PARTS = NT / TPX, VROW = TPX / 4;              // threads of a pixel's column, float4s of a tile row
    constexpr int TSH = TPX == 64 ? 6 : 5;                       // log2 TPX
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int La = (L + 1) & ~1;
    float *S = lds, *red_m = lds + La * TPX, *red_s = red_m + NT, *red_c = red_s + NT;
    const int t = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int64_t p0 = (int64_t)tile * TPX, base = (int64_t)b * L * n + p0;
    const int np = (int)(n - p0 < TPX ? n - p0 : TPX);            // pixels of this tile
    const float *e0 = E0 + base, *g = G ? G + base : nullptr;
    float *o = out + base;

    // ---- 1. S = -(E0 + G), coalesced along the pixel axis
    if (VEC) {
        const int q = (t & (VROW - 1)) * 4, r = t >> (TSH - 2);     // n % 4 == 0: a float4 lies inside the image or outside
#pragma unroll 4
        for (int a = r; a < L; a += NT / VROW) {
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < np) {
                x = *reinterpret_cast<const float4 *>(e0 + a * n + q);
                if (g) {
                    const float4 y = *reinterpret_cast<const float4 *>(g + a * n + q);
                    x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
                }
                x = make_float4(-x.x, -x.y, -x.z, -x.w);
            }
            *reinterpret_cast<float4 *>(S + a * TPX + q) = x;
        }
    } else {
        const int q = t & (TPX - 1), r = t >> TSH;
#pragma unroll 4
        for (int a = r; a < L; a += PARTS) {
            float x = 0.f;
            if (q < np) {
                x = e0[a * n + q];
                if (g) x += g[a * n + q];
                x = -x;
            }
            S[a * TPX + q] = x;
        }
    }
    if (MODE == T_MFMA && La != L && t < TPX) S[L * TPX + t] = 0.f;       // the k step's second row at an odd L
    __syncthreads();

    // ---- 2. column softmax: pixel p, labels part, part + PARTS, ... per thread; partials combined in a fixed order
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int p = t & (TPX - 1), part = TPX == 64 ? wave : t >> TSH;
    float m = -INFINITY;
    for (int a = part; a < L; a += PARTS) m = fmaxf(m, S[a * TPX + p]);
    red_m[part * TPX + p] = m;
    __syncthreads();
    m = combine_parts<PARTS, TPX>(red_m, p, [](float x, float y) { return fmaxf(x, y); });
    float s = 0.f;
    for (int a = part; a < L; a += PARTS) {
        const float e = expf(S[a * TPX + p] - m);
        S[a * TPX + p] = e;
        s += e;
    }
    red_s[part * TPX + p] = s;
    __syncthreads();
    s = combine_parts<PARTS, TPX>(red_s, p, [](float x, float y) { return x + y; });
    const float inv = 1.0f / s;
    float cs = 0.f;
    for (int a = part; a < L; a += PARTS) {
        const float qv = S[a * TPX + p] * inv;
        S[a * TPX + p] = qv;
        cs += qv;
    }
    if (MODE == T_UNIFORM) {         // Y = alpha colsum(Q) + beta Q: every thread rewrites the labels it owns
        red_c[part * TPX + p] = cs;
        __syncthreads();
        cs = alpha * combine_parts<PARTS, TPX>(red_c, p, [](float x, float y) { return x + y; });
        for (int a = part; a < L; a += PARTS) S[a * TPX + p] = cs + beta * S[a * TPX + p];
    }
    __syncthreads();                 // S = Q (UNIFORM: Y already)

    // ---- 3. Y[c][p] = sum_a M[a][c] Q[a][p], an fma chain in a order, back into S
    if (MODE == T_VALU) {
        float y[VALU_MAX_L / 4];
#pragma unroll
        for (int i = 0; i < VALU_MAX_L / 4; i++) {
            const int c = part + 4 * i;                          // wave-uniform: M comes through scalar loads
            y[i] = 0.f;
            if (c < L)
                for (int a = 0; a < L; a++) y[i] = __builtin_fmaf(M[a * L + c], S[a * TPX + p], y[i]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VALU_MAX_L / 4; i++)
            if (part + 4 * i < L) S[(part + 4 * i) * TPX + p] = y[i];
        __syncthreads();
    }
    if (MODE == T_MFMA) {
        const int j = t & 31, kh = (t >> 5) & 1;                 // 32x32x2: A[i = j][k = kh], B[k = kh][column j]
        constexpr int PH = TPX / 32;                             // pixel halves; a wave owns one, and every (4 / PH)-th label tile
        const int ph = wave & (PH - 1), ct0 = wave >> (PH - 1), nct = (L + 31) >> 5;
        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
        if constexpr (TPX == WIDE_TP) {
            switch (ct0 < nct ? (nct - ct0 + 3) >> 2 : 0) {          // the label tiles of this wave: a branch-free loop for each count
            case 1: wide_product<1>(M, S, L, La, ct0, j, kh, acc); break;
            case 2: wide_product<2>(M, S, L, La, ct0, j, kh, acc); break;
            case 3: wide_product<3>(M, S, L, La, ct0, j, kh, acc); break;
            case 4: wide_product<4>(M, S, L, La, ct0, j, kh, acc); break;
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < La; k += 2) {
                const int a = k + kh;
                const float bv = S[a * TPX + 32 * ph + j];
                const int ar = a < L ? a : L - 1;                    // loads stay inside M; what lies beyond L counts as 0
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int ct = ct0 + (4 / PH) * i;
                    if (ct < nct) {
                        const int c = 32 * ct + j;
                        float av = M[ar * L + (c < L ? c : L - 1)];
                        av = (a < L && c < L) ? av : 0.f;
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();             // every wave has read its Q
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ct = ct0 + (4 / PH) * i;
            if (ct < nct) {
#pragma unroll
                for (int r = 0; r < 16; r++) {                   // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                    const int c = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (c < L) S[c * TPX + 32 * ph + j] = acc[i][r];
                }
            }
        }
        __syncthreads();
    }

    // ---- 4. store, as loaded
    if (VEC) {
        const int q = (t & (VROW - 1)) * 4, r = t >> (TSH - 2);
        if (q < np)
#pragma unroll 4
            for (int a = r; a < L; a += NT / VROW) *reinterpret_cast<float4 *>(o + a * n + q) = *reinterpret_cast<const float4 *>(S + a * TPX + q);
    } else {
        const int q = t & (TPX - 1), r = t >> TSH;
        if (q < np)
#pragma unroll 4
            for (int a = r; a < L; a += PARTS) o[a * n + q] = S[a * TPX + q];
    }
}

// Columns longer than an LDS tile: a thread per pixel, the column read from memory in every pass (consecutive threads on
// consecutive pixels of a label plane).  The arithmetic is k_nchw_tile's with one partial instead of four.
template <bool UNIFORM>
__global__ __launch_bounds__(NT) void k_nchw_stream(const float *__restrict__ E0, const float *__restrict__ G, float alpha,
                                                    float beta, float *__restrict__ out, int L, int64_t n, int tiles)
{
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int64_t p = (int64_t)tile * NT + threadIdx.x;
    if (p >= n) return;
    const int64_t base = (int64_t)b * L * n + p;
    const float *e0 = E0 + base, *g = G ? G + base : nullptr;
    float *o = out + base;
    float m = -INFINITY;
    for (int a = 0; a < L; a++) m = fmaxf(m, -(e0[a * n] + (g ? g[a * n] : 0.f)));
    float s = 0.f;
    for (int a = 0; a < L; a++) s += expf(-(e0[a * n] + (g ? g[a * n] : 0.f)) - m);
    const float inv = 1.0f / s;
    float cs = 0.f;
    for (int a = 0; a < L; a++) {
        const float qv = expf(-(e0[a * n] + (g ? g[a * n] : 0.f)) - m) * inv;
        o[a * n] = qv;
        cs += qv;
    }
    if (UNIFORM) {
        cs *= alpha;
        for (int a = 0; a < L; a++) o[a * n] = cs + beta * o[a * n];       // the thread's own stores
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void k_nchw_logits(const float *__restrict__ E0, const float *__restrict__ G,
                                                    float *__restrict__ out, int64_t count)       // count: float4s if VEC
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < count; i += stride) {
        if (VEC) {
            const float4 e = reinterpret_cast<const float4 *>(E0)[i], y = reinterpret_cast<const float4 *>(G)[i];
            reinterpret_cast<float4 *>(out)[i] = make_float4(-(e.x + y.x), -(e.y + y.y), -(e.z + y.z), -(e.w + y.w));
        } else {
            out[i] = -(E0[i] + G[i]);
        }
    }
}

template <int MODE, int TPX = TP>
int launch_tile(const float *E0, const float *G, const float *M, float alpha, float beta, float *out, int B, int L, int64_t n,
                hipStream_t st)
{
    const int tiles = nchw_tiles(n, TPX);
    const size_t lds = tile_lds_bytes(L, TPX);
    return nchw_dispatch(nchw_vec(n, {E0, G, out}), false, [&](auto vec, auto) -> int {
        constexpr bool VEC = decltype(vec)::value;
        if (const int rc = phl_allow_lds(&k_nchw_tile<MODE, VEC, TPX>, lds)) return rc;
        k_nchw_tile<MODE, VEC, TPX><<<nchw_grid(B, tiles), dim3(NT), lds, st>>>(E0, G, M, alpha, beta, out, L, n, tiles);
        PHL_HIP(hipGetLastError());
        return PHL_OK;
    });
}

}  // namespace

extern "C" {

int phl_nchw_softmax_compat(const float *E0, const float *G, const float *mu, float alpha, float beta, float *out, int B, int L,
                            int64_t n, int mode, phl_stream stream)
{
    const char *who = "phl_nchw_softmax_compat";
    const bool known = mode == PHL_NCHW_PRODUCT || mode == PHL_NCHW_UNIFORM || mode == PHL_NCHW_SOFTMAX || mode == PHL_NCHW_LOGITS;
    const bool bad = B < 0 || n < 0 || L < 1 || !known || (mode == PHL_NCHW_UNIFORM && !(isfinite(alpha) && isfinite(beta)));
    const int px = mode == PHL_NCHW_LOGITS ? 0 : L > TILE_MAX_L ? NT : TP;      // pixels of a workgroup (the logits' grid is capped)
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld mode=%d alpha=%g beta=%g", B, L, (long long)n, mode, (double)alpha, (double)beta).s,
                   bad, B == 0 || n == 0, {E0, out, mode == PHL_NCHW_PRODUCT ? mu : out, mode == PHL_NCHW_LOGITS ? G : out},
                   mode == PHL_NCHW_PRODUCT ? "E0 / out / mu" : mode == PHL_NCHW_LOGITS ? "E0 / out / G" : "E0 / out", {E0, G}, out,
                   "out", B, L, n, px, rc))
        return rc;
    if ((mode == PHL_NCHW_PRODUCT && L > TILE_MAX_L) || (mode == PHL_NCHW_UNIFORM && L > 1024)) {
        phl_set_error("%s: %d labels, at most %d in this mode", who, L, mode == PHL_NCHW_PRODUCT ? TILE_MAX_L : 1024);
        return PHL_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (mode == PHL_NCHW_LOGITS) {
        const int64_t total = (int64_t)B * L * n;
        const bool vec = nchw_vec(total, {E0, G, out});
        const int64_t count = vec ? total / 4 : total, want = (count + NT - 1) / NT;
        const dim3 grid((unsigned)(want < 65536 ? want : 65536));
        if (vec) k_nchw_logits<true><<<grid, dim3(NT), 0, st>>>(E0, G, out, count);
        else k_nchw_logits<false><<<grid, dim3(NT), 0, st>>>(E0, G, out, count);
        PHL_HIP(hipGetLastError());
        return PHL_OK;
    }
    if (L > TILE_MAX_L) {
        const int tiles = nchw_tiles(n, NT);
        if (mode == PHL_NCHW_UNIFORM) k_nchw_stream<true><<<nchw_grid(B, tiles), dim3(NT), 0, st>>>(E0, G, alpha, beta, out, L, n, tiles);
        else k_nchw_stream<false><<<nchw_grid(B, tiles), dim3(NT), 0, st>>>(E0, G, alpha, beta, out, L, n, tiles);
        PHL_HIP(hipGetLastError());
        return PHL_OK;
    }
    if (mode == PHL_NCHW_UNIFORM) return launch_tile<T_UNIFORM>(E0, G, nullptr, alpha, beta, out, B, L, n, st);
    if (mode == PHL_NCHW_SOFTMAX) return launch_tile<T_SOFTMAX>(E0, G, nullptr, 0.f, 0.f, out, B, L, n, st);
    if (L <= VALU_MAX_L) return launch_tile<T_VALU>(E0, G, mu, 0.f, 0.f, out, B, L, n, st);
    return launch_tile<T_MFMA>(E0, G, mu, 0.f, 0.f, out, B, L, n, st);
}

int phl_nchw_softmax_compat_wide(const float *E0, const float *G, const float *mu, float *out, int B, int L, int64_t n,
                                 phl_stream stream)
{
    const char *who = "phl_nchw_softmax_compat_wide";
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0, {E0, out, mu},
                   "E0 / out / mu", {E0, G}, out, "out", B, L, n, L > TILE_MAX_L ? WIDE_TP : TP, rc))
        return rc;
    if (L > WIDE_MAX_L) {
        phl_set_error("%s: %d labels, at most %d", who, L, WIDE_MAX_L);
        return PHL_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (L <= VALU_MAX_L) return launch_tile<T_VALU>(E0, G, mu, 0.f, 0.f, out, B, L, n, st);
    if (L <= TILE_MAX_L) return launch_tile<T_MFMA>(E0, G, mu, 0.f, 0.f, out, B, L, n, st);
    return launch_tile<T_MFMA, WIDE_TP>(E0, G, mu, 0.f, 0.f, out, B, L, n, st);
}

}  // extern "C"
