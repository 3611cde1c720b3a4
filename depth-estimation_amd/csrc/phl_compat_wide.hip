// phl_compat_wide.hip -- the fused mean-field step out = softmax(-(E0 + X @ Mu)) for 256 < L <= 512 labels.
//
// k_compat_split (phl_meanfield.hip) carries a whole 256-label row of 32 pixels per wave in 128 accumulator registers;
// a 512-label row of 32 pixels does not fit.  This kernel keeps the split-operand arithmetic and changes the shape:
//
//  * arithmetic after k_compat_split: both operands split into three bf16 addends by truncation (split3, exact), partial
//    products on v_mfma_f32_16x16x32_bf16 accumulated in f32, the softmax on the accumulators.  Two differences, both for
//    accuracy at these label counts, where energies reach the hundreds: EIGHT of the nine products (hH + hM + mH + hL +
//    lH + mM + mL + lM; the dropped ones of k_compat_split are biased -- truncation remainders share the operand's
//    sign), and the accumulators start at zero, E0 is added to the finished product.  Measured on the mean-field check
//    at 341 labels (tests/test_gpu_crf_api.py, max |Q - Q_torch|): six products on top of E0 4.57e-5, eight on top of
//    E0 4.35e-5, six then E0 4.01e-5, eight then E0 3.92e-5 (the bound is 4e-5); 4.44 -> 5.06 ms at 3,145,728 x 344.
//    Neither G = X @ Mu nor E exists in HBM: E0 and X are read once, Q is written once.
//  * shape: a wave owns 16 pixels x the whole row (Lp = L rounded up to 32, NL = Lp / 16 label tiles of 16, at most 32
//    tiles = 128 accumulator registers), so the softmax and the epilogue map are those of the 256-label kernels for one
//    pixel group.  The product is transposed (labels = MFMA rows): lane (i, g4) holds labels 16T + 4g4 .. +3 of pixel i,
//    a pixel's row sits in lanes i + 16 g4.  Matrix work scales with Lp^2 (344 runs as 352), not with a 512 tile.
//  * a workgroup is four waves (64 pixels, one tile), two workgroups per CU (<= 256 VGPRs, 72 KiB of LDS each): the
//    epilogue of one (softmax, Q stores, the next tile's E0) overlaps the other's MFMA stream without any choreography.
//  * the compatibility matrix arrives PREPARED (k_compat_wide_planes): piece (K chunk kc of 32, label quarter q of 8
//    tiles) = [tile][plane][lane] x 16 B = 24 KiB, the format of k_compat_split's pieces.  A slot is one piece; the four
//    waves fetch it by LDS-DMA (six 1 KiB units each) two slots ahead into a ring of three, and every slot ends in the
//    workgroup barrier.  Operand reads are lane-linear (no bank conflict).  The last quarter of a row may hold fewer than
//    8 real tiles: its piece is fetched whole (zeros), only the real tiles are multiplied.
//  * X comes straight from global memory into registers (two 16-byte loads per lane and chunk, a chunk ahead), split
//    once per chunk and kept across the chunk's NQ slots.
//  * columns above L are padding: planes zero there, E0 reads as +inf, X fetches clamped into the row and zeroed when
//    consumed, nothing stored (only the last K chunk and the last two label tiles can hold padding: Lp - L < 32).
//  * the last n % 64 rows go to k_compat_wide_tail (one workgroup per pixel, f64 dot product from mu_t).
#include <math.h>

#include "phl_internal.h"
#include "phl_compat_common.h"

namespace {

constexpr int CW_PIECE = 24576;                  // bytes of one slot's piece of the planes: 8 tiles x 3 planes x 64 lanes x 16 B
constexpr int CW_TILE = 64;                      // pixels per workgroup (4 waves x 16)

// MuT [Lp][Lp] f32 (zero beyond the real label count) -> planes: piece kc * NQ + q, label tile Tl of the quarter, plane P,
// lane (i, g): eight bf16 = plane P of MuT[16 (8 q + Tl) + i][32 kc + 8 g .. + 7]; zero for labels >= Lp
__global__ __launch_bounds__(256) void k_compat_wide_planes(const float *__restrict__ MuT, int Lp, int NQ, u32x4 *__restrict__ planes)
{
    const int t = blockIdx.x * 256 + threadIdx.x;           // one thread per (piece, Tl, lane)
    const int npieces = Lp / 32 * NQ;
    if (t >= npieces * 8 * 64) return;
    const int lane = t & 63, Tl = (t >> 6) & 7, piece = t >> 9, kc = piece / NQ, q = piece - kc * NQ;
    const int label = 16 * (8 * q + Tl) + (lane & 15), k0 = 32 * kc + 8 * (lane >> 4);
    const bool in = label < Lp && k0 < Lp;                  // (Lp is a multiple of 32: a lane's eight values are all in or all out)
    const float *src = MuT + (size_t)(in ? label : 0) * Lp + (in ? k0 : 0);
    u32x4 h, m, l;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        unsigned a, b, c;
        split3(in ? src[2 * j] : 0.f, in ? src[2 * j + 1] : 0.f, a, b, c);
        h[j] = a; m[j] = b; l[j] = c;
    }
    u32x4 *dst = planes + (size_t)piece * (CW_PIECE / 16) + (size_t)Tl * 3 * 64 + lane;
    dst[0] = h;
    dst[64] = m;
    dst[128] = l;
}

// NT = Lp / 32 K chunks (9 .. 16); Lr = the real label count (a multiple of 4, Lp - 32 < Lr <= Lp).  One tile of 64 whole
// rows per workgroup (the launcher passes n / 64 workgroups).
template <int NT, bool LOGITS>
__global__ __launch_bounds__(256, 2) void k_compat_wide(const float *__restrict__ E0, int64_t e_rs,
                                                        const float *__restrict__ X, int64_t x_rs,
                                                        const unsigned char *__restrict__ planes, float *__restrict__ out,
                                                        int64_t o_rs, int Lr)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int NL = 2 * NT, NQ = (NL + 7) / 8, S = NT * NQ;     // label tiles, label quarters (pieces per chunk), slots
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int w4 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g4 = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * CW_TILE + w4 * 16;     // the wave's first pixel
    const float *erow = E0 + p0 * e_rs;
    const char *xrow = reinterpret_cast<const char *>(X + p0 * x_rs);
    float *orow = out + p0 * o_rs;
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)lds;
    const char *ldsb = reinterpret_cast<const char *>(lds);

    // piece -> ring buffer b: the wave's six 1 KiB units (the four waves together move the 24 units of a piece)
    const unsigned char *wplanes = planes + w4 * 6 * 1024;
    auto fetch = [&](int piece, int b) {
        const unsigned char *src = wplanes + (size_t)piece * CW_PIECE;
        const unsigned dst = lds_base + b * CW_PIECE + w4 * 6 * 1024;
#pragma unroll
        for (int r = 0; r < 6; r++) glds16(reinterpret_cast<const float *>(src + r * 1024), (unsigned)lane * 16u, dst + r * 1024);
        asm volatile("" ::: "memory");           // the X loads of the slot stay behind the DMAs (counted waits)
    };
    // X of chunk kc: k-parts 2 g4, 2 g4 + 1 of the lane's pixel, clamped into the row (zeroed where it is padding, at the chunk's split)
    const unsigned xlo = (unsigned)(i * x_rs) * 4u;
    auto load_x = [&](int kc, float4 &v0, float4 &v1) {
        const int c0 = min(32 * kc + 8 * g4, Lr - 4), c1 = min(32 * kc + 8 * g4 + 4, Lr - 4);
        v0 = *reinterpret_cast<const float4 *>(xrow + xlo + c0 * 4);
        v1 = *reinterpret_cast<const float4 *>(xrow + xlo + c1 * 4);
    };

    f32x4 acc[NL];
    const unsigned lo_e = (unsigned)(i * e_rs) * 4u, lo_o = (unsigned)(i * o_rs) * 4u;

    // prologue: the first two pieces, X of chunk 0 (the tile's E0 is added to the finished product, see the top)
    fetch(0, 0);
    fetch(1, 1);
    auto load_e0 = [&](f32x4 (&dst)[NL]) {
#pragma unroll
        for (int T = 0; T < NL; T++) {
            const int c = min(16 * T + 4 * g4, Lr - 4);
            const float4 v = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(erow) + lo_e + c * 4);
            dst[T] += f32x4{v.x, v.y, v.z, v.w};
            if ((T & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // eight tiles' loads in flight at a time: no spill at 512
        }
#pragma unroll
        for (int T = NL - 2; T < NL; T++)
            if (16 * T + 4 * g4 >= Lr) dst[T] = f32x4{INFINITY, INFINITY, INFINITY, INFINITY};
    };
#pragma unroll
    for (int T = 0; T < NL; T++) acc[T] = 0.f;
    float4 xr0, xr1;
    load_x(0, xr0, xr1);
    dma_drain();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    u32x4 xh, xm, xl;                              // the chunk's X operand, split
    for (int kc = 0; kc < NT; kc++) {
        static_for<NQ>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const int s = kc * NQ + q;
            if (q == 0) {
                if (32 * kc + 8 * g4 >= Lr) xr0 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (32 * kc + 8 * g4 + 4 >= Lr) xr1 = make_float4(0.f, 0.f, 0.f, 0.f);
                unsigned h_[4], m_[4], l_[4];
                split3(xr0.x, xr0.y, h_[0], m_[0], l_[0]);
                split3(xr0.z, xr0.w, h_[1], m_[1], l_[1]);
                split3(xr1.x, xr1.y, h_[2], m_[2], l_[2]);
                split3(xr1.z, xr1.w, h_[3], m_[3], l_[3]);
                xh = u32x4{h_[0], h_[1], h_[2], h_[3]};
                xm = u32x4{m_[0], m_[1], m_[2], m_[3]};
                xl = u32x4{l_[0], l_[1], l_[2], l_[3]};
            }
            // the piece of slot s + 2 into the buffer slot s - 1 read (everybody is past that slot's barrier); past the
            // end a valid piece again, into a buffer nobody reads any more, so that every slot's wait count is the same
            fetch(s + 2 < S ? s + 2 : S - 1, (s + 2) % 3);
            if (q == 0) load_x(kc + 1 < NT ? kc + 1 : NT - 1, xr0, xr1);     // (the last chunk re-reads itself)
            const char *ab = ldsb + (s % 3) * CW_PIECE + lane * 16;
            constexpr int NTL = NL - 8 * q < 8 ? NL - 8 * q : 8;            // real label tiles of this quarter
            u32x4 pa[2][3];
            auto read_a = [&](int j, u32x4 (&dst)[3]) {
#pragma unroll
                for (int P = 0; P < 3; P++) dst[P] = *reinterpret_cast<const u32x4 *>(ab + (j * 3 + P) * 1024);
            };
            read_a(0, pa[0]);
#pragma unroll
            for (int j = 0; j < NTL; j++) {
                if (j + 1 < NTL) read_a(j + 1, pa[(j + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                u32x4(&pc)[3] = pa[j & 1];
                f32x4 &a = acc[8 * q + j];
                // smallest terms first: L m, M l, L h, M m, H l, M h, H m, H h
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[2]), __builtin_bit_cast(bf16x8, xm), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[1]), __builtin_bit_cast(bf16x8, xl), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[2]), __builtin_bit_cast(bf16x8, xh), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[1]), __builtin_bit_cast(bf16x8, xm), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[0]), __builtin_bit_cast(bf16x8, xl), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[1]), __builtin_bit_cast(bf16x8, xh), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[0]), __builtin_bit_cast(bf16x8, xm), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pc[0]), __builtin_bit_cast(bf16x8, xh), a, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // what slot s + 1 reads was requested in slot s - 1 (or the prologue).  vmcnt counts in issue order, so what
            // this wave issued behind it may stay in flight: the X loads of slot s - 1 (if it began a chunk, q == 1), the
            // six units of slot s and the X loads of slot s (q == 0)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 + (q <= 1 ? 2 : 0)) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        });
    }

    load_e0(acc);                          // E = E0 + X @ Mu: E0 added to the finished product
    if (!LOGITS) {
        // softmax(-E) of the lane's pixel: shift by the row MINIMUM of E; exp(-(E - min)) = exp2((E - min) * -log2e), the
        // difference taken first.  The one-fma form of the 256-label kernels, exp2(fma(E, -log2e, min log2e)), is as
        // accurate: the fma is fused, and the rounding of min log2e is common to the row and cancels in the normalisation
        // (measured up to |E| = 7.65e4: those kernels' Q equals an exact softmax of their own E to the printed digits,
        // tests/test_gpu_energy_range.py).  The ~3e-5 = ulp(300) relative in Q they lose at energies in the hundreds comes
        // from accumulating the product ON TOP OF E0; here E0 is added to the finished product
        float m = acc[0][0];
        m = vmin3(m, acc[0][1], acc[0][2]);
#pragma unroll
        for (int T = 1; T < NL; T++) {
            m = vmin3(m, acc[T][0], acc[T][1]);
            m = vmin3(m, acc[T][2], acc[T][3]);
        }
        m = vmin3(m, acc[0][3], acc[0][3]);
        {
            float ma = m, mb = m;
            PHL_ROW_SWAP(ma, mb);
            m = vmin3(ma, mb, mb);
            ma = m; mb = m;
            PHL_HALF_SWAP(ma, mb);
            m = vmin3(ma, mb, mb);
        }
        f32x4 vs = 0.f;
#pragma unroll
        for (int T = 0; T < NL; T++) {
            acc[T] = (acc[T] - (f32x4)m) * (f32x4)(-1.4426950408889634f);
#pragma unroll
            for (int r = 0; r < 4; r++) acc[T][r] = __builtin_amdgcn_exp2f(acc[T][r]);
            vs += acc[T];
        }
        float sum = (vs[0] + vs[1]) + (vs[2] + vs[3]);
        {
            float sa = sum, sb = sum;
            PHL_ROW_SWAP(sa, sb);
            sum = sa + sb;
            sa = sum; sb = sum;
            PHL_HALF_SWAP(sa, sb);
            sum = sa + sb;
        }
        const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int T = 0; T < NL; T++) acc[T] *= inv;
    } else {                                     // CRFasRNN returns -E of the last iteration, not Q (crf_module.py:103)
#pragma unroll
        for (int T = 0; T < NL; T++) acc[T] = -acc[T];
    }
#pragma unroll
    for (int T = 0; T < NL; T++)
        if (T < NL - 2 || 16 * T + 4 * g4 < Lr)
            *reinterpret_cast<float4 *>(reinterpret_cast<char *>(orow + 16 * T) + lo_o + 16 * g4) =
                make_float4(acc[T][0], acc[T][1], acc[T][2], acc[T][3]);
    dma_drain();                                 // the last fetches nobody reads: landed before the LDS is given back
}

// The last n % 64 pixels (the tile kernel takes whole tiles only): one workgroup per pixel, thread c owns label c -- the
// dot product over k straight from the transposed compatibility matrix, accumulated in f64 and rounded once (at most 63
// rows: its speed does not matter; an f32 chain over 512 terms would carry more error than the tile kernel's
// accumulation), then the row softmax through LDS (the tile kernel's exponent form).
template <bool LOGITS>
__global__ __launch_bounds__(512) void k_compat_wide_tail(const float *__restrict__ E0, int64_t e_rs, const float *__restrict__ X,
                                                          int64_t x_rs, const float *__restrict__ MuT, int Lp,
                                                          float *__restrict__ out, int64_t o_rs, int64_t p0, int L)
{
    __shared__ float xs[512], red[512];
    const int64_t p = p0 + blockIdx.x;
    const int c = threadIdx.x;
    xs[c] = c < L ? X[p * x_rs + c] : 0.f;
    __syncthreads();
    float e = INFINITY;
    if (c < L) {
        double d = E0[p * e_rs + c];
        for (int k = 0; k < L; k++) d = __builtin_fma((double)xs[k], (double)MuT[(int64_t)c * Lp + k], d);
        e = (float)d;
    }
    if (LOGITS) {
        if (c < L) out[p * o_rs + c] = -e;
        return;
    }
    red[c] = e;
    __syncthreads();
    for (int o = 256; o > 0; o >>= 1) {
        if (c < o) red[c] = fminf(red[c], red[c + o]);
        __syncthreads();
    }
    const float m = red[0];
    __syncthreads();
    const float v = c < L ? __builtin_amdgcn_exp2f((e - m) * -1.4426950408889634f) : 0.f;
    red[c] = v;
    __syncthreads();
    for (int o = 256; o > 0; o >>= 1) {
        if (c < o) red[c] += red[c + o];
        __syncthreads();
    }
    if (c < L) out[p * o_rs + c] = v * __builtin_amdgcn_rcpf(red[0]);
}

inline int wide_nq(int Lp) { return (Lp / 16 + 7) / 8; }

}  // namespace

// Host side, called by phl_compat_planes_bytes / phl_compat_prepare / phl_compat_softmax_split (phl_meanfield.hip) for
// 256 < L <= 512; argument checks are theirs.
size_t phl_compat_wide_planes_bytes(int L)
{
    if (L <= 256 || L > 512 || L % 4) return 0;
    const int Lp = (L + 31) / 32 * 32;
    return (size_t)(Lp / 32) * wide_nq(Lp) * CW_PIECE;
}

int phl_compat_wide_prepare(const float *MuT, int L, void *planes, hipStream_t st)
{
    const int Lp = (L + 31) / 32 * 32, nthreads = Lp / 32 * wide_nq(Lp) * 8 * 64;
    k_compat_wide_planes<<<dim3((nthreads + 255) / 256), dim3(256), 0, st>>>(MuT, Lp, wide_nq(Lp), reinterpret_cast<u32x4 *>(planes));
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

int phl_compat_wide_softmax(const float *E0, int64_t e_rs, const float *X, int64_t x_rs, const float *MuT, const void *planes,
                            float *out, int64_t o_rs, int64_t n, int L, bool logits, hipStream_t st)
{
    const int Lp = (L + 31) / 32 * 32;
    const int64_t ntiles = n / CW_TILE, n_main = ntiles * CW_TILE;
    const size_t lds = (size_t)3 * CW_PIECE;     // ring of three pieces: 72 KiB, two workgroups per CU
#define PHL_CW_LAUNCH(NT_, LG_)                                                                                           \
    do {                                                                                                                  \
        if (const int rc = phl_allow_lds(&k_compat_wide<NT_, LG_>, lds)) return rc;                                       \
        k_compat_wide<NT_, LG_><<<dim3((unsigned)ntiles), dim3(256), lds, st>>>(                                          \
            E0, e_rs, X, x_rs, reinterpret_cast<const unsigned char *>(planes), out, o_rs, L);                            \
    } while (0)
#define PHL_CW(NT_)                                                                                                       \
    case NT_:                                                                                                             \
        if (logits) PHL_CW_LAUNCH(NT_, true);                                                                             \
        else PHL_CW_LAUNCH(NT_, false);                                                                                   \
        break;
    if (ntiles > 0) {
        switch (Lp / 32) {
            PHL_CW(9) PHL_CW(10) PHL_CW(11) PHL_CW(12) PHL_CW(13) PHL_CW(14) PHL_CW(15) PHL_CW(16)
        }
    }
#undef PHL_CW
#undef PHL_CW_LAUNCH
    if (n > n_main) {
        if (logits) k_compat_wide_tail<true><<<dim3((unsigned)(n - n_main)), dim3(512), 0, st>>>(E0, e_rs, X, x_rs, MuT, Lp, out, o_rs, n_main, L);
        else k_compat_wide_tail<false><<<dim3((unsigned)(n - n_main)), dim3(512), 0, st>>>(E0, e_rs, X, x_rs, MuT, Lp, out, o_rs, n_main, L);
    }
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}
