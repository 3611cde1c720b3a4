// phl_nchw_train.hip -- the non-W half of a mean-field iteration on channel-major data for TRAINING: the step of
// phl_nchw.hip and its backward, 1 <= L <= PHL_NCHW_TRAIN_MAX_L = 64 labels (the reference trains at 18 and at w / 6 = 60).
//
//     forward    Q_a = softmax_a(-(E0_a + G_a))  (G optional),     Y_c = sum_a M[a][c] Q_a
//     backward   t_a = sum_c M[a][c] gY_c,   s = sum_a Q_a t_a,    dE_a = Q_a (s - t_a)     (the gradient of E0 and of G alike)
//                gM[a][c] = sum over images and pixels of Q_a gY_c
//
// per pixel column; M is the dense [L][L] matrix of the _compat_matrix convention.  The backward needs nothing but the
// forward's inputs and gY: Q is recomputed.
//
//   k_step_train   A workgroup of NT = 256 threads owns tiles of TP = 64 consecutive pixels of one image and all L labels
//                  of them: the forward one tile, the backward tiles blockIdx.x, blockIdx.x + gridDim.x, ...  LDS:
//                    Qd  double [L][TP]       -(E0 + G), then Q                                  32 KiB at 64 labels
//                    red double [2][4][TP]    a pixel's four partials (maximum, sum; the backward's s)     4 KiB
//                    F   float  [L][TP + 1]   the backward's gY, then the result on its way out       16.25 KiB
//                  52.25 KiB at 64 labels: two workgroups per CU.  Thread t owns pixel p = t % 64 and the labels wave,
//                  wave + 4, ...: at most 16.  Loads and stores run along the pixel axis through LDS, 256 contiguous bytes
//                  per label plane: float4 accesses when n % 4 == 0 and every volume pointer is 16-byte aligned, dwords
//                  otherwise; pixels past the end of an image load as zeros and are not stored.
//                    softmax   max-subtracted, in double; the four partials of a pixel combined (r0 . r1) . (r2 . r3)
//                    product   acc[i] = sum_k M[..] * src[k][p], an fma chain in k order in double: the forward with k = a
//                              over Qd, the backward with k = c over F -- ONE function, instantiated twice.  The labels
//                              the wave owns are wave-uniform, so M comes through scalar loads: k_step_train_mu lays it
//                              out once per call as doubles, the 16 values a wave needs at step k side by side
//                              (stream-ordered scratch, 32 KiB at 64 labels), so a step is two 64-byte scalar loads
//                              whose registers are the fma's operands as they are.  The other operand is read along
//                              the pixel axis (no bank conflict).  The chain is instantiated for every label count of a
//                              wave (1 .. 16): no guard inside it.  (M read as floats where it lies, one dword and one
//                              conversion per fma, took 2.4 times as long at 64 labels.)
//                    gM        thread t owns column c = t % 64 and the rows wave, wave + 4, ...: 16 (a, c) pairs, summed
//                              over the tile's pixels in double and kept in registers across all tiles of the workgroup.
//                              Q[a][p] is one address per wave (a broadcast); gY[c][p] has the label varying across the
//                              lanes, which is why F's rows are TP + 1 floats: bank (c + p) % 64, no conflict.  A zero gY
//                              keeps the pixels past the end of an image out of the sum.  At the end the workgroup writes
//                              one [L][L] double partial.
//   k_step_train_sum   adds the R partials in index order in double and stores fp32 (16 loads in flight per thread).
// Between the fp32 loads and the fp32 stores everything is float64 (as phl_nchw_expect.hip and phl_nchw_scalar.hip): every
// output is the float64 result rounded once.  No atomics, every sum in a fixed order, R a function of (B, L, n) alone: a
// repeated call gives the same bits.
#include <math.h>

#include "phl_nchw_common.h"

namespace {

constexpr int TP = 64;                             // pixels of a tile
constexpr int MAX_L = PHL_NCHW_TRAIN_MAX_L;
constexpr int OWN = MAX_L / 4;                     // labels of a thread (of a wave): wave, wave + 4, ...
constexpr int FS = TP + 1;                         // row stride of F
constexpr int MAX_PARTIALS = 1024;                 // workgroups of a backward that wants gM: 32 MiB of partials at 64 labels
static_assert(NT == 4 * TP && OWN * 4 == MAX_L, "four waves, one pixel per lane");

inline size_t train_lds_bytes(int L) { return (size_t)L * TP * sizeof(double) + 2 * NT * sizeof(double) + (size_t)L * FS * sizeof(float); }

// red[part][TP]: the four partials of pixel p, (r0 . r1) . (r2 . r3)
template <class Op>
__device__ __forceinline__ double combine4(const double *red, int p, Op op)
{
    return op(op(red[p], red[TP + p]), op(red[2 * TP + p], red[3 * TP + p]));
}

// Qd = -(E0 + G) (exact in double) and, for the backward, F = gY, along the pixel axis; zeros beyond np pixels
template <bool VEC, bool BACK>
__device__ __forceinline__ void load_tile(const float *e0, const float *g, const float *gy, int L, int64_t n, int np, double *Qd,
                                          float *F, int t)
{
    if (VEC) {
        const int q = (t & 15) * 4, r = t >> 4;                  // n % 4 == 0: a float4 lies inside the image or outside
        for (int a = r; a < L; a += NT / 16) {
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x, u = x;
            if (q < np) {
                x = *reinterpret_cast<const float4 *>(e0 + a * n + q);
                if (g) y = *reinterpret_cast<const float4 *>(g + a * n + q);
                if (BACK) u = *reinterpret_cast<const float4 *>(gy + a * n + q);
            }
            double *d = Qd + a * TP + q;
            d[0] = -((double)x.x + (double)y.x);
            d[1] = -((double)x.y + (double)y.y);
            d[2] = -((double)x.z + (double)y.z);
            d[3] = -((double)x.w + (double)y.w);
            if (BACK) {
                float *f = F + a * FS + q;
                f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w;
            }
        }
    } else {
        const int q = t & (TP - 1), r = t >> 6;
        for (int a = r; a < L; a += NT / TP) {
            float x = 0.f, y = 0.f, u = 0.f;
            if (q < np) {
                x = e0[a * n + q];
                if (g) y = g[a * n + q];
                if (BACK) u = gy[a * n + q];
            }
            Qd[a * TP + q] = -((double)x + (double)y);
            if (BACK) F[a * FS + q] = u;
        }
    }
}

// the tile's result, F, to memory the way the input was loaded
template <bool VEC>
__device__ __forceinline__ void store_tile(float *o, int L, int64_t n, int np, const float *F, int t)
{
    if (VEC) {
        const int q = (t & 15) * 4, r = t >> 4;
        if (q < np)
            for (int a = r; a < L; a += NT / 16) {
                const float *f = F + a * FS + q;
                *reinterpret_cast<float4 *>(o + a * n + q) = make_float4(f[0], f[1], f[2], f[3]);
            }
    } else {
        const int q = t & (TP - 1), r = t >> 6;
        if (q < np)
            for (int a = r; a < L; a += NT / TP) o[a * n + q] = F[a * FS + q];
    }
}

// Qd: -(E0 + G) -> Q, the column softmax of pixel p; the thread's labels are part, part + 4, ...  Ends behind a barrier.
__device__ __forceinline__ void softmax_tile(double *Qd, double *red, int L, int p, int part)
{
    double *red_m = red, *red_s = red + NT;
    double m = -INFINITY;
    for (int a = part; a < L; a += 4) m = fmax(m, Qd[a * TP + p]);
    red_m[part * TP + p] = m;
    __syncthreads();
    m = combine4(red_m, p, [](double x, double y) { return fmax(x, y); });
    double s = 0.0;
    for (int a = part; a < L; a += 4) {
        const double z = Qd[a * TP + p], e = z == -INFINITY ? 0.0 : exp(z - m);
        Qd[a * TP + p] = e;
        s += e;
    }
    red_s[part * TP + p] = s;
    __syncthreads();
    s = combine4(red_s, p, [](double x, double y) { return x + y; });
    const double inv = 1.0 / s;
    for (int a = part; a < L; a += 4) Qd[a * TP + p] *= inv;
    __syncthreads();
}

// Md[wave][k][i], double, of a product: the forward's M[k][wave + 4 i], the backward's M[wave + 4 i][k], 0 beyond L labels --
// what wave `wave` needs at step k as 16 consecutive doubles, so that M comes through wide scalar loads and goes into the
// fma as it is (converted here, once per call, not once per use).
__global__ __launch_bounds__(NT) void k_step_train_mu(const float *__restrict__ M, double *__restrict__ Md, int L, int backward)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= 4 * L * OWN) return;
    const int i = idx % OWN, k = (idx / OWN) % L, o = idx / (OWN * L) + 4 * i;
    Md[idx] = o < L ? (double)(backward ? M[o * L + k] : M[k * L + o]) : 0.0;
}

// acc[i] = sum_k Mw[k][i] * src[k * STRIDE + p] for i < NI, an fma chain in k order; Mw: the wave's [L][OWN] of Md, read
// at wave-uniform addresses.  The forward: k = a, src = Qd.  The backward: k = c, src = F.
template <class T, int STRIDE, int NI>
__device__ __forceinline__ void product_n(const double *__restrict__ Mw, const T *src, int L, int p, double (&acc)[OWN])
{
    double a[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) a[i] = 0.0;
#pragma unroll 2
    for (int k = 0; k < L; k++) {
        const double v = (double)src[k * STRIDE + p];
#pragma unroll
        for (int i = 0; i < NI; i++) a[i] = __builtin_fma(Mw[k * OWN + i], v, a[i]);
    }
#pragma unroll
    for (int i = 0; i < NI; i++) acc[i] = a[i];
}

// gm[i] += sum over the tile's pixels of Q[wave + 4 i][px] * gY[c][px] for i < NI; Qw = Qd + wave * TP, Fc = F + c * FS
template <int NI>
__device__ __forceinline__ void gm_n(const double *Qw, const float *Fc, double (&gm)[OWN])
{
#pragma unroll 2
    for (int px = 0; px < TP; px++) {
        const double f = (double)Fc[px];
#pragma unroll
        for (int i = 0; i < NI; i++) gm[i] = __builtin_fma(Qw[4 * i * TP + px], f, gm[i]);
    }
}

// the run-time label count of the wave, ni = |{i : wave + 4 i < L}| (wave-uniform), as a template argument
#define PHL_TRAIN_NI(ni, call)                                                                                           \
    switch (ni) {                                                                                                        \
    case 1: { constexpr int NI = 1; call; } break;                                                                       \
    case 2: { constexpr int NI = 2; call; } break;                                                                       \
    case 3: { constexpr int NI = 3; call; } break;                                                                       \
    case 4: { constexpr int NI = 4; call; } break;                                                                       \
    case 5: { constexpr int NI = 5; call; } break;                                                                       \
    case 6: { constexpr int NI = 6; call; } break;                                                                       \
    case 7: { constexpr int NI = 7; call; } break;                                                                       \
    case 8: { constexpr int NI = 8; call; } break;                                                                       \
    case 9: { constexpr int NI = 9; call; } break;                                                                       \
    case 10: { constexpr int NI = 10; call; } break;                                                                     \
    case 11: { constexpr int NI = 11; call; } break;                                                                     \
    case 12: { constexpr int NI = 12; call; } break;                                                                     \
    case 13: { constexpr int NI = 13; call; } break;                                                                     \
    case 14: { constexpr int NI = 14; call; } break;                                                                     \
    case 15: { constexpr int NI = 15; call; } break;                                                                     \
    case 16: { constexpr int NI = 16; call; } break;                                                                     \
    }

template <class T, int STRIDE>
__device__ __forceinline__ void product_tile(const double *__restrict__ Mw, const T *src, int L, int ni, int p, double (&acc)[OWN])
{
#pragma unroll
    for (int i = 0; i < OWN; i++) acc[i] = 0.0;
    PHL_TRAIN_NI(ni, (product_n<T, STRIDE, NI>(Mw, src, L, p, acc)))
}

// BACK = false: out = Y of tile blockIdx.x (gY, partial unused).  BACK = true: the tiles blockIdx.x + i gridDim.x of the
// B * tiles; NEED_E: out = dE; NEED_MU: partial[blockIdx.x][L][L] = the workgroup's share of gM.
template <bool VEC, bool BACK, bool NEED_E, bool NEED_MU>
__global__ __launch_bounds__(NT) void k_step_train(const float *__restrict__ E0, const float *__restrict__ G,
                                                   const double *__restrict__ Md, const float *__restrict__ gY,
                                                   float *__restrict__ out, double *__restrict__ partial, int L, int64_t n,
                                                   int tiles, int64_t total)
{
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    double *Qd = lds_d, *red = Qd + L * TP;
    float *F = reinterpret_cast<float *>(red + 2 * NT);
    const int t = threadIdx.x, p = t & (TP - 1);
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ni = wave < L ? (L - wave + 3) >> 2 : 0;           // labels of this wave
    const double *Mw = Md + wave * L * OWN;
    double gm[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) gm[i] = 0.0;

    for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const int b = (int)(blk / tiles), tile = (int)(blk - (int64_t)b * tiles);
        const int64_t p0 = (int64_t)tile * TP, base = (int64_t)b * L * n + p0;
        const int np = (int)(n - p0 < TP ? n - p0 : TP);
        if (BACK) __syncthreads();                               // the tile before this one is out of Qd and F
        load_tile<VEC, BACK>(E0 + base, G ? G + base : nullptr, BACK ? gY + base : nullptr, L, n, np, Qd, F, t);
        __syncthreads();
        softmax_tile(Qd, red, L, p, wave);

        double acc[OWN];
        if (!BACK) {
            product_tile<double, TP>(Mw, Qd, L, ni, p, acc);
#pragma unroll
            for (int i = 0; i < OWN; i++)
                if (wave + 4 * i < L) F[(wave + 4 * i) * FS + p] = (float)acc[i];
        } else {
            if (NEED_MU && p < L) {                              // column c = p of gM, rows wave + 4 i
                PHL_TRAIN_NI(ni, (gm_n<NI>(Qd + wave * TP, F + p * FS, gm)))
            }
            if (NEED_E) {
                product_tile<float, FS>(Mw, F, L, ni, p, acc);                 // t_a
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < OWN; i++)
                    if (wave + 4 * i < L) s = __builtin_fma(Qd[(wave + 4 * i) * TP + p], acc[i], s);
                red[wave * TP + p] = s;
                __syncthreads();                                 // ... and every wave has read its gY
                s = combine4(red, p, [](double x, double y) { return x + y; });
#pragma unroll
                for (int i = 0; i < OWN; i++)
                    if (wave + 4 * i < L) F[(wave + 4 * i) * FS + p] = (float)(Qd[(wave + 4 * i) * TP + p] * (s - acc[i]));
            }
        }
        if (!BACK || NEED_E) {
            __syncthreads();
            store_tile<VEC>(out + base, L, n, np, F, t);
        }
    }
    if (BACK && NEED_MU && p < L) {
        double *o = partial + (int64_t)blockIdx.x * L * L;
#pragma unroll
        for (int i = 0; i < OWN; i++)
            if (wave + 4 * i < L) o[(wave + 4 * i) * L + p] = gm[i];
    }
}

#undef PHL_TRAIN_NI

// gmu[i] = the R partials of element i, added in index order
__global__ __launch_bounds__(NT) void k_step_train_sum(const double *__restrict__ partial, int R, int LL, float *__restrict__ gmu)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= LL) return;
    constexpr int FLY = 16;                                      // loads in flight; the additions stay in index order
    const double *q = partial + i;
    double s = 0.0;
    int w = 0;
    for (; w + FLY <= R; w += FLY) {
        double v[FLY];
#pragma unroll
        for (int j = 0; j < FLY; j++) v[j] = q[(int64_t)(w + j) * LL];
#pragma unroll
        for (int j = 0; j < FLY; j++) s += v[j];
    }
    for (; w < R; w++) s += q[(int64_t)w * LL];
    gmu[i] = (float)s;
}

// tmp gets the prepared M of this call; rc of the launches
template <bool BACK, bool NEED_E, bool NEED_MU>
int launch_train(phl_temps &tmp, const float *E0, const float *G, const float *M, const float *gY, float *out, double *partial,
                 int B, int L, int64_t n, unsigned grid, hipStream_t st)
{
    const int tiles = nchw_tiles(n, TP), md = 4 * L * OWN;
    const size_t lds = train_lds_bytes(L);
    double *Md = tmp.get<double>((size_t)md);
    if (tmp.rc != PHL_OK) return tmp.rc;
    return nchw_dispatch(nchw_vec(n, {E0, G, gY, out}), false, [&](auto vec, auto) -> int {
        constexpr bool VEC = decltype(vec)::value;
        if (const int rc = phl_allow_lds(&k_step_train<VEC, BACK, NEED_E, NEED_MU>, lds)) return rc;
        k_step_train_mu<<<dim3((md + NT - 1) / NT), dim3(NT), 0, st>>>(M, Md, L, BACK ? 1 : 0);
        k_step_train<VEC, BACK, NEED_E, NEED_MU>
            <<<dim3(grid), dim3(NT), lds, st>>>(E0, G, Md, gY, out, partial, L, n, tiles, (int64_t)B * tiles);
        PHL_HIP(hipGetLastError());
        return PHL_OK;
    });
}

bool too_many_labels(const char *who, int L, int &status)
{
    if (L <= MAX_L) return false;
    phl_set_error("%s: %d labels, at most %d", who, L, MAX_L);
    status = PHL_ERR_UNSUPPORTED;
    return true;
}

}  // namespace

extern "C" {

int phl_nchw_step_train_partials(int B, int L, int64_t n)
{
    if (B < 1 || L < 1 || n < 1) return 0;
    const int64_t tiles = (n - 1) / TP + 1;
    if (tiles >= MAX_PARTIALS) return MAX_PARTIALS;
    const int64_t total = tiles * B;
    return (int)(total < MAX_PARTIALS ? total : MAX_PARTIALS);
}

int phl_nchw_step_train(const float *E0, const float *G, const float *mu, float *out, int B, int L, int64_t n, phl_stream stream)
{
    const char *who = "phl_nchw_step_train";
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0, {E0, out, mu},
                   "E0 / out / mu", {E0, G, mu}, out, "out", B, L, n, TP, rc))
        return rc;
    if (too_many_labels(who, L, rc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    phl_temps tmp(st);
    tmp.rc = launch_train<false, false, false>(tmp, E0, G, mu, nullptr, out, nullptr, B, L, n, nchw_grid(B, nchw_tiles(n, TP)).x, st);
    return tmp.release();
}

int phl_nchw_step_train_grad(const float *E0, const float *G, const float *mu, const float *gY, float *dE, float *gmu, int B, int L,
                             int64_t n, phl_stream stream)
{
    const char *who = "phl_nchw_step_train_grad";
    // one result for nchw_check: dE, or gmu where only that is asked for; the other one's aliasing joins its inputs
    const void *result = dE ? (const void *)dE : (const void *)gmu;
    const bool second = dE && gmu && (gmu == dE || (const float *)gmu == E0 || (const float *)gmu == G || (const float *)gmu == mu ||
                                      (const float *)gmu == gY);
    int rc;
    if (nchw_check(who, nchw_text("B=%d L=%d n=%lld", B, L, (long long)n).s, B < 0 || n < 0 || L < 1, B == 0 || n == 0,
                   {E0, mu, gY, result}, "E0 / mu / gY, or both of dE and gmu", {E0, G, mu, gY, second ? result : nullptr}, result,
                   "dE / gmu", B, L, n, TP, rc))
        return rc;
    if (too_many_labels(who, L, rc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int R = gmu ? phl_nchw_step_train_partials(B, L, n) : 0, LL = L * L;
    phl_temps tmp(st);
    double *partial = gmu ? tmp.get<double>((size_t)R * LL) : nullptr;
    if (tmp.rc != PHL_OK) return tmp.release();
    tmp.rc = !gmu ? launch_train<true, true, false>(tmp, E0, G, mu, gY, dE, nullptr, B, L, n, nchw_grid(B, nchw_tiles(n, TP)).x, st)
             : dE ? launch_train<true, true, true>(tmp, E0, G, mu, gY, dE, partial, B, L, n, (unsigned)R, st)
                  : launch_train<true, false, true>(tmp, E0, G, mu, gY, nullptr, partial, B, L, n, (unsigned)R, st);
    if (tmp.rc == PHL_OK && gmu) {
        k_step_train_sum<<<dim3((LL + NT - 1) / NT), dim3(NT), 0, st>>>(partial, R, LL, gmu);
        phl_launched(tmp.rc, who);
    }
    return tmp.release();
}

}  // extern "C"
