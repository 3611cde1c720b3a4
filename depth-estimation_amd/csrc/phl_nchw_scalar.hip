// phl_nchw_scalar.hip -- the unary energies of the upsampler head from a low-resolution disparity, and their backward.
//
// Reference (crf/mb_stereo_crf.py:155-163, CRFdepthUpsampler.forward, and crf_module.py:74-75): a bilinear F.interpolate, its
// maximum read back on the host, a linspace of labels, the Charbonnier energies get_energies_from_scalar, * -10, the
// confidence mask and E0 = -logits * confidence inside CRFasRNN -- eight or nine passes over [B, L, H, W] in front of a
// loop of two kernels per iteration.  Here, with up[b, y, x] the bilinear sample of disp [B, 1, h, w] at output pixel
// (y, x) (torch's align_corners=False form, any ratio), lmax = max(up), labels[a] = lmax * a / (L - 1), g = gamma * lmax:
//
//     E0[b, a, y, x] = up > threshold ?  scale * exp(s) * (sqrt(g^2 + (labels[a] - up)^2) - g)  :  +0.0
//
//   k_scalar_max           launch 1: a thread evaluates up at its pixels (the low-resolution image is tiny and stays in
//                          cache: no [B, 1, H, W] plane is written), the workgroup reduces the maximum and hands it to
//                          the workgroup that arrives last, which reduces the workgroups' maxima and writes labels[L]
//                          (labels[L - 1] = lmax).  The maximum does not depend on the order, so this is the same bits
//                          whichever workgroup comes last.
//   k_scalar_unaries       launch 2, the layout of phl_nchw_common.h: a thread evaluates up and the mask at its four
//                          pixels once and walks the L planes.  Its only global traffic worth the name is one write of
//                          the volume.
//   k_scalar_grad          reads gE0 once in the same layout, recomputes up, the mask and r = sqrt(g^2 + delta^2), and sums
//                            grad_s     = sum gE0 * E0
//                            grad_gamma = sum gE0 * c * scale * exp(s) * lmax * (g / r - 1)        (a term with r == 0: 0)
//                          per workgroup into one float64 pair; k_sum_partials<2> (phl_reduce.h) adds the pairs in index
//                          order: no atomics, the same bits on every call.
//
// gamma and s are read from device memory (the 0-dim parameters of charb): nothing is read back on the host.
//
// Arithmetic.  sqrt(g^2 + delta^2) - g cancels wherever the disparity sits near a label -- where the unary matters -- and
// in fp32 most of the bits go.  Everything between the fp32 loads and the one fp32 store is float64 (-ffp-contract=off: no
// fused multiply-add changes a rounding): the source coordinates, the blend, delta, r, r - g and the product with
// scale * exp(s).  The float64 cancellation that remains is 1e-16 of g.
#include <math.h>

#include "phl_nchw_common.h"
#include "phl_reduce.h"

namespace {

// the bilinear sampling of one image: sizes and the ratios in / out
struct Resize {
    int h, w, H, W;
    double ry, rx;
};

// torch's source index (align_corners=False): src = max(0, (dst + 0.5) * in / out - 0.5), i0 = floor(src),
// i1 = min(i0 + 1, in - 1), lambda = src - i0
__device__ __forceinline__ void source_index(int dst, double ratio, int in, int &i0, int &i1, double &lam)
{
    const double src = fmax(0.0, ((double)dst + 0.5) * ratio - 0.5);
    i0 = min((int)src, in - 1);                                  // (src < in always; the min guards the loads)
    i1 = min(i0 + 1, in - 1);
    lam = src - (double)i0;
}

__device__ __forceinline__ double up_at(const float *__restrict__ img, const Resize &z, int y, int x)
{
    int y0, y1, x0, x1;
    double ly, lx;
    source_index(y, z.ry, z.h, y0, y1, ly);
    source_index(x, z.rx, z.w, x0, x1, lx);
    const float *r0 = img + (int64_t)y0 * z.w, *r1 = img + (int64_t)y1 * z.w;
    const double a = r0[x0], b = r0[x1], c = r1[x0], d = r1[x1];
    return (1.0 - ly) * ((1.0 - lx) * a + lx * b) + ly * ((1.0 - lx) * c + lx * d);
}

// thread_pixels of tile blk, and up[j] = the sample at pixel j (0 outside the image); false: the thread has no pixel
template <bool VEC>
__device__ __forceinline__ bool thread_samples(const float *__restrict__ disp, const Resize &z, int64_t n, int tiles, unsigned blk,
                                               int &b, int64_t &q, bool (&ok)[PX], double (&up)[PX])
{
    if (!thread_pixels<VEC>(n, tiles, blk, b, q, ok)) return false;
    const float *img = disp + (int64_t)b * z.h * z.w;
    int y = n <= INT32_MAX ? (int)((unsigned)q / (unsigned)z.W) : (int)(q / z.W);      // (wave-uniform choice)
    unsigned x = (unsigned)(q - (int64_t)y * z.W);               // x + NT < 2^32
#pragma unroll
    for (int j = 0; j < PX; j++) {
        up[j] = ok[j] ? up_at(img, z, y, (int)x) : 0.0;
        x += VEC ? 1u : (unsigned)NT;
        if (x >= (unsigned)z.W) {
            y += (int)(x / (unsigned)z.W);
            x %= (unsigned)z.W;
        }
    }
    return true;
}

// Launch 1, at most MAX_GRID workgroups that stride over the `total` tiles.  part[gridDim.x]: the workgroups' maxima,
// count: arrivals (zeroed on the stream before the launch).  The maxima cross workgroups inside the launch: thread 0
// stores its workgroup's with a device-scope (write-through) store, waits for it, and adds to the counter with a
// device-scope atomic; the workgroup whose add came last reads the maxima with device-scope loads, behind a barrier its
// thread 0 joins after the add has returned.  The add's release / acquire is paid once per workgroup: with one workgroup
// per tile (1507 at 1110 x 1390) this kernel took 31 us, as long as the 18 planes of launch 2; with the cap, about one
// workgroup per CU, 15 us.  Rounding to fp32 is monotonic: the maximum of the rounded samples is the rounded
// maximum.
constexpr unsigned MAX_GRID = 256;

__global__ __launch_bounds__(NT) void k_scalar_max(const float *__restrict__ disp, Resize z, int64_t n, int tiles, unsigned total,
                                                   int L, float *part, unsigned *count, float *__restrict__ labels)
{
    __shared__ float red[NT / 64];
    __shared__ int last;
    float m = -INFINITY;
    for (unsigned blk = blockIdx.x; blk < total; blk += gridDim.x) {
        int b;
        int64_t q;
        bool ok[PX];
        double up[PX];
        if (thread_samples<false>(disp, z, n, tiles, blk, b, q, ok, up)) {
#pragma unroll
            for (int j = 0; j < PX; j++)
                if (ok[j]) m = fmaxf(m, (float)up[j]);
        }
    }
    m = block_max_f(m, red);
    if (threadIdx.x == 0) {
        __hip_atomic_store(part + blockIdx.x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned seen = __hip_atomic_fetch_add(count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = seen == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    m = -INFINITY;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += NT)
        m = fmaxf(m, __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const double lmax = block_max_f(m, red);                     // (the barrier above lies behind every read of red)
    for (int a = threadIdx.x; a < L; a += NT) labels[a] = a == L - 1 ? (float)lmax : (float)(lmax * (double)a / (double)(L - 1));
}

// what both per-element kernels need of the parameters: g = gamma * lmax and k = scale * exp(s)
struct Params {
    double lmax, g, k;
};
__device__ __forceinline__ Params params(const float *__restrict__ labels, const float *__restrict__ gamma,
                                         const float *__restrict__ s, int L, double scale)
{
    Params p;
    p.lmax = labels[L - 1];
    p.g = (double)*gamma * p.lmax;
    p.k = scale * exp((double)*s);
    return p;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void k_scalar_unaries(const float *__restrict__ disp, const float *__restrict__ labels,
                                                       const float *__restrict__ gamma, const float *__restrict__ s,
                                                       float *__restrict__ E0, Resize z, int64_t n, int tiles, int L, double scale,
                                                       float threshold)
{
    int b;
    int64_t q;
    bool ok[PX], c[PX];
    double up[PX];
    if (!thread_samples<VEC>(disp, z, n, tiles, blockIdx.x, b, q, ok, up)) return;
    const Params p = params(labels, gamma, s, L, scale);
    const double g2 = p.g * p.g;
#pragma unroll
    for (int j = 0; j < PX; j++) c[j] = (float)up[j] > threshold;
    float *o = E0 + (int64_t)b * L * n + q;
    for (int a = 0; a < L; a++, o += n) {
        const double lab = labels[a];                            // wave-uniform
        float e[PX];
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const double d = lab - up[j];
            e[j] = c[j] ? (float)(p.k * (sqrt(g2 + d * d) - p.g)) : 0.f;
        }
        store_px<VEC>(o, ok, e);
    }
}

// partial[2 blk] = the workgroup's share of grad_gamma, partial[2 blk + 1] of grad_s
template <bool VEC>
__global__ __launch_bounds__(NT) void k_scalar_grad(const float *__restrict__ disp, const float *__restrict__ labels,
                                                    const float *__restrict__ gamma, const float *__restrict__ s,
                                                    const float *__restrict__ gE0, double *__restrict__ partial, Resize z, int64_t n,
                                                    int tiles, int L, double scale, float threshold)
{
    __shared__ double red[2][NT / 64];
    int b;
    int64_t q;
    bool ok[PX], c[PX];
    double up[PX];
    double acc_g = 0.0, acc_s = 0.0;                              // sum ge (g / r - 1) and sum ge (r - g) over the masked pixels
    if (thread_samples<VEC>(disp, z, n, tiles, blockIdx.x, b, q, ok, up)) {
        const Params p = params(labels, gamma, s, L, scale);
        const double g2 = p.g * p.g;
#pragma unroll
        for (int j = 0; j < PX; j++) c[j] = ok[j] && (float)up[j] > threshold;
        const float *gp = gE0 + (int64_t)b * L * n + q;
        for (int a = 0; a < L; a++, gp += n) {
            const double lab = labels[a];
            float ge[PX];
            load_px<VEC>(gp, ok, ge);
#pragma unroll
            for (int j = 0; j < PX; j++) {
                const double d = lab - up[j], r = sqrt(g2 + d * d);
                const double w = c[j] ? (double)ge[j] : 0.0;
                acc_s += w * (r - p.g);
                acc_g += r > 0.0 ? w * (p.g / r - 1.0) : 0.0;
            }
        }
        acc_s *= p.k;
        acc_g *= p.k * p.lmax;
    }
    acc_g = wave_sum_d(acc_g);
    acc_s = wave_sum_d(acc_s);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = acc_g;
        red[1][threadIdx.x >> 6] = acc_s;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *r = red[threadIdx.x];
        partial[2 * (int64_t)blockIdx.x + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// The argument checks both entry points share, in the order include/phl.h states (the forward's second output, labels,
// is checked against its inputs by the forward itself); true: nothing to launch
bool check_args(const char *who, const float *disp, const float *labels, const float *gamma, const float *s, const float *gE0,
                bool grad, const float *result, int B, int h, int w, int H, int W, int L, int &status)
{
    const nchw_text sizes("B=%d L=%d H=%d W=%d from h=%d w=%d", B, L, H, W, h, w);
    if (nchw_check(who, sizes.s, L < 2 || h < 1 || w < 1 || H < 1 || W < 1 || B < 0, B == 0,
                   {disp, labels, gamma, s, result, grad ? gE0 : result},
                   grad ? "disp / labels / gamma / s / gE0 / grad" : "disp / gamma / s / E0 / labels", {disp, gamma, s, labels, gE0},
                   result, grad ? "grad" : "E0", B, L, (int64_t)H * W, WGP, status))
        return true;
    if (nchw_too_large(B, 1, (int64_t)h * w, 0)) {              // the disparity alone (h, w <= 2^31 - 1: no overflow)
        phl_set_error("%s: too many elements (%s)", who, sizes.s);
        status = PHL_ERR_TOO_LARGE;
        return true;
    }
    return false;
}

inline Resize resize(int h, int w, int H, int W)
{
    return Resize{h, w, H, W, (double)h / (double)H, (double)w / (double)W};
}

}  // namespace

extern "C" {

int phl_nchw_scalar_unaries(const float *disp, const float *gamma, const float *s, float *E0, float *labels, int B, int h, int w,
                            int H, int W, int L, double scale, double threshold, phl_stream stream)
{
    const char *who = "phl_nchw_scalar_unaries";
    int rc;
    if (check_args(who, disp, labels, gamma, s, nullptr, false, E0, B, h, w, H, W, L, rc)) return rc;
    if (labels == disp || labels == gamma || labels == s) {
        phl_set_error("%s: labels aliases an input", who);
        return PHL_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const int tiles = nchw_tiles(n);
    const unsigned blocks = nchw_grid(B, tiles).x;
    const Resize z = resize(h, w, H, W);
    // scratch: 16 bytes that hold the arrival counter (the block the memset zeroes), then one maximum per workgroup
    const unsigned grid1 = blocks < MAX_GRID ? blocks : MAX_GRID;
    phl_temps tmp(st);
    unsigned *words = tmp.get<unsigned>(4 + (size_t)grid1);
    if (tmp.rc != PHL_OK) return tmp.release();
    PHL_HIP(hipMemsetAsync(words, 0, 16, st));
    k_scalar_max<<<dim3(grid1), dim3(NT), 0, st>>>(disp, z, n, tiles, blocks, L, reinterpret_cast<float *>(words + 4), words, labels);
    nchw_dispatch(nchw_vec(n, {E0}), false, [&](auto vec, auto) {
        k_scalar_unaries<decltype(vec)::value>
            <<<dim3(blocks), dim3(NT), 0, st>>>(disp, labels, gamma, s, E0, z, n, tiles, L, scale, (float)threshold);
    });
    phl_launched(tmp.rc, who);
    return tmp.release();
}

int phl_nchw_scalar_unaries_grad(const float *disp, const float *labels, const float *gamma, const float *s, const float *gE0,
                                 float *grad, int B, int h, int w, int H, int W, int L, double scale, double threshold,
                                 phl_stream stream)
{
    const char *who = "phl_nchw_scalar_unaries_grad";
    int rc;
    if (check_args(who, disp, labels, gamma, s, gE0, true, grad, B, h, w, H, W, L, rc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const int tiles = nchw_tiles(n);
    const unsigned blocks = nchw_grid(B, tiles).x;
    const Resize z = resize(h, w, H, W);
    phl_temps tmp(st);
    double *partial = tmp.get<double>(2 * (size_t)blocks);
    if (tmp.rc != PHL_OK) return tmp.release();
    nchw_dispatch(nchw_vec(n, {gE0}), false, [&](auto vec, auto) {
        k_scalar_grad<decltype(vec)::value>
            <<<dim3(blocks), dim3(NT), 0, st>>>(disp, labels, gamma, s, gE0, partial, z, n, tiles, L, scale, (float)threshold);
    });
    k_sum_partials<2><<<dim3(1), dim3(256), 0, st>>>(partial, (int64_t)blocks, 1.0, grad);      // grad[0] = grad_gamma, grad[1] = grad_s
    phl_launched(tmp.rc, who);
    return tmp.release();
}

}  // extern "C"
