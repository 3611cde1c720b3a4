// phl_tiles.hip -- pixel chunks ("tiles") and the LDS-staged splat / slice kernels.
//
// Why: in the plain gather kernels (phl_filter.hip) every pixel row is re-read by its d+1
// vertices (splat) and every vertex row by all pixels of its cell (slice).  Those re-reads
// come out of L2 / the Infinity Cache at fabric rate and bound the kernels (round-1 profile:
// splat moved 19 GB for 3.2 GB of input).  A chunk is a set of <= P pixels that are close in
// feature space, so they share most of their lattice vertices; a workgroup stages the chunk's
// rows ONCE in LDS (channel slab by channel slab) and all reuse happens there:
//
//   k_splat_tiled   stage Q[chunk pixels][slab] -> every local vertex sums its pixel-sorted
//                   segment out of LDS -> the vertex row if this chunk is the vertex's only
//                   contributor, else a partial row; k_splat_reduce then adds a vertex's
//                   partial rows in ascending chunk order (deterministic, no float atomics)
//   k_slice_tiled   stage vert[chunk's local vertices][slab] -> every pixel gathers its d+1
//                   rows from LDS with the reference's per-term arithmetic (bit-exact)
//
// The chunks and everything these kernels read of them are made once per lattice, in phl_tiles_build.hip.
//
// Reference semantics are those of crf/lattice/lite/permutohedral.h:454-455 (splat
// accumulate) and :473-483 (slice); summation ORDER of multi-chunk vertices differs from the
// reference's pixel order (partial sums), hence results agree to fp32 rounding (~1e-7), not
// bit for bit; PHL_FILTER_EXACT selects the pixel-ordered gather splat instead.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "phl_internal.h"

namespace {

// ---- hot kernels -----------------------------------------------------------------------------
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float div_c(float t, float c, float rc)
{
    float q = t * rc;
    float rem = __builtin_fmaf(-q, c, t);
    return __builtin_fmaf(rem, rc, q);
}
__device__ __forceinline__ float4 term4(float4 acc, float w, float4 v, float c, float rc)   // acc + (w*v)/c  (:480)
{
    return make_float4(acc.x + div_c(w * v.x, c, rc), acc.y + div_c(w * v.y, c, rc), acc.z + div_c(w * v.z, c, rc),
                       acc.w + div_c(w * v.w, c, rc));
}
__device__ __forceinline__ float4 fma4(float4 acc, float w, float4 v)
{
    return make_float4(__builtin_fmaf(w, v.x, acc.x), __builtin_fmaf(w, v.y, acc.y), __builtin_fmaf(w, v.z, acc.z),
                       __builtin_fmaf(w, v.w, acc.w));
}

// lane K of every 16-lane DPP row, to all lanes of that row (v_mov_b32_dpp row_newbcast:K -- VALU, no LDS traffic)
#define PHL_ROW_BCAST(x, K) ((unsigned)__builtin_amdgcn_update_dpp(0, (int)(x), 0x150 + (K), 0xF, 0xF, false))

// Eight consecutive entries of a segment, held one per lane in lanes K0..K0+7 of each DPP row (e.x = byte offset
// of the pixel's LDS row, e.y = weight bits): broadcast each, issue the eight 16-byte row reads back to
// back (one LDS round trip for all of them), then accumulate in entry order.
template <int K0>
__device__ __forceinline__ float4 sum8(float4 acc, const uint2 e, const char *rbase)
{
    float4 q[8];
    unsigned w[8];
#define PHL_E(k) w[k] = PHL_ROW_BCAST(e.y, K0 + k); q[k] = *reinterpret_cast<const float4 *>(rbase + PHL_ROW_BCAST(e.x, K0 + k));
    PHL_E(0) PHL_E(1) PHL_E(2) PHL_E(3) PHL_E(4) PHL_E(5) PHL_E(6) PHL_E(7)
#undef PHL_E
#pragma unroll
    for (int k = 0; k < 8; k++) acc = fma4(acc, __uint_as_float(w[k]), q[k]);
    return acc;
}

// One workgroup (TPB threads) per chunk.  LPRS lanes own one row of a channel slab of
// SL = 4*LPRS floats.  LDS: [rows x SL] staged rows | per-entry {LDS byte offset, weight} |
// chunk pixel ids | local segment pointers | destination of each local vertex.  Index data
// is staged ONCE per chunk; inside the slab loop global memory is touched only for value rows,
// and the rows of slab s+1 are prefetched into registers while slab s is being summed.
// Each of a wavefront's 64/LPRS lane groups owns one local vertex and sums its pixel-sorted
// segment sequentially out of LDS: a segmented reduction with one segment per lane group,
// deterministic, no atomics (details at the loop).
// splat: segments of at least this many entries are summed by a whole wavefront (see k_splat_tiled).  Two workgroups
// share a CU, so imbalance inside one is mostly absorbed by the other and what counts is total work: the
// cooperative form pads a segment to a multiple of 64 entries and pays a cross-row combine, so it is reserved for
// segments that would otherwise be the whole critical path (flat image regions: all 256 pixels in one vertex).
inline int long_seg()
{
    static const int v = getenv("PHL_LONG_SEG") ? atoi(getenv("PHL_LONG_SEG")) : 128;
    return v < 16 ? 16 : v;
}
constexpr int TPB = 512;     // slice workgroup
constexpr int TPB_S = 512;   // splat workgroup (1024 threads and 1 workgroup per CU measured no better)

template <int LPRS>
__global__ __launch_bounds__(TPB_S) void k_splat_tiled(const float *__restrict__ src, int64_t src_rs, int vd, int n, int P,
                                                     int dp1, int nv_cap, const int *__restrict__ pix_order,
                                                     const int *__restrict__ vptr, const int *__restrict__ slot_vert,
                                                     const int *__restrict__ slot_pidx, const int2 *__restrict__ seg_rng,
                                                     const phl_contrib_t *__restrict__ seg, float *__restrict__ vert,
                                                     float *__restrict__ partial, int nchunks, int xcd_chunk,
                                                     unsigned long long *__restrict__ tl, const int *__restrict__ chunk_list,
                                                     int nv_lo, int nv_hi, int long_seg, int nsets,
                                                     const float *__restrict__ fref, int64_t fref_rs, int64_t fref_cs,
                                                     int64_t out_rs)
{
    // nsets > 1 (the wide splat of the gradient w.r.t. the features, phl_filter_grad): every staged slab is summed
    // nsets times, set 0 with the barycentric weights w and set 1+k with w * fref[pixel][k] -- the splat of
    // src (x) ref[:, k] without ever forming that product in memory -- into channel block `set` of rows that are
    // out_rs = nsets * vd floats long.  nsets == 1: the plain splat (fref unused, out_rs = vd).
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SL = LPRS * 4;
    constexpr int G = TPB_S / LPRS;          // row groups of the workgroup (staging)
    constexpr int Q = 64 / LPRS;           // lane groups of a wavefront (entry-parallel)
    constexpr int NW = TPB_S / 64;
    constexpr int PF = (256 / G) < 8 ? (256 / G) : 8;   // rows prefetched per thread
    const int g = threadIdx.x / LPRS, l = threadIdx.x % LPRS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = lane / LPRS;
    // XCD-aware chunk order (see k_blur): neighbouring chunks share boundary vertices.  With a chunk list
    // (phl_splat_part: a subset of the chunks, `nchunks` = its length) the same order runs over list positions.
    const int ci = xcd_chunk > 0 ? (int)(blockIdx.x & 7) * xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (ci >= nchunks) return;
    const int c = chunk_list ? chunk_list[ci] : ci;
    // debug timeline (PHL_TIMELINE=file): 100 MHz wall-clock stamps per workgroup, tl == nullptr in normal runs
    unsigned long long *tlb = tl ? tl + (size_t)blockIdx.x * 8 : nullptr;
    if (tlb && threadIdx.x == 0) {
        tlb[0] = wall_clock64();
        tlb[7] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | __builtin_amdgcn_s_getreg((31 << 11) | 4);
    }
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int64_t ebase = (int64_t)base * dp1;
    const int vbase = vptr[c], nv = vptr[c + 1] - vbase;
    // chunk classes (phl_launch_splat_tiled): this launch's LDS is sized for chunks with nv_lo < nv <= nv_hi local
    // vertices; the others belong to the launch of another class
    if (nv <= nv_lo || nv > nv_hi) return;
    float *rows = lds;                                             // [P][SL] staged pixel rows + one row of zeros
    uint2 *ent = reinterpret_cast<uint2 *>(lds + (size_t)(P + 1) * SL);
    int2 *meta = reinterpret_cast<int2 *>(ent + P * dp1);          // [nv_cap] {seg begin | seg end << 16, destination row}
    int *pixl = reinterpret_cast<int *>(meta + nv_cap);           // [P]
    int *ctr = pixl + P;                                           // two work counters, used by alternate slabs; [2] = #long segments
    // Loads are issued UNCONDITIONALLY from clamped (always valid) addresses and only the LDS
    // stores are predicated: a load under a divergent `if` makes hipcc wait vmcnt(0) per load.
    const int kclamp = cnt - 1;
    const char *rbase = reinterpret_cast<const char *>(rows) + l * 16;
    float4 pf[PF];
    // Prologue, arranged so that the chunk pays ONE dependent HBM round trip, not two: every
    // thread fetches the pixel ids of its own first PF rows itself and launches slab 0's row loads
    // on them, while the index data (entries, pixel ids, per-vertex records) streams into LDS.
    int prow[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) prow[u] = pix_order[base + min(g + u * G, kclamp)];
    for (int e = threadIdx.x; e < E; e += TPB_S) {
        const phl_contrib_t s = seg[ebase + e];
        ent[e] = make_uint2((unsigned)(s.pixel * SL * 4), __float_as_uint(s.w));
    }
    for (int k = threadIdx.x; k < cnt; k += TPB_S) pixl[k] = pix_order[base + k];
    for (int i = threadIdx.x; i < nv; i += TPB_S) {
        const int2 rg = seg_rng[vbase + i];
        // destination: the vertex row (bit 31 set) if this chunk is the vertex's only contributor, else a partial row
        const int sv = slot_vert[vbase + i];
        meta[i] = make_int2((int)(rg.x - ebase) | ((int)(rg.y - ebase) << 16), sv < 0 ? sv : slot_pidx[vbase + i]);
        // Local vertices come in descending segment length (k_chunk_group), so the LONG ones (>= long_seg entries:
        // summed by a whole wavefront, below) are a prefix; its length is written by exactly one thread.
        const bool lng = rg.y - rg.x >= long_seg;
        if (i + 1 < nv) {
            const int2 rn = seg_rng[vbase + i + 1];
            if (lng && rn.y - rn.x < long_seg) ctr[2] = i + 1;
        } else if (lng) {
            ctr[2] = nv;
        }
        if (i == 0 && !lng) ctr[2] = 0;
    }
    if (nv == 0 && threadIdx.x == 0) ctr[2] = 0;
    if (threadIdx.x < 2) ctr[threadIdx.x] = NW;
    if (threadIdx.x < LPRS) st4(rows + (size_t)P * SL + threadIdx.x * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    {
        const bool chok = l * 4 < vd;
        const int chc = chok ? l * 4 : 0;
#pragma unroll
        for (int u = 0; u < PF; u++) pf[u] = ld4(src + (int64_t)prow[u] * src_rs + chc);
#pragma unroll
        for (int u = 0; u < PF; u++)
            if (chok && g + u * G < cnt) st4(rows + (g + u * G) * SL + l * 4, pf[u]);
        if (PF * G < 256) {                // wide slabs: more rows per thread than the prefetch depth
            __syncthreads();               // pixl is needed for the remaining rows
            for (int k0 = g + PF * G; k0 < cnt; k0 += PF * G) {
#pragma unroll
                for (int u = 0; u < PF; u++) pf[u] = ld4(src + (int64_t)pixl[min(k0 + u * G, kclamp)] * src_rs + chc);
#pragma unroll
                for (int u = 0; u < PF; u++)
                    if (chok && k0 + u * G < cnt) st4(rows + (k0 + u * G) * SL + l * 4, pf[u]);
            }
        }
    }
    for (int c0 = 0; c0 < vd; c0 += SL) {
        const int ch = c0 + l * 4;
        const bool chok = ch < vd;
        __syncthreads();                   // rows of this slab are in LDS
        const int slab = c0 / SL;
        if (tlb && threadIdx.x == 0 && slab < 2) tlb[1 + 2 * slab] = wall_clock64();
        const int chn = ch + SL;
        const bool more = c0 + SL < vd;    // wave-uniform
        const bool chnok = more && chn < vd;
        const int chnc = chnok ? chn : 0;
        if (more) {
#pragma unroll
            for (int u = 0; u < PF; u++) pf[u] = ld4(src + (int64_t)pixl[min(g + u * G, kclamp)] * src_rs + chnc);
        }
        // Each of the wavefront's Q lane groups sums ONE local vertex (its pixel-sorted segment,
        // sequentially, out of LDS).  Local vertices are numbered by descending segment length
        // (k_chunk_group), so the Q vertices of a group have nearly equal loops, and the waves take
        // groups longest-first from a shared counter: no cross-lane combine, no padding, and the
        // per-vertex bookkeeping is paid once per Q vertices.
        for (int set = 0; set < nsets; set++) {
        const int phase = slab * nsets + set;
        if (nsets > 1) {
            if (set > 0) __syncthreads();                 // the previous set's sums are done with the entry weights
            for (int e = threadIdx.x; e < E; e += TPB_S) {
                const phl_contrib_t sg = seg[ebase + e];
                const float f = set ? fref[(int64_t)pixl[sg.pixel] * fref_rs + (int64_t)(set - 1) * fref_cs] : 1.f;
                ent[e].y = __float_as_uint(sg.w * f);
            }
        }
        if (threadIdx.x == 0) ctr[(phase + 1) & 1] = NW;  // re-arm the other counter for the next phase
        if (nsets > 1) __syncthreads();                   // weights of this set are in LDS
        int *slab_ctr = ctr + (phase & 1);
        // Work items, handed out longest-first: items [0, nlong) are single LONG vertices (LPRS >= 16 only), summed
        // by all Q lane groups of the wave together -- group q takes the 16-entry batches q, q+Q, ... of the
        // segment and the Q partial sums are combined across the DPP rows in a fixed order -- so that one 256-entry
        // segment (a flat image region: every pixel of the chunk in one vertex) costs a wave 4 batches, not 16;
        // the remaining items are groups of Q vertices, one per lane group.
        const int nlong = (LPRS >= 16 && Q > 1) ? ctr[2] : 0;
        const int nitems = nlong + (nv - nlong + Q - 1) / Q;
        for (int gi = wave; gi < nitems;) {
            const bool coop = gi < nlong;                       // wave-uniform
            const int i = coop ? gi : nlong + (gi - nlong) * Q + q;
            int2 m = make_int2(0, 0);
            if (i < nv) m = meta[i];
            int nxt = 0;
            if (lane == 0) nxt = atomicAdd(slab_ctr, 1);       // next item, fetched under this one's work
            const int s1 = (int)((unsigned)m.x >> 16);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int s = m.x & 0xFFFF;
            if constexpr (LPRS >= 16) {
                // A lane group is one or more whole 16-lane DPP rows.  Each row keeps SIXTEEN entries of its
                // vertex's segment in registers, one per lane (a single 8-byte LDS read per lane), and hands
                // them round with row broadcasts; the row reads of eight entries are in flight together.
                // The trip count is the longest of the wave's segments, so the loop is wave-uniform; a
                // shorter segment pads with weight 0 on the row of zeros.
                const int len = s1 - s;
                int lmax = __builtin_amdgcn_readlane(len, 0);
                if (Q > 1) lmax = max(lmax, __builtin_amdgcn_readlane(len, 32));
                if (Q > 2) lmax = max(max(lmax, __builtin_amdgcn_readlane(len, 16)), __builtin_amdgcn_readlane(len, 48));
                const int r16 = lane & 15;
                const unsigned zoff = (unsigned)P * SL * 4;
                const int elast = E - 1;
                // cooperative item: group q starts at batch q and strides over Q batches
                const int step = coop ? 16 * Q : 16;
                if (coop) s += 16 * q;
                uint2 e = ent[min(max(s + r16, 0), elast)];
                if (s + r16 >= s1) e = make_uint2(zoff, 0u);
                for (int b = 0; b < lmax; b += step) {
                    const int nx = s + b + step + r16;
                    uint2 en = ent[min(nx, elast)];              // next sixteen, under this batch's work
                    if (nx >= s1) en = make_uint2(zoff, 0u);
                    acc = sum8<0>(acc, e, rbase);
                    if (b + 8 < lmax) acc = sum8<8>(acc, e, rbase);
                    e = en;
                }
                if (Q > 1 && coop) {
                    // ((g0 + g1) + (g2 + g3)): every lane adds its partner's value, so all groups end with the same bits
                    acc = make_float4(acc.x + __shfl_xor(acc.x, LPRS), acc.y + __shfl_xor(acc.y, LPRS),
                                      acc.z + __shfl_xor(acc.z, LPRS), acc.w + __shfl_xor(acc.w, LPRS));
                    if (Q > 2)
                        acc = make_float4(acc.x + __shfl_xor(acc.x, 2 * LPRS), acc.y + __shfl_xor(acc.y, 2 * LPRS),
                                          acc.z + __shfl_xor(acc.z, 2 * LPRS), acc.w + __shfl_xor(acc.w, 2 * LPRS));
                }
            } else {
            // software pipeline: the index reads of batch b+1 are issued before the row reads of
            // batch b are consumed, so a batch costs one LDS round trip instead of two (LDS returns
            // in order: waiting for the rows leaves the next indices in flight)
            if (s + 4 <= s1) {
                uint2 e0 = ent[s], e1 = ent[s + 1], e2 = ent[s + 2], e3 = ent[s + 3];
                for (; s + 8 <= s1; s += 4) {
                    const float4 q0 = *reinterpret_cast<const float4 *>(rbase + e0.x);
                    const float4 q1 = *reinterpret_cast<const float4 *>(rbase + e1.x);
                    const float4 q2 = *reinterpret_cast<const float4 *>(rbase + e2.x);
                    const float4 q3 = *reinterpret_cast<const float4 *>(rbase + e3.x);
                    const uint2 n0 = ent[s + 4], n1 = ent[s + 5], n2 = ent[s + 6], n3 = ent[s + 7];
                    acc = fma4(acc, __uint_as_float(e0.y), q0);
                    acc = fma4(acc, __uint_as_float(e1.y), q1);
                    acc = fma4(acc, __uint_as_float(e2.y), q2);
                    acc = fma4(acc, __uint_as_float(e3.y), q3);
                    e0 = n0; e1 = n1; e2 = n2; e3 = n3;
                }
                const float4 q0 = *reinterpret_cast<const float4 *>(rbase + e0.x);
                const float4 q1 = *reinterpret_cast<const float4 *>(rbase + e1.x);
                const float4 q2 = *reinterpret_cast<const float4 *>(rbase + e2.x);
                const float4 q3 = *reinterpret_cast<const float4 *>(rbase + e3.x);
                acc = fma4(acc, __uint_as_float(e0.y), q0);
                acc = fma4(acc, __uint_as_float(e1.y), q1);
                acc = fma4(acc, __uint_as_float(e2.y), q2);
                acc = fma4(acc, __uint_as_float(e3.y), q3);
                s += 4;
            }
            for (; s < s1; s++) {
                const uint2 e0 = ent[s];
                acc = fma4(acc, __uint_as_float(e0.y), *reinterpret_cast<const float4 *>(rbase + e0.x));
            }
            }
            if (i < nv && chok && !(coop && q != 0)) {
                float *dst = m.y < 0 ? vert + (int64_t)(m.y & 0x7FFFFFFF) * out_rs : partial + (int64_t)m.y * out_rs;
                st4(dst + (int64_t)set * vd + ch, acc);
            }
            gi = __builtin_amdgcn_readfirstlane(nxt);
        }
        }   // sets
        __syncthreads();                   // everyone is done reading this slab
        if (tlb && threadIdx.x == 0 && slab < 2) tlb[2 + 2 * slab] = wall_clock64();
        if (tlb && threadIdx.x == 0 && !more) tlb[5] = wall_clock64();
        if (more) {
#pragma unroll
            for (int u = 0; u < PF; u++)
                if (chnok && g + u * G < cnt) st4(rows + (g + u * G) * SL + l * 4, pf[u]);
            for (int k0 = g + PF * G; k0 < cnt; k0 += PF * G) {   // rows beyond the prefetch depth (wide slabs)
#pragma unroll
                for (int u = 0; u < PF; u++) pf[u] = ld4(src + (int64_t)pixl[min(k0 + u * G, kclamp)] * src_rs + chnc);
#pragma unroll
                for (int u = 0; u < PF; u++)
                    if (chnok && k0 + u * G < cnt) st4(rows + (k0 + u * G) * SL + l * 4, pf[u]);
            }
        }
    }
}

// ---- wide splat, one sum phase per slab -------------------------------------------------------------------------------
// phl_filter_grad's first stage: vertex rows [set][vd], set 0 = splat of src, set 1+k = splat of src (x) fref[:, k]
// (NS = d+1 sets).  k_splat_tiled's nsets > 1 mode runs its sum phase NS times per slab, re-staging the entry weights in
// between: NS times the LDS row reads, which is what bounds it (1.56 ms at C2 against 0.42 for a plain splat).  Here
// every LDS row read feeds NS accumulators: a lane keeps its entry's barycentric weight AND its pixel's d features
// (gathered from the L2-resident feature rows one batch ahead), and per entry the weights w, w*f_0 ... w*f_{d-1} are
// formed from row broadcasts.  Same products, same summation order, same combine as the nsets > 1 mode: bitwise the
// same rows.  64-channel slabs (16 lanes per row) only; other widths keep the multi-phase mode.
// one entry (lane K of every DPP row) into all NS accumulators; K must be a literal for the DPP control field
template <int K, int NS>
__device__ __forceinline__ void wide_entry(float4 (&acc)[NS], const float4 q, const float w, const float (&f)[NS > 1 ? NS - 1 : 1])
{
    acc[0] = fma4(acc[0], w, q);
#define PHL_WJ(j)                                                                                            \
    if constexpr (j + 1 < NS) {                                                                              \
        const float wj = w * __uint_as_float(PHL_ROW_BCAST(__float_as_uint(f[j < NS - 1 ? j : 0]), K));      \
        acc[j + 1 < NS ? j + 1 : 0] = fma4(acc[j + 1 < NS ? j + 1 : 0], wj, q);                              \
    }
    PHL_WJ(0) PHL_WJ(1) PHL_WJ(2) PHL_WJ(3) PHL_WJ(4) PHL_WJ(5) PHL_WJ(6)
#undef PHL_WJ
}

// four consecutive entries K0..K0+3: the four row reads in flight together, then the NS x 4 accumulations
template <int K0, int NS>
__device__ __forceinline__ void sum4w(float4 (&acc)[NS], const uint2 e, const float (&f)[NS > 1 ? NS - 1 : 1], const char *rbase)
{
    const float w0 = __uint_as_float(PHL_ROW_BCAST(e.y, K0 + 0)), w1 = __uint_as_float(PHL_ROW_BCAST(e.y, K0 + 1));
    const float w2 = __uint_as_float(PHL_ROW_BCAST(e.y, K0 + 2)), w3 = __uint_as_float(PHL_ROW_BCAST(e.y, K0 + 3));
    const float4 q0 = *reinterpret_cast<const float4 *>(rbase + PHL_ROW_BCAST(e.x, K0 + 0));
    const float4 q1 = *reinterpret_cast<const float4 *>(rbase + PHL_ROW_BCAST(e.x, K0 + 1));
    const float4 q2 = *reinterpret_cast<const float4 *>(rbase + PHL_ROW_BCAST(e.x, K0 + 2));
    const float4 q3 = *reinterpret_cast<const float4 *>(rbase + PHL_ROW_BCAST(e.x, K0 + 3));
    wide_entry<K0 + 0, NS>(acc, q0, w0, f);
    wide_entry<K0 + 1, NS>(acc, q1, w1, f);
    wide_entry<K0 + 2, NS>(acc, q2, w2, f);
    wide_entry<K0 + 3, NS>(acc, q3, w3, f);
}

// DP1 = 0 (phl_filter_grad's feature groups): the NS sets are block 0 and NS - 1 of the d features (fref points at the
// group's first column) while an entry list still has dp1_rt = d + 1 entries per pixel; DP1 = NS: all d features.
template <int NS, int DP1 = NS>
__global__ __launch_bounds__(TPB_S) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_splat_wide(const float *__restrict__ src, int64_t src_rs, int vd, int n, int P,
                                                    int nv_cap, const int *__restrict__ pix_order, const int *__restrict__ vptr,
                                                    const int *__restrict__ slot_vert, const int *__restrict__ slot_pidx,
                                                    const int2 *__restrict__ seg_rng, const phl_contrib_t *__restrict__ seg,
                                                    float *__restrict__ vert, float *__restrict__ partial, int nchunks, int xcd_chunk,
                                                    const int *__restrict__ chunk_list, int nv_lo, int nv_hi, int long_seg,
                                                    const float *__restrict__ fref, int64_t fref_rs, int64_t fref_cs, int dp1_rt)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LPRS = 16, SL = 64, G = TPB_S / LPRS, Q = 4, NW = TPB_S / 64, PF = 8, NF = NS - 1;
    const int dp1 = DP1 ? DP1 : dp1_rt;
    const int g = threadIdx.x / LPRS, l = threadIdx.x % LPRS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = lane / LPRS;
    const int ci = xcd_chunk > 0 ? (int)(blockIdx.x & 7) * xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (ci >= nchunks) return;
    const int c = chunk_list ? chunk_list[ci] : ci;
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int64_t ebase = (int64_t)base * dp1;
    const int vbase = vptr[c], nv = vptr[c + 1] - vbase;
    if (nv <= nv_lo || nv > nv_hi) return;
    const int64_t out_rs = (int64_t)NS * vd;
    // LDS layout and prologue as in k_splat_tiled<16>
    float *rows = lds;
    uint2 *ent = reinterpret_cast<uint2 *>(lds + (size_t)(P + 1) * SL);
    int2 *meta = reinterpret_cast<int2 *>(ent + P * dp1);
    int *pixl = reinterpret_cast<int *>(meta + nv_cap);
    int *ctr = pixl + P;
    const int kclamp = cnt - 1;
    const char *rbase = reinterpret_cast<const char *>(rows) + l * 16;
    float4 pf[PF];
    int prow[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) prow[u] = pix_order[base + min(g + u * G, kclamp)];
    for (int e = threadIdx.x; e < E; e += TPB_S) {
        const phl_contrib_t sg = seg[ebase + e];
        ent[e] = make_uint2((unsigned)(sg.pixel * SL * 4), __float_as_uint(sg.w));
    }
    for (int k = threadIdx.x; k < cnt; k += TPB_S) pixl[k] = pix_order[base + k];
    for (int i = threadIdx.x; i < nv; i += TPB_S) {
        const int2 rg = seg_rng[vbase + i];
        const int sv = slot_vert[vbase + i];
        meta[i] = make_int2((int)(rg.x - ebase) | ((int)(rg.y - ebase) << 16), sv < 0 ? sv : slot_pidx[vbase + i]);
        const bool lng = rg.y - rg.x >= long_seg;
        if (i + 1 < nv) {
            const int2 rn = seg_rng[vbase + i + 1];
            if (lng && rn.y - rn.x < long_seg) ctr[2] = i + 1;
        } else if (lng) {
            ctr[2] = nv;
        }
        if (i == 0 && !lng) ctr[2] = 0;
    }
    if (nv == 0 && threadIdx.x == 0) ctr[2] = 0;
    if (threadIdx.x < 2) ctr[threadIdx.x] = NW;
    if (threadIdx.x < LPRS) st4(rows + (size_t)P * SL + threadIdx.x * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    {
        const bool chok = l * 4 < vd;
        const int chc = chok ? l * 4 : 0;
#pragma unroll
        for (int u = 0; u < PF; u++) pf[u] = ld4(src + (int64_t)prow[u] * src_rs + chc);
#pragma unroll
        for (int u = 0; u < PF; u++)
            if (chok && g + u * G < cnt) st4(rows + (g + u * G) * SL + l * 4, pf[u]);
    }
    const int r16 = lane & 15;
    const unsigned zoff = (unsigned)P * SL * 4;
    const int elast = E - 1;
    // an entry and the features of its pixel (weight-0 padding entries point at the row of zeros; any pixel's features do)
    auto fetch = [&](int pos, int s1, uint2 &e, float (&f)[NF > 0 ? NF : 1]) {
        e = ent[min(max(pos, 0), elast)];
        if (pos >= s1) e = make_uint2(zoff, 0u);
        const int64_t px = pixl[min((int)(e.x / (SL * 4)), kclamp)];
#pragma unroll
        for (int j = 0; j < NF; j++) f[j] = fref[px * fref_rs + (int64_t)j * fref_cs];
    };
    for (int c0 = 0; c0 < vd; c0 += SL) {
        const int ch = c0 + l * 4;
        const bool chok = ch < vd;
        __syncthreads();                   // rows of this slab are in LDS
        const int slab = c0 / SL;
        if (threadIdx.x == 0) ctr[(slab + 1) & 1] = NW;
        const int chn = ch + SL;
        const bool more = c0 + SL < vd;
        const bool chnok = more && chn < vd;
        const int chnc = chnok ? chn : 0;
        int *slab_ctr = ctr + (slab & 1);
        const int nlong = ctr[2];
        const int nitems = nlong + (nv - nlong + Q - 1) / Q;
        for (int gi = wave; gi < nitems;) {
            const bool coop = gi < nlong;
            const int i = coop ? gi : nlong + (gi - nlong) * Q + q;
            int2 m = make_int2(0, 0);
            if (i < nv) m = meta[i];
            int nxt = 0;
            if (lane == 0) nxt = atomicAdd(slab_ctr, 1);
            const int s1 = (int)((unsigned)m.x >> 16);
            int s = m.x & 0xFFFF;
            float4 acc[NS];
#pragma unroll
            for (int t = 0; t < NS; t++) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int len = s1 - s;
            int lmax = __builtin_amdgcn_readlane(len, 0);
            lmax = max(lmax, __builtin_amdgcn_readlane(len, 32));
            lmax = max(max(lmax, __builtin_amdgcn_readlane(len, 16)), __builtin_amdgcn_readlane(len, 48));
            const int step = coop ? 16 * Q : 16;
            if (coop) s += 16 * q;
            uint2 e;
            float f[NF > 0 ? NF : 1];
            fetch(s + r16, s1, e, f);
            for (int b = 0; b < lmax; b += step) {
                uint2 en;
                float fn[NF > 0 ? NF : 1];
                fetch(s + b + step + r16, s1, en, fn);       // next sixteen, under this batch's work
                sum4w<0, NS>(acc, e, f, rbase);
                sum4w<4, NS>(acc, e, f, rbase);
                if (b + 8 < lmax) {
                    sum4w<8, NS>(acc, e, f, rbase);
                    sum4w<12, NS>(acc, e, f, rbase);
                }
                e = en;
#pragma unroll
                for (int j = 0; j < NF; j++) f[j] = fn[j];
            }
            if (coop) {
#pragma unroll
                for (int t = 0; t < NS; t++) {
                    float4 a = acc[t];
                    a = make_float4(a.x + __shfl_xor(a.x, LPRS), a.y + __shfl_xor(a.y, LPRS), a.z + __shfl_xor(a.z, LPRS),
                                    a.w + __shfl_xor(a.w, LPRS));
                    a = make_float4(a.x + __shfl_xor(a.x, 2 * LPRS), a.y + __shfl_xor(a.y, 2 * LPRS), a.z + __shfl_xor(a.z, 2 * LPRS),
                                    a.w + __shfl_xor(a.w, 2 * LPRS));
                    acc[t] = a;
                }
            }
            if (i < nv && chok && !(coop && q != 0)) {
                float *dst = m.y < 0 ? vert + (int64_t)(m.y & 0x7FFFFFFF) * out_rs : partial + (int64_t)m.y * out_rs;
#pragma unroll
                for (int t = 0; t < NS; t++) st4(dst + (int64_t)t * vd + ch, acc[t]);
            }
            gi = __builtin_amdgcn_readfirstlane(nxt);
        }
        __syncthreads();                   // everyone is done reading this slab
        if (more) {
            // next slab's rows: loaded here, not prefetched into registers under the sums (32 VGPRs that decide between one
            // and two workgroups per CU; the other workgroup's sums cover this round trip)
#pragma unroll
            for (int u = 0; u < PF; u++) pf[u] = ld4(src + (int64_t)pixl[min(g + u * G, kclamp)] * src_rs + chnc);
#pragma unroll
            for (int u = 0; u < PF; u++)
                if (chnok && g + u * G < cnt) st4(rows + (g + u * G) * SL + l * 4, pf[u]);
        }
    }
}

// vertices with != 1 contributing chunk: sum their partial rows in ascending chunk order
// (0 chunks = ghost vertex of a neighbouring row band: zeros).  One lane group per vertex, independent waves.
// Vertices with more than `long_list` rows (LONG_LIST, phl_internal.h) are left to k_splat_reduce_long.
template <int LPR>
__global__ __launch_bounds__(256) void k_splat_reduce(const float *__restrict__ partial, const int *__restrict__ vs_ptr,
                                                      const phl_contrib_t *__restrict__ vs,
                                                      const int *__restrict__ slot_pidx, int M, int vd,
                                                      float *__restrict__ vert, const int *__restrict__ vlist, int long_list,
                                                      const int *__restrict__ pack_pos, float *__restrict__ pack, int64_t pack_rs)
{
    // vlist (optional): only these M vertex rows (phl_splat_part); pack_pos (optional, with vlist): listed row i is also
    // written to pack[pack_pos[i]] -- the row-band exchange's send buffer filled by the kernel that completes the rows
    constexpr int Gw = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR, l = lane % LPR;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4 * Gw;
    auto add4 = [](float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
    for (int64_t v0 = (int64_t)wave * Gw; v0 < M; v0 += stride) {
        if (v0 + sub >= M) continue;
        const int64_t v = vlist ? vlist[v0 + sub] : v0 + sub;
        const int beg = vs_ptr[v], end = vs_ptr[v + 1];
        const int pp = pack_pos ? pack_pos[v0 + sub] : -1;
        if (end - beg > long_list) continue;
        if (end - beg == 1) {
            // the chunk kernel wrote the row itself (launches before this one): only the copy into the send buffer is left
            if (pp >= 0)
                for (int ch = l * 4; ch < vd; ch += LPR * 4) st4(pack + (int64_t)pp * pack_rs + ch, ld4(vert + v * vd + ch));
            continue;
        }
        for (int ch = l * 4; ch < vd; ch += LPR * 4) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int e = beg;
            for (; e + 4 <= end; e += 4) {
                const float4 q0 = ld4(partial + (int64_t)__float_as_int(vs[e].w) * vd + ch);
                const float4 q1 = ld4(partial + (int64_t)__float_as_int(vs[e + 1].w) * vd + ch);
                const float4 q2 = ld4(partial + (int64_t)__float_as_int(vs[e + 2].w) * vd + ch);
                const float4 q3 = ld4(partial + (int64_t)__float_as_int(vs[e + 3].w) * vd + ch);
                acc = add4(add4(add4(add4(acc, q0), q1), q2), q3);
            }
            for (; e < end; e++) acc = add4(acc, ld4(partial + (int64_t)__float_as_int(vs[e].w) * vd + ch));
            st4(vert + v * vd + ch, acc);
            if (pp >= 0) st4(pack + (int64_t)pp * pack_rs + ch, acc);
        }
    }
}

// A vertex fed by MANY chunks (a flat image region spans hundreds of 16x16 tiles: natural images at M/n ~ 0.01
// have vertices with 100-600 partial rows, which one wave would add up one dependent load after the other) is
// summed by a whole workgroup: lane group j of the 256/LPR groups adds rows j, j+NG, ... (four loads in flight
// each) and the NG sums are added in ascending j -- a fixed order, so the result does not depend on scheduling.
// One workgroup per entry of `list` (the lattice's long vertices, or the caller's rows: then short ones exit).
template <int LPR>
__global__ __launch_bounds__(256) void k_splat_reduce_long(const float *__restrict__ partial, const int *__restrict__ vs_ptr,
                                                           const phl_contrib_t *__restrict__ vs,
                                                           const int *__restrict__ slot_pidx, int vd,
                                                           float *__restrict__ vert, const int *__restrict__ list, int long_list,
                                                           const int *__restrict__ pack_pos, float *__restrict__ pack, int64_t pack_rs)
{
    constexpr int NG = 256 / LPR;
    __shared__ float4 red[256];
    const int l = (int)threadIdx.x % LPR, jg = (int)threadIdx.x / LPR;
    const int64_t v = list[blockIdx.x];
    const int b0 = vs_ptr[v], b1 = vs_ptr[v + 1];
    if (b1 - b0 <= long_list) return;                       // workgroup-uniform
    auto add4 = [](float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
    for (int c0 = 0; c0 < vd; c0 += LPR * 4) {              // uniform trip count: there are barriers inside
        const bool chok = c0 + l * 4 < vd;
        const int ch = chok ? c0 + l * 4 : 0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int e = b0 + jg;
        for (; e + 7 * NG < b1; e += 8 * NG) {               // eight row loads in flight per lane group
            float4 q[8];
#pragma unroll
            for (int u = 0; u < 8; u++) q[u] = ld4(partial + (int64_t)__float_as_int(vs[e + u * NG].w) * vd + ch);
#pragma unroll
            for (int u = 0; u < 8; u++) acc = add4(acc, q[u]);
        }
        for (; e < b1; e += NG) acc = add4(acc, ld4(partial + (int64_t)__float_as_int(vs[e].w) * vd + ch));
        red[threadIdx.x] = acc;
        __syncthreads();
        if (jg == 0 && chok) {
            float4 t = red[l];
            for (int k = 1; k < NG; k++) t = add4(t, red[k * LPR + l]);
            st4(vert + v * vd + ch, t);
            if (pack_pos && pack_pos[blockIdx.x] >= 0) st4(pack + (int64_t)pack_pos[blockIdx.x] * pack_rs + ch, t);
        }
        __syncthreads();
    }
}

// One workgroup per chunk; the SLAB WIDTH IS CHOSEN BY THE WORKGROUP from its own chunk: 2^LSH lanes (of 4 floats)
// per row, the widest (up to `lsh_max`) whose nv staged vertex rows fit next to the index data in the `lds_bytes`
// the launch was given.  A typical chunk of a natural image has 20-60 local vertices and takes all 256 channels in
// one slab, a textured one with 300 takes 32-channel slabs, and neither decides for the other (round 2 sized every
// chunk for the worst one).  A chunk whose rows do not fit even the narrowest slab gathers them from global memory
// (DIRECT: pixels that share next to nothing -- there is nothing to stage).  The width is a template parameter of
// the body (a workgroup-uniform switch in the kernel): with a run-time width the same loops ran 40 % slower.
struct slice_args {
    const float *vert;
    int vd, dp1, cnt, nv;
    float *out;
    int64_t out_rs;
    const float *sub_src;
    int64_t sub_rs;
    float cdiv, rcdiv;
};

template <int LSH, bool EXACT, bool DIRECT>
__device__ __forceinline__ void slice_chunk(const slice_args &a, const uint2 *__restrict__ ent, const int *__restrict__ pixl,
                                            const int *__restrict__ vl, float *__restrict__ rows)
{
    constexpr int LPRS = 1 << LSH;
    constexpr int SL = LPRS * 4;
    constexpr int G = TPB / LPRS;
    const int g = threadIdx.x / LPRS, l = threadIdx.x % LPRS;
    const int vd = a.vd, dp1 = a.dp1, cnt = a.cnt, nv = a.nv;
    for (int c0 = 0; c0 < vd; c0 += SL) {
        const int ch = c0 + l * 4;
        const bool chok = ch < vd;
        const int chc = chok ? ch : 0;
        if (!DIRECT) {
            const int iclamp = nv - 1;
            for (int i0 = g; i0 < nv; i0 += 8 * G) {
                float4 q[8];
#pragma unroll
                for (int u = 0; u < 8; u++) q[u] = ld4(a.vert + (int64_t)vl[min(i0 + u * G, iclamp)] * vd + chc);
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (chok && i0 + u * G < nv) st4(rows + (i0 + u * G) * SL + l * 4, q[u]);
            }
            __syncthreads();
        }
        const char *rbase = reinterpret_cast<const char *>(rows) + l * 16;
        const float *gbase = a.vert + chc;
        auto row = [&](unsigned x) -> float4 {
            if (DIRECT) return ld4(gbase + (int64_t)x * vd);
            return *reinterpret_cast<const float4 *>(rbase + x);
        };
        for (int k = g; k < cnt; k += G) {
            const uint2 *ek = ent + k * dp1;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int r = 0;
            for (; r + 3 <= dp1; r += 3) {
                const uint2 e0 = ek[r], e1 = ek[r + 1], e2 = ek[r + 2];
                const float4 q0 = row(e0.x), q1 = row(e1.x), q2 = row(e2.x);
                if (EXACT) {
                    acc = term4(acc, __uint_as_float(e0.y), q0, a.cdiv, a.rcdiv);
                    acc = term4(acc, __uint_as_float(e1.y), q1, a.cdiv, a.rcdiv);
                    acc = term4(acc, __uint_as_float(e2.y), q2, a.cdiv, a.rcdiv);
                } else {
                    acc = fma4(acc, __uint_as_float(e0.y), q0);
                    acc = fma4(acc, __uint_as_float(e1.y), q1);
                    acc = fma4(acc, __uint_as_float(e2.y), q2);
                }
            }
            for (; r < dp1; r++) {
                const uint2 e0 = ek[r];
                const float4 q0 = row(e0.x);
                if (EXACT) acc = term4(acc, __uint_as_float(e0.y), q0, a.cdiv, a.rcdiv);
                else acc = fma4(acc, __uint_as_float(e0.y), q0);
            }
            if (chok) {
                const int p = pixl[k];
                if (!EXACT) acc = make_float4(acc.x * a.rcdiv, acc.y * a.rcdiv, acc.z * a.rcdiv, acc.w * a.rcdiv);
                if (a.sub_src) {
                    const float4 s = ld4(a.sub_src + (int64_t)p * a.sub_rs + ch);
                    acc = make_float4(acc.x - s.x, acc.y - s.y, acc.z - s.z, acc.w - s.w);
                }
                st4(a.out + (int64_t)p * a.out_rs + ch, acc);
            }
        }
        if (!DIRECT) __syncthreads();
    }
}

template <bool EXACT>
__global__ __launch_bounds__(TPB) void k_slice_tiled(const float *__restrict__ vert, int vd, int n, int P, int dp1,
                                                     int lsh_max, int lds_bytes, const int *__restrict__ pix_order,
                                                     const int *__restrict__ vptr, const int *__restrict__ slot_vert,
                                                     const unsigned short *__restrict__ lidx,
                                                     const phl_replay_t *__restrict__ replay, float *__restrict__ out,
                                                     int64_t out_rs, const float *__restrict__ sub_src, int64_t sub_rs,
                                                     float cdiv, float rcdiv, int nchunks, int xcd_chunk,
                                                     const int *__restrict__ heavy_list, int heavy_n, int heavy_pad, int heavy_thr)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // Heavy chunks first: the first heavy_pad blocks take the heavy_n chunks with more than heavy_thr local vertices
    // (narrow slabs, several times the work of a typical chunk) so that they run under the bulk instead of forming
    // the launch's tail; the other blocks walk all chunks in the XCD-aware order (see k_blur: neighbouring chunks
    // share boundary vertices) and skip those.  heavy_pad is a multiple of 8: the XCD of a chunk does not move.
    int c;
    const bool heavy_block = (int)blockIdx.x < heavy_pad;
    if (heavy_block) {
        if ((int)blockIdx.x >= heavy_n) return;
        c = heavy_list[blockIdx.x];
    } else {
        const int b = (int)blockIdx.x - heavy_pad;
        c = xcd_chunk > 0 ? (b & 7) * xcd_chunk + (b >> 3) : b;
        if (c >= nchunks) return;
    }
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int64_t ebase = (int64_t)base * dp1;
    const int vbase = vptr[c], nv = vptr[c + 1] - vbase;
    if (!heavy_block && nv > heavy_thr) return;
    // index data first (its size does not depend on the slab width), rows behind it
    uint2 *ent = reinterpret_cast<uint2 *>(lds);                    // [P*dp1] {row offset or vertex id, weight}
    int *pixl = reinterpret_cast<int *>(ent + P * dp1);             // [P]
    int *vl = pixl + P;                                             // [nv]
    const int fixed = (P * dp1 * 8 + P * 4 + nv * 4 + 15) & ~15;
    float *rows = reinterpret_cast<float *>(reinterpret_cast<char *>(lds) + fixed);
    int lsh = lsh_max;                                              // workgroup-uniform
    while (lsh > 2 && fixed + (int64_t)nv * (16 << lsh) > lds_bytes) lsh--;
    const bool direct = fixed + (int64_t)nv * (16 << lsh) > lds_bytes;
    if (direct) lsh = lsh_max;
    for (int k = threadIdx.x; k < cnt; k += TPB) pixl[k] = pix_order[base + k];
    if (!direct)
        for (int i = threadIdx.x; i < nv; i += TPB) vl[i] = slot_vert[vbase + i] & 0x7FFFFFFF;
    for (int e = threadIdx.x; e < E; e += TPB) {
        const int k = e / dp1, r = e - k * dp1;
        const int p = pix_order[base + k];
        const unsigned li = lidx[ebase + e];
        // staged: byte offset of the local vertex's LDS row; direct: the vertex id itself
        ent[e] = make_uint2(direct ? (unsigned)(slot_vert[vbase + li] & 0x7FFFFFFF) : li << (lsh + 4),
                            __float_as_uint(replay[(int64_t)p * dp1 + r].w));
    }
    __syncthreads();
    slice_args a;
    a.vert = vert; a.vd = vd; a.dp1 = dp1; a.cnt = cnt; a.nv = nv;
    a.out = out; a.out_rs = out_rs; a.sub_src = sub_src; a.sub_rs = sub_rs; a.cdiv = cdiv; a.rcdiv = rcdiv;
    if (direct) {
        switch (lsh) {
            case 6: slice_chunk<6, EXACT, true>(a, ent, pixl, vl, rows); break;
            case 5: slice_chunk<5, EXACT, true>(a, ent, pixl, vl, rows); break;
            case 4: slice_chunk<4, EXACT, true>(a, ent, pixl, vl, rows); break;
            case 3: slice_chunk<3, EXACT, true>(a, ent, pixl, vl, rows); break;
            default: slice_chunk<2, EXACT, true>(a, ent, pixl, vl, rows); break;
        }
    } else {
        switch (lsh) {
            case 6: slice_chunk<6, EXACT, false>(a, ent, pixl, vl, rows); break;
            case 5: slice_chunk<5, EXACT, false>(a, ent, pixl, vl, rows); break;
            case 4: slice_chunk<4, EXACT, false>(a, ent, pixl, vl, rows); break;
            case 3: slice_chunk<3, EXACT, false>(a, ent, pixl, vl, rows); break;
            default: slice_chunk<2, EXACT, false>(a, ent, pixl, vl, rows); break;
        }
    }
}

// ---- gradient w.r.t. the features: slice of the WIDE vertex buffer, contracted on the fly ---------------------------
// crf/gaussian_matrix.py:450-463 filters [g, g(x)ref, src, src(x)ref] (2L(1+d) channels) and contracts the result to
// [n, d].  Here one pass (x, y) of phl_filter_grad holds the blurred wide vertex rows [M][NS*L] (block 0 = splat of x,
// block 1+k = splat of x (x) ref[:, k]; NS = d+1) and this kernel evaluates, per pixel i,
//     T_ik = -2 / (1 + 2^-d) * ( f_ik * sum_l y_il (Wx)_il  -  sum_l y_il (W(x f_k))_il )
// without writing any sliced row.  Per slab of 4*LG channels the chunk's vertex rows are staged for ALL NS blocks at
// once ([nv][NS][4*LG] floats), so a chunk passes L / (4 LG) barriers-bounded phases, not NS times as many; an
// LG-lane group owns 256 / (512 / LG) pixels and keeps their NS running dot products in registers.  y is read once,
// the vertex array about twice (chunks overlap), [n, d] is written; (Wx) itself is written on request (it is the
// gradient w.r.t. the source when x = g).  The workgroup picks LG = 8 (32-channel slabs) if its rows fit the LDS it
// was given, else 4; DIRECT: chunks that fit neither gather their rows from global memory.
template <int NS, int LG, bool DIRECT>
__device__ __forceinline__ void slice_grad_chunk(const float *__restrict__ vertw, int L, int cnt, int nv,
                                                 const uint2 *ent, const int *pixl, const int *vl, float *rows,   // (one LDS block:
                                                 // NOT restrict -- with it the compiler hoists every pixel's entries and
                                                 // all NS*NS row addresses out of the slab loop and spills 800 bytes per lane)
                                                 const float *__restrict__ y, int64_t y_rs, const float *__restrict__ ref,
                                                 int64_t ref_rs, int64_t ref_cs, float *__restrict__ grad_ref, int accumulate,
                                                 float *__restrict__ wx_out, int64_t wx_rs, float rcdiv)
{
    constexpr int SLG = LG * 4;              // channels per slab
    constexpr int G = TPB / LG;              // lane groups
    constexpr int PPG = 256 / G;             // pixels per group (P <= 256)
    constexpr int PITCH = NS * SLG;          // floats per staged local vertex
    const int g = threadIdx.x / LG, l = threadIdx.x % LG;
    const int64_t vdw = (int64_t)NS * L;
    float acc[PPG][NS];
#pragma unroll
    for (int u = 0; u < PPG; u++)
#pragma unroll
        for (int t = 0; t < NS; t++) acc[u][t] = 0.f;
    const int kclamp = cnt - 1;
    for (int c0 = 0; c0 < L; c0 += SLG) {
        const int ch = c0 + l * 4;
        const bool chok = ch < L;
        const int chc = chok ? ch : 0;
        float4 yv[PPG];
#pragma unroll
        for (int u = 0; u < PPG; u++) yv[u] = ld4(y + (int64_t)pixl[min(g + u * G, kclamp)] * y_rs + chc);
        if (!DIRECT) {
            // [nv][NS][LG] 16-byte pieces, LG consecutive threads on LG consecutive pieces of one (vertex, block)
            const int total = nv * NS * LG;
            for (int i0 = threadIdx.x; i0 < total; i0 += 4 * TPB) {
                float4 q[4];
                int dsto[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = min(i0 + u * TPB, total - 1);
                    const int i = idx / (NS * LG), rem = idx - i * (NS * LG);
                    const int set = rem / LG, ll = rem - set * LG;
                    const int cc = c0 + ll * 4 < L ? c0 + ll * 4 : 0;
                    q[u] = ld4(vertw + (int64_t)vl[i] * vdw + (int64_t)set * L + cc);
                    dsto[u] = i * PITCH + set * SLG + ll * 4;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (i0 + u * TPB < total) st4(rows + dsto[u], q[u]);
            }
            __syncthreads();
        }
        const char *rbase = reinterpret_cast<const char *>(rows) + l * 16;
#pragma unroll
        for (int u = 0; u < PPG; u++) {
            const int k = min(g + u * G, kclamp);
            const bool live = chok && g + u * G < cnt;
            uint2 e[NS];                       // the pixel's d+1 = NS simplex vertices {row offset | vertex id, weight}
            const char *pr[NS];
#pragma unroll
            for (int r = 0; r < NS; r++) {
                e[r] = ent[k * NS + r];
                pr[r] = rbase + e[r].x;         // block `set` of the row: a constant offset from here
            }
#pragma unroll
            for (int set = 0; set < NS; set++) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int r = 0; r < NS; r++) {
                    const float4 q0 = DIRECT ? ld4(vertw + (int64_t)e[r].x * vdw + (int64_t)set * L + chc)
                                             : *reinterpret_cast<const float4 *>(pr[r] + set * (SLG * 4));
                    v = fma4(v, __uint_as_float(e[r].y), q0);
                }
                const float dot = yv[u].x * v.x + yv[u].y * v.y + yv[u].z * v.z + yv[u].w * v.w;
                acc[u][set] += live ? dot : 0.f;
                if (set == 0 && wx_out && live)
                    st4(wx_out + (int64_t)pixl[k] * wx_rs + ch, make_float4(v.x * rcdiv, v.y * rcdiv, v.z * rcdiv, v.w * rcdiv));
                // one (pixel, block) at a time: left alone, the compiler issues all NS*NS row reads of a pixel first and
                // spills them (800 bytes of scratch per lane); sched_barrier did not stop that, this does
                asm volatile("" : "+v"(acc[u][set])::"memory");
            }
        }
        if (!DIRECT) __syncthreads();
    }
    // the LG lanes of a group hold a slab's channels between them: add their dot products
#pragma unroll
    for (int u = 0; u < PPG; u++)
#pragma unroll
        for (int t = 0; t < NS; t++) {
            float a = acc[u][t];
#pragma unroll
            for (int o = LG / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, LG);
            acc[u][t] = a;
        }
    if (l == 0) {
#pragma unroll
        for (int u = 0; u < PPG; u++) {
            const int k = g + u * G;
            if (k >= cnt) continue;
            const int64_t p = pixl[k];
#pragma unroll
            for (int t = 1; t < NS; t++) {
                const float f = ref[p * ref_rs + (int64_t)(t - 1) * ref_cs];
                const float val = -2.f * rcdiv * (f * acc[u][0] - acc[u][t]);
                float *dst = grad_ref + p * (NS - 1) + (t - 1);
                *dst = accumulate ? *dst + val : val;
            }
        }
    }
}

template <int NS>
__global__ __launch_bounds__(TPB) void k_slice_grad(const float *__restrict__ vertw, int L, int n, int P, int lds_bytes,
                                                    const int *__restrict__ pix_order, const int *__restrict__ vptr,
                                                    const int *__restrict__ slot_vert, const unsigned short *__restrict__ lidx,
                                                    const phl_replay_t *__restrict__ replay, const float *__restrict__ y,
                                                    int64_t y_rs, const float *__restrict__ ref, int64_t ref_rs, int64_t ref_cs,
                                                    float *__restrict__ grad_ref, int accumulate, float *__restrict__ wx_out,
                                                    int64_t wx_rs, float rcdiv, int nchunks, int xcd_chunk)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int dp1 = NS;
    const int c = xcd_chunk > 0 ? (int)(blockIdx.x & 7) * xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (c >= nchunks) return;
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int64_t ebase = (int64_t)base * dp1;
    const int vbase = vptr[c], nv = vptr[c + 1] - vbase;
    uint2 *ent = reinterpret_cast<uint2 *>(lds);
    int *pixl = reinterpret_cast<int *>(ent + P * dp1);
    int *vl = pixl + P;
    const int fixed = (P * dp1 * 8 + P * 4 + nv * 4 + 15) & ~15;
    float *rows = reinterpret_cast<float *>(reinterpret_cast<char *>(lds) + fixed);
    // workgroup-uniform choice: 32-channel slabs, 16-channel slabs, or no staging
    const int mode = fixed + (int64_t)nv * (NS * 128) <= lds_bytes ? 8 : (fixed + (int64_t)nv * (NS * 64) <= lds_bytes ? 4 : 0);
    const unsigned pitch_bytes = (unsigned)NS * (mode == 8 ? 128u : 64u);
    for (int k = threadIdx.x; k < cnt; k += TPB) pixl[k] = pix_order[base + k];
    if (mode)
        for (int i = threadIdx.x; i < nv; i += TPB) vl[i] = slot_vert[vbase + i] & 0x7FFFFFFF;
    for (int e = threadIdx.x; e < E; e += TPB) {
        const int k = e / dp1, r = e - k * dp1;
        const int p = pix_order[base + k];
        const unsigned li = lidx[ebase + e];
        ent[e] = make_uint2(mode ? li * pitch_bytes : (unsigned)(slot_vert[vbase + li] & 0x7FFFFFFF),
                            __float_as_uint(replay[(int64_t)p * dp1 + r].w));
    }
    __syncthreads();
    if (mode == 8)
        slice_grad_chunk<NS, 8, false>(vertw, L, cnt, nv, ent, pixl, vl, rows, y, y_rs, ref, ref_rs, ref_cs, grad_ref, accumulate,
                                       wx_out, wx_rs, rcdiv);
    else if (mode == 4)
        slice_grad_chunk<NS, 4, false>(vertw, L, cnt, nv, ent, pixl, vl, rows, y, y_rs, ref, ref_rs, ref_cs, grad_ref, accumulate,
                                       wx_out, wx_rs, rcdiv);
    else
        slice_grad_chunk<NS, 8, true>(vertw, L, cnt, nv, ent, pixl, vl, rows, y, y_rs, ref, ref_rs, ref_cs, grad_ref, accumulate,
                                      wx_out, wx_rs, rcdiv);
}

// ---- the same contraction for a GROUP of features (d = 8..16, or a forced split) ----------------------------------------
// k_slice_grad uses one number, NS = d + 1, for two things: the simplex vertices of a pixel and the blocks of a staged
// row.  phl_filter_grad runs d > 7 in feature groups [k0, k0 + NB - 1): the wide rows then hold NB = 1 + (group size)
// <= 8 blocks (block 0 = W x, block t = W(x f_{k0+t-1})) while a pixel still has nvp = d + 1 vertices.  NB stays a
// compile-time value (the accumulators), nvp is a run-time one: the loop over a pixel's vertices is the OUTER one --
// one entry read per vertex -- and feeds NB running rows v[t]; the NB dots with y follow.  That is NB float4 of row
// sums per pixel and PPG * NB accumulators per lane, and no table of NS x NS row addresses for the compiler to hoist:
// 98 .. 246 registers at NB = 2 .. 8, no scratch.  Block 0 sums the vertices in the order k_slice_grad does: W x has
// the same bits.
// Same LDS layout ([nv][NB][4 LG] floats after the index data, entries [P][nvp]) and the same three forms.
template <int NB, int LG, bool DIRECT>
__device__ __forceinline__ void slice_grad_group_chunk(const float *__restrict__ vertw, int L, int cnt, int nv, int nvp,
                                                       const uint2 *ent, const int *pixl, const int *vl, float *rows,   // (one LDS
                                                       // block, not restrict: see slice_grad_chunk)
                                                       const float *__restrict__ y, int64_t y_rs, const float *__restrict__ ref,
                                                       int64_t ref_rs, int64_t ref_cs, float *__restrict__ grad_ref, int d, int k0,
                                                       int accumulate, float *__restrict__ wx_out, int64_t wx_rs, float rcdiv)
{
    constexpr int SLG = LG * 4;              // channels per slab
    constexpr int G = TPB / LG;              // lane groups
    constexpr int PPG = 256 / G;             // pixels per group (P <= 256)
    constexpr int PITCH = NB * SLG;          // floats per staged local vertex
    const int g = threadIdx.x / LG, l = threadIdx.x % LG;
    const int64_t vdw = (int64_t)NB * L;
    float acc[PPG][NB];
#pragma unroll
    for (int u = 0; u < PPG; u++)
#pragma unroll
        for (int t = 0; t < NB; t++) acc[u][t] = 0.f;
    const int kclamp = cnt - 1;
    for (int c0 = 0; c0 < L; c0 += SLG) {
        const int ch = c0 + l * 4;
        const bool chok = ch < L;
        const int chc = chok ? ch : 0;
        float4 yv[PPG];
#pragma unroll
        for (int u = 0; u < PPG; u++) yv[u] = ld4(y + (int64_t)pixl[min(g + u * G, kclamp)] * y_rs + chc);
        if (!DIRECT) {
            // [nv][NB][LG] 16-byte pieces, LG consecutive threads on LG consecutive pieces of one (vertex, block)
            const int total = nv * NB * LG;
            for (int i0 = threadIdx.x; i0 < total; i0 += 4 * TPB) {
                float4 q[4];
                int dsto[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = min(i0 + u * TPB, total - 1);
                    const int i = idx / (NB * LG), rem = idx - i * (NB * LG);
                    const int set = rem / LG, ll = rem - set * LG;
                    const int cc = c0 + ll * 4 < L ? c0 + ll * 4 : 0;
                    q[u] = ld4(vertw + (int64_t)vl[i] * vdw + (int64_t)set * L + cc);
                    dsto[u] = i * PITCH + set * SLG + ll * 4;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (i0 + u * TPB < total) st4(rows + dsto[u], q[u]);
            }
            __syncthreads();
        }
        const char *rbase = reinterpret_cast<const char *>(rows) + l * 16;
#pragma unroll
        for (int u = 0; u < PPG; u++) {
            const int k = min(g + u * G, kclamp);
            const bool live = chok && g + u * G < cnt;
            const uint2 *pe = ent + k * nvp;   // the pixel's d+1 simplex vertices {row offset | vertex id, weight}
            float4 v[NB];
#pragma unroll
            for (int t = 0; t < NB; t++) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            uint2 en = pe[0];
#pragma unroll 1
            for (int r = 0; r < nvp; r++) {
                const uint2 e = en;
                en = pe[min(r + 1, nvp - 1)];      // the next vertex's entry, under this one's row reads
                const float w = __uint_as_float(e.y);
                const char *pr = rbase + e.x;
                const float *gr = vertw + (int64_t)e.x * vdw + chc;
#pragma unroll
                for (int t = 0; t < NB; t++) {
                    const float4 q0 = DIRECT ? ld4(gr + (int64_t)t * L) : *reinterpret_cast<const float4 *>(pr + t * (SLG * 4));
                    v[t] = fma4(v[t], w, q0);
                }
            }
#pragma unroll
            for (int t = 0; t < NB; t++) {
                const float dot = yv[u].x * v[t].x + yv[u].y * v[t].y + yv[u].z * v[t].z + yv[u].w * v[t].w;
                acc[u][t] += live ? dot : 0.f;
            }
            if (wx_out && live)
                st4(wx_out + (int64_t)pixl[k] * wx_rs + ch, make_float4(v[0].x * rcdiv, v[0].y * rcdiv, v[0].z * rcdiv, v[0].w * rcdiv));
            // (no scheduling barrier between the pixels, unlike slice_grad_chunk: the compiler runs the PPG vertex loops
            // side by side -- 246 registers at NB = 8, no scratch -- and that is the faster form where most chunks
            // gather from memory: 28.5 against 30.6 ms for a d = 8 backward at 1110 x 1390 x 64, equal at d = 16)
        }
        if (!DIRECT) __syncthreads();
    }
    // the LG lanes of a group hold a slab's channels between them: add their dot products
#pragma unroll
    for (int u = 0; u < PPG; u++)
#pragma unroll
        for (int t = 0; t < NB; t++) {
            float a = acc[u][t];
#pragma unroll
            for (int o = LG / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, LG);
            acc[u][t] = a;
        }
    if (l == 0) {
#pragma unroll
        for (int u = 0; u < PPG; u++) {
            const int k = g + u * G;
            if (k >= cnt) continue;
            const int64_t p = pixl[k];
#pragma unroll
            for (int t = 1; t < NB; t++) {
                const float f = ref[p * ref_rs + (int64_t)(k0 + t - 1) * ref_cs];
                const float val = -2.f * rcdiv * (f * acc[u][0] - acc[u][t]);
                float *dst = grad_ref + p * d + (k0 + t - 1);
                *dst = accumulate ? *dst + val : val;
            }
        }
    }
}

template <int NB>
__global__ __launch_bounds__(TPB) void k_slice_grad_group(const float *__restrict__ vertw, int L, int n, int P, int dp1, int k0,
                                                          int lds_bytes, const int *__restrict__ pix_order,
                                                          const int *__restrict__ vptr, const int *__restrict__ slot_vert,
                                                          const unsigned short *__restrict__ lidx,
                                                          const phl_replay_t *__restrict__ replay, const float *__restrict__ y,
                                                          int64_t y_rs, const float *__restrict__ ref, int64_t ref_rs, int64_t ref_cs,
                                                          float *__restrict__ grad_ref, int accumulate, float *__restrict__ wx_out,
                                                          int64_t wx_rs, float rcdiv, int nchunks, int xcd_chunk)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int c = xcd_chunk > 0 ? (int)(blockIdx.x & 7) * xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (c >= nchunks) return;
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int64_t ebase = (int64_t)base * dp1;
    const int vbase = vptr[c], nv = vptr[c + 1] - vbase;
    uint2 *ent = reinterpret_cast<uint2 *>(lds);
    int *pixl = reinterpret_cast<int *>(ent + P * dp1);
    int *vl = pixl + P;
    const int fixed = (P * dp1 * 8 + P * 4 + nv * 4 + 15) & ~15;      // (the launcher gives at least this much)
    float *rows = reinterpret_cast<float *>(reinterpret_cast<char *>(lds) + fixed);
    // workgroup-uniform choice: 32-channel slabs, 16-channel slabs, or no staging
    const int mode = fixed + (int64_t)nv * (NB * 128) <= lds_bytes ? 8 : (fixed + (int64_t)nv * (NB * 64) <= lds_bytes ? 4 : 0);
    const unsigned pitch_bytes = (unsigned)NB * (mode == 8 ? 128u : 64u);
    for (int k = threadIdx.x; k < cnt; k += TPB) pixl[k] = pix_order[base + k];
    if (mode)
        for (int i = threadIdx.x; i < nv; i += TPB) vl[i] = slot_vert[vbase + i] & 0x7FFFFFFF;
    for (int e = threadIdx.x; e < E; e += TPB) {
        const int k = e / dp1, r = e - k * dp1;
        const int p = pix_order[base + k];
        const unsigned li = lidx[ebase + e];
        ent[e] = make_uint2(mode ? li * pitch_bytes : (unsigned)(slot_vert[vbase + li] & 0x7FFFFFFF),
                            __float_as_uint(replay[(int64_t)p * dp1 + r].w));
    }
    __syncthreads();
    const int d = dp1 - 1;
    if (mode == 8)
        slice_grad_group_chunk<NB, 8, false>(vertw, L, cnt, nv, dp1, ent, pixl, vl, rows, y, y_rs, ref, ref_rs, ref_cs, grad_ref, d, k0,
                                             accumulate, wx_out, wx_rs, rcdiv);
    else if (mode == 4)
        slice_grad_group_chunk<NB, 4, false>(vertw, L, cnt, nv, dp1, ent, pixl, vl, rows, y, y_rs, ref, ref_rs, ref_cs, grad_ref, d, k0,
                                             accumulate, wx_out, wx_rs, rcdiv);
    else
        slice_grad_group_chunk<NB, 8, true>(vertw, L, cnt, nv, dp1, ent, pixl, vl, rows, y, y_rs, ref, ref_rs, ref_cs, grad_ref, d, k0,
                                            accumulate, wx_out, wx_rs, rcdiv);
}

// LDS per workgroup: default 80 KiB -> two workgroups per CU (160 KiB LDS per CU on gfx950)
int lds_budget()
{
    static int b = [] {
        const char *e = getenv("PHL_TILE_LDS");
        int v = e ? atoi(e) : 80 * 1024;
        return v < 8192 ? 8192 : (v > 160 * 1024 ? 160 * 1024 : v);
    }();
    return b;
}

// bytes of index data staged next to the rows (entries, pixel ids, local pointers)
inline int64_t lds_extra(int P, int dp1, int nv_max) { return (int64_t)P * dp1 * 8 + (int64_t)P * 4 + ((int64_t)nv_max + 2) * 8 + 16 + 256; }
// k_slice_tiled keeps less: entries, pixel ids, one vertex id per local vertex

// Launch configuration of a chunk kernel: lanes (of 4 floats) per slab row and LDS bytes per workgroup.
// Candidates in order of preference: every slab width, widest first, at two workgroups per CU (80 KiB); only then
// the same widths at one workgroup per CU.  Measured on C3: the splat with 128-channel slabs and one workgroup per
// CU takes 0.96 ms against 0.78 with 64-channel slabs and two; at M/n = 0.5 64 channels / one workgroup 2.0 ms
// against 1.47 with 32 channels / two -- a second workgroup hides the staging round trips of the first.
struct tile_cfg {
    int lprs = -1;
    size_t lds = 0;
    int cap = 0;        // most local vertices a chunk may have under this configuration
};
inline int64_t lds_big() { return lds_budget() > 160 * 1024 ? lds_budget() : 160 * 1024; }

// k-th candidate for `vd` channels (k = 0 is the preferred one); returns false past the last
inline bool cfg_candidate(int vd, int k, int *lprs, int64_t *budget)
{
    const int need = (vd + 3) / 4;
    int w = 4;
    while (w < 64 && w < need) w <<= 1;
    static const int max_w = getenv("PHL_MAX_LPRS_SPLAT") ? atoi(getenv("PHL_MAX_LPRS_SPLAT")) : 64;   // experiments
    while (w > 4 && w > max_w) w >>= 1;
    int nw = 0;
    for (int x = w; x >= 4; x >>= 1) nw++;
    if (k >= 2 * nw) return false;
    *lprs = w >> (k % nw);
    *budget = k / nw ? lds_big() : lds_budget();
    return true;
}

inline int64_t splat_lds(int P, int dp1, int lprs, int nv) { return (int64_t)(P + 1) * lprs * 16 + lds_extra(P, dp1, nv); }

// first candidate that holds a chunk of `nv` local vertices, sized for exactly that many
inline tile_cfg pick_cfg(const phl_lattice *lat, int vd, int nv)
{
    tile_cfg c;
    int lprs;
    int64_t budget;
    const int P = lat->P, dp1 = lat->d + 1;
    for (int k = 0; cfg_candidate(vd, k, &lprs, &budget); k++) {
        const int64_t need = splat_lds(P, dp1, lprs, nv);
        if (need > budget) continue;
        c.lprs = lprs;
        c.cap = nv;
        c.lds = (size_t)need;
        return c;
    }
    return c;
}

// Chunk classes.  A launch's LDS layout is sized by the most local vertices a chunk of it may have.  Sizing every
// chunk for the worst one (round 2) lets a single textured 16x16 tile narrow the slabs of the whole image: natural
// images at M/n ~ 0.01 have 30 vertices in a typical chunk and 300 in the worst (0.3 % of the chunks above 158).
// So the chunks are cut into classes by their vertex count, one launch per class: walking the candidate
// configurations in order of preference, each one takes the chunks it can hold that no better one took (a class of
// fewer than MIN_CLASS chunks is left to the next candidate).  The largest class runs over the whole grid in
// chunk order (chunks of other classes exit at once); the others are contiguous ranges of `chunk_by_nv` (chunk
// ids by descending vertex count, built with the lattice).
struct tile_class {
    tile_cfg cfg;
    int lo, hi;         // chunks with lo < nv <= hi
    int begin, count;   // range of chunk_by_nv
    bool full_grid;
};
struct tile_plan {
    tile_class cls[12];
    int n = 0;
};
constexpr int MIN_CLASS = 64;
// chunks with more than nv local vertices
inline int chunks_above(const phl_lattice *lat, int nv) { return nv >= lat->nv_max ? 0 : lat->nchunks - lat->nv_cum[nv < 0 ? 0 : nv]; }

inline tile_plan plan_tiles(const phl_lattice *lat, int vd)
{
    tile_plan p;
    const tile_cfg all = pick_cfg(lat, vd, lat->nv_max);
    if (all.lprs < 0) return p;
    static const bool classes = !(getenv("PHL_CLASSES") && atoi(getenv("PHL_CLASSES")) == 0);
    const int P = lat->P, dp1 = lat->d + 1;
    int covered = -1;                                         // chunks with nv <= covered are taken
    if (classes && lat->nv_cum && lat->chunk_by_nv) {
        int lprs;
        int64_t budget;
        for (int k = 0; covered < lat->nv_max && cfg_candidate(vd, k, &lprs, &budget); k++) {
            const int64_t base = splat_lds(P, dp1, lprs, 0);
            if (base > budget) continue;
            const int64_t per_v = 8;
            int cap = (int)((budget - base) / per_v);
            if (cap > lat->nv_max) cap = lat->nv_max;
            if (cap <= covered) continue;
            const int count = chunks_above(lat, covered) - chunks_above(lat, cap);
            if (cap < lat->nv_max && count < MIN_CLASS) continue;
            if (count == 0) { covered = cap; continue; }
            // a class of at most one chunk per CU is all tail: occupancy buys nothing, half the slabs halve its time
            if (count <= 256) {
                int wmax = 4;
                while (wmax < 64 && wmax < (vd + 3) / 4) wmax <<= 1;
                for (int x = wmax; x > lprs; x >>= 1)
                    if (splat_lds(P, dp1, x, cap) <= lds_big()) { lprs = x; break; }
            }
            tile_class &c = p.cls[p.n++];
            c.cfg.lprs = lprs;
            c.cfg.cap = cap;
            c.cfg.lds = (size_t)splat_lds(P, dp1, lprs, cap);
            c.lo = covered;
            c.hi = cap;
            c.begin = chunks_above(lat, cap);
            c.count = count;
            c.full_grid = false;
            covered = cap;
            if (p.n == 11) break;
        }
    }
    if (covered < lat->nv_max) {                              // no classes, or candidates exhausted: `all` takes the rest
        tile_class &c = p.cls[p.n++];
        c.cfg = all;
        c.lo = covered;
        c.hi = 0x7FFFFFFF;
        c.begin = 0;
        c.count = chunks_above(lat, covered);
        c.full_grid = false;
    }
    int big = 0;
    for (int i = 1; i < p.n; i++)
        if (p.cls[i].count > p.cls[big].count) big = i;
    p.cls[big].full_grid = true;
    if (p.n == 1) { p.cls[0].lo = -1; p.cls[0].hi = 0x7FFFFFFF; }
    static const bool dbg = getenv("PHL_DEBUG") != nullptr;
    if (dbg)
        for (int i = 0; i < p.n; i++)
            fprintf(stderr, "[phl] splat vd=%d class %d/%d: %d < nv <= %d, %d chunks, %d lanes, %zu B LDS%s\n",
                    vd, i, p.n, p.cls[i].lo, p.cls[i].hi, p.cls[i].count, p.cls[i].cfg.lprs, p.cls[i].cfg.lds,
                    p.cls[i].full_grid ? " (whole grid)" : "");
    return p;
}

// The slice picks its slab width per workgroup (k_slice_tiled); the launch only fixes the widest slab worth
// having (as wide as vd) and the LDS per workgroup: what the worst chunk needs at that width, at most the budget
// of two workgroups per CU (the index data alone, P*(8(d+1)+4) bytes, is always below it).
struct slice_cfg {
    int lsh_max;
    size_t lds;
};
inline slice_cfg plan_slice(const phl_lattice *lat, int vd)
{
    const int need = (vd + 3) / 4;
    int lsh = 2;
    while (lsh < 6 && (1 << lsh) < need) lsh++;
    static const int max_w = getenv("PHL_MAX_LPRS_SLICE") ? atoi(getenv("PHL_MAX_LPRS_SLICE")) : 64;   // experiments
    while (lsh > 2 && (1 << lsh) > max_w) lsh--;
    const int P = lat->P, dp1 = lat->d + 1;
    const int64_t fixed = (((int64_t)P * dp1 * 8 + (int64_t)P * 4 + (int64_t)lat->nv_max * 4 + 15) & ~(int64_t)15);
    int64_t lds = fixed + (int64_t)lat->nv_max * (16 << lsh);
    if (lds > lds_budget()) lds = lds_budget();     // chunks that do not fit take narrower slabs, or go direct
    slice_cfg c;
    c.lsh_max = lsh;
    c.lds = (size_t)lds;
    return c;
}

template <typename K>
inline int allow_lds(K kernel, size_t bytes, int threads = 512)
{
    const int rc = phl_allow_lds(kernel, bytes);
    if (rc != PHL_OK) return rc;
    static const bool dbg = getenv("PHL_DEBUG") != nullptr;
    if (dbg) {
        int nb = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(kernel), threads, bytes);
        fprintf(stderr, "[phl] chunk kernel: %d threads, %zu B LDS -> %d workgroups per CU (occupancy API)\n", threads, bytes, nb);
    }
    return PHL_OK;
}

inline int pick_lpr_row(int vd)
{
    const int need = (vd + 3) / 4;
    return need >= 64 ? 64 : need >= 16 ? 16 : need >= 4 ? 4 : 1;
}

}  // namespace

// Is the LDS-staged path available for this channel count?
int phl_tiles_lprs(const phl_lattice *lat, int vd, int for_slice)
{
    if (lat->nchunks == 0 || vd % 4 != 0) return -1;
    if (for_slice) return 1 << plan_slice(lat, vd).lsh_max;      // any chunk: the workgroup picks its own slab width
    return pick_cfg(lat, vd, lat->nv_max).lprs;
}

int phl_launch_splat_tiled(phl_lattice *lat, const float *src, int64_t src_rs, int vd, float *vert, float *partial,
                           hipStream_t st, const phl_splat_opts &o)
{
    const phl_splat_wide *const wide = o.wide;
    if (o.pack_pos && (!o.subset || wide)) { phl_set_error("tiled splat: row packing needs a row list and a plain splat"); return PHL_ERR_INVALID; }
    // wide: vertex / partial rows of wide->nsets * vd floats, block k+1 = splat of src (x) fref[:, k] (k_splat_tiled)
    const int64_t out_rs = (int64_t)vd * (wide ? wide->nsets : 1);
    const int M = o.subset ? (int)o.nvl : (int)lat->M;
    if (lat->M == 0 || vd == 0) return PHL_OK;
    const tile_plan plan = plan_tiles(lat, vd);
    if (plan.n == 0) {
        phl_set_error("tiled splat: chunk does not fit LDS");
        return PHL_ERR_UNSUPPORTED;
    }
    int rc = PHL_OK;
    const int nrun = o.subset ? o.nlist : lat->nchunks;
    static const char *tl_path = getenv("PHL_TIMELINE");     // debug: dump per-workgroup time stamps of the main launch
    phl_dev_block<unsigned long long> tl(st);               // (an early exit waits for the stream, then frees it)
    size_t tl_n = 0;
    // the small classes go first, on a forked high-priority stream, and run beside the main grid (see phl_fork_guard);
    // any early return below drains that stream and gives the slot back (the guard's destructor)
    static const bool side_classes = !(getenv("PHL_SIDE_CLASSES") && atoi(getenv("PHL_SIDE_CLASSES")) == 0);
    phl_fork_guard fk;
    if (plan.n > 1 && !o.subset && !tl_path && side_classes) fk.fork(st);
    hipStream_t const st_main = st;
    int order[12];
    int no = 0;
    for (int ci = 0; ci < plan.n; ci++)
        if (!plan.cls[ci].full_grid) order[no++] = ci;
    for (int ci = 0; ci < plan.n; ci++)
        if (plan.cls[ci].full_grid) order[no++] = ci;
    for (int oi = 0; oi < plan.n && rc == PHL_OK && nrun > 0; oi++) {
        const int ci = fk ? order[oi] : oi;
        const tile_class &c = plan.cls[ci];
        st = (fk && !c.full_grid) ? fk.stream() : st_main;
        // the largest class (and every class of a caller's subset) walks the whole grid / list in chunk order and
        // filters by vertex count in the kernel; the others run exactly their range of chunk_by_nv
        const bool filtered = o.subset || c.full_grid;
        const int *list = o.subset ? o.chunk_list : (c.full_grid ? nullptr : lat->chunk_by_nv + c.begin);
        const int cnt = filtered ? nrun : c.count;
        if (cnt == 0) continue;
        int xcd_chunk;
        const unsigned cgrid = phl_xcd_grid(cnt, &xcd_chunk);
        unsigned long long *tlc = nullptr;
        if (tl_path && c.full_grid && !tl.get()) {
            tl_n = (size_t)cgrid * 8;
            PHL_TRY(tl.alloc(tl_n));
            tlc = tl.get();
            PHL_HIP(hipMemsetAsync(tlc, 0, tl_n * 8, st));
        }
        const char *env1 = getenv("PHL_WIDE_ONE_PHASE");            // read per call: the parity test toggles it
        const bool one_phase = !(env1 && atoi(env1) == 0);
        if (wide && one_phase && c.cfg.lprs == 16 && wide->nsets >= 2 && wide->nsets <= 8 && lat->P <= 256) {
            // every LDS row read feeds all nsets accumulators (k_splat_wide)
            // (all d features: the instantiation with d + 1 entries per pixel built in; a feature group: the run-time one)
            const bool all_sets = wide->nsets == lat->d + 1;
            dispatch_int<2, 3, 4, 5, 6, 7, 8>(wide->nsets, [&](auto N) {
                constexpr int NS = decltype(N)::value;
                auto launch = [&](auto kernel) {
                    if ((rc = allow_lds(kernel, c.cfg.lds)) != PHL_OK) return;
                    kernel<<<dim3(cgrid), dim3(TPB_S), c.cfg.lds, st>>>(
                        src, src_rs, vd, (int)lat->n, lat->P, c.cfg.cap, lat->pix_order, lat->chunk_vptr, lat->slot_vert, lat->slot_pidx,
                        lat->seg_rng, lat->seg, vert, partial, cnt, xcd_chunk, list, c.lo, c.hi, long_seg(), wide->fref, wide->rs,
                        wide->cs, lat->d + 1);
                };
                if (all_sets) launch(k_splat_wide<NS, NS>);
                else launch(k_splat_wide<NS, 0>);
            });
            continue;
        }
        auto splat = [&](auto L) {
            constexpr int LPRS = decltype(L)::value;
            if ((rc = allow_lds(k_splat_tiled<LPRS>, c.cfg.lds)) != PHL_OK) return;
            k_splat_tiled<LPRS><<<dim3(cgrid), dim3(TPB_S), c.cfg.lds, st>>>(
                src, src_rs, vd, (int)lat->n, lat->P, lat->d + 1, c.cfg.cap, lat->pix_order, lat->chunk_vptr, lat->slot_vert,
                lat->slot_pidx, lat->seg_rng, lat->seg, vert, partial, cnt, xcd_chunk, tlc, list, c.lo, c.hi, long_seg(),
                wide ? wide->nsets : 1, wide ? wide->fref : nullptr, wide ? wide->rs : 0, wide ? wide->cs : 0, out_rs);
        };
        if (!dispatch_int<64, 32, 16, 8>(c.cfg.lprs, splat)) splat(std::integral_constant<int, 4>{});
    }
    st = st_main;
    {
        const hipError_t e = fk.join(st);                     // the reduction below needs every class's sums
        if (e != hipSuccess) return phl_hip_fail(e, "joining the side stream of the chunk classes", __FILE__, __LINE__);
    }
    if (tl.get()) {                                           // debug only
        std::vector<unsigned long long> h(tl_n);
        PHL_HIP(hipMemcpyAsync(h.data(), tl.get(), tl_n * 8, hipMemcpyDeviceToHost, st));
        PHL_HIP(hipStreamSynchronize(st));
        PHL_TRY(tl.drop());
        if (FILE *f = fopen(tl_path, "wb")) {
            fwrite(h.data(), 8, tl_n, f);
            fclose(f);
        }
    }
    if (rc) return rc;
    if (M == 0) return PHL_OK;
    const int lpr = pick_lpr_row((int)out_rs);
    int64_t waves = ((int64_t)M + (64 / lpr) - 1) / (64 / lpr);
    int64_t blocks = (waves + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    // long slot lists: the lattice's own list of such vertices, or (subset) the caller's rows, short ones exiting
    // (a subset call walks its own rows only if the lattice has long vertices at all: one workgroup per listed row is
    //  tens of thousands of empty workgroups on the row-band path otherwise)
    // (with a send buffer to fill, the long kernel walks the caller's rows even when ... see above: n_long == 0 means no
    //  listed row can be long, so nothing is lost by skipping it)
    const int *llist = o.subset ? o.vlist : lat->vlong;
    const int64_t nl = lat->n_long == 0 ? 0 : (o.subset ? o.nvl : lat->n_long);
    const int long_list = llist ? LONG_LIST : 0x7FFFFFFF;
    auto reduce = [&](auto W) {
        constexpr int LPR = decltype(W)::value;
        k_splat_reduce<LPR><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(partial, lat->vs_ptr, lat->vs, lat->slot_pidx, M,
                                                                          (int)out_rs, vert, o.vlist, long_list, o.pack_pos, o.pack,
                                                                          o.pack_rs);
        if (llist && nl > 0)
            k_splat_reduce_long<LPR><<<dim3((unsigned)nl), dim3(256), 0, st>>>(partial, lat->vs_ptr, lat->vs, lat->slot_pidx,
                                                                               (int)out_rs, vert, llist, long_list,
                                                                               o.subset ? o.pack_pos : nullptr, o.pack, o.pack_rs);
    };
    if (!dispatch_int<64, 16, 4>(lpr, reduce)) reduce(std::integral_constant<int, 1>{});
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

int phl_launch_slice_tiled(const phl_lattice *lat, const float *vert, int vd, float *out, int64_t out_rs, const float *sub,
                           int64_t sub_rs, unsigned flags, hipStream_t st)
{
    if (lat->n == 0 || vd == 0) return PHL_OK;
    const slice_cfg cfg = plan_slice(lat, vd);
    const float cdiv = 1 + powf(2, -lat->d);  // permutohedral.h:480
    const float rcdiv = 1.0f / cdiv;
    const bool exact = (flags & PHL_FILTER_EXACT) != 0;
    int rc = PHL_OK;
    int xcd_chunk;
    unsigned cgrid = phl_xcd_grid(lat->nchunks, &xcd_chunk);
    // heavy chunks = those that cannot take at least half the widest slab; worth a head start only if they are few
    int heavy_thr = 0x7FFFFFFF, heavy_n = 0;
    if (lat->nv_cum && lat->chunk_by_nv && cfg.lsh_max > 2) {
        const int64_t fixed0 = (int64_t)lat->P * (lat->d + 1) * 8 + (int64_t)lat->P * 4 + 16;
        const int thr = (int)(((int64_t)cfg.lds - fixed0) / ((16 << (cfg.lsh_max - 1)) + 4));
        const int above = chunks_above(lat, thr);
        if (above > 0 && (int64_t)above * 16 <= lat->nchunks) { heavy_thr = thr; heavy_n = above; }
    }
    const int heavy_pad = (heavy_n + 7) & ~7;
    cgrid += (unsigned)heavy_pad;
    dispatch_bool(exact, [&](auto X) {
        constexpr bool EXACT = decltype(X)::value;
        if ((rc = allow_lds(k_slice_tiled<EXACT>, cfg.lds)) != PHL_OK) return;
        k_slice_tiled<EXACT><<<dim3(cgrid), dim3(TPB), cfg.lds, st>>>(
            vert, vd, (int)lat->n, lat->P, lat->d + 1, cfg.lsh_max, (int)cfg.lds, lat->pix_order, lat->chunk_vptr, lat->slot_vert,
            lat->lidx, lat->replay, out, out_rs, sub, sub_rs, cdiv, rcdiv, lat->nchunks, xcd_chunk, lat->chunk_by_nv, heavy_n,
            heavy_pad, heavy_thr);
    });
    if (rc) return rc;
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

// phl_filter_grad's last stage for the feature group [k0, k0 + ncols) (see k_slice_grad_group): the wide rows hold
// ncols + 1 <= 8 blocks, a pixel has d + 1 <= 17 vertices.  LDS is sized from the blocks, and never below the index data.
static int launch_slice_grad_group(const phl_lattice *lat, const float *vertw, int L, const float *y, int64_t y_rs, const float *ref,
                                   int64_t ref_rs, int64_t ref_cs, float *grad_ref, int k0, int ncols, int accumulate, float *wx_out,
                                   int64_t wx_rs, hipStream_t st)
{
    const int dp1 = lat->d + 1, nb = ncols + 1;
    const int64_t fixed = (((int64_t)lat->P * dp1 * 8 + (int64_t)lat->P * 4 + (int64_t)lat->nv_max * 4 + 15) & ~(int64_t)15);
    if (nb < 2 || nb > 8 || k0 < 0 || k0 + ncols > lat->d || dp1 > PHL_FILTER_GRAD_MAX_D + 1 || lat->P > 256 || lat->nchunks == 0 ||
        fixed > lds_big()) {
        phl_set_error("fused feature gradient: features [%d, %d) of d = %d not supported (groups of 1..7, d <= %d)", k0, k0 + ncols,
                      lat->d, PHL_FILTER_GRAD_MAX_D);
        return PHL_ERR_UNSUPPORTED;
    }
    int64_t lds = fixed + (int64_t)lat->nv_max * nb * 128;      // every chunk on 32-channel slabs, if the budget allows
    if (lds > lds_budget()) lds = lds_budget() > fixed ? lds_budget() : fixed;      // (fixed alone: every chunk DIRECT)
    const float rcdiv = 1.0f / (1 + powf(2, -lat->d));      // permutohedral.h:480
    int xcd_chunk;
    const unsigned cgrid = phl_xcd_grid(lat->nchunks, &xcd_chunk);
    int rc = PHL_OK;
    dispatch_int<2, 3, 4, 5, 6, 7, 8>(nb, [&](auto N) {          // (nb outside 2..8 was rejected above)
        constexpr int NB = decltype(N)::value;
        if ((rc = allow_lds(k_slice_grad_group<NB>, (size_t)lds)) != PHL_OK) return;
        k_slice_grad_group<NB><<<dim3(cgrid), dim3(TPB), (size_t)lds, st>>>(
            vertw, L, (int)lat->n, lat->P, dp1, k0, (int)lds, lat->pix_order, lat->chunk_vptr, lat->slot_vert, lat->lidx, lat->replay, y,
            y_rs, ref, ref_rs, ref_cs, grad_ref, accumulate, wx_out, wx_rs, rcdiv, lat->nchunks, xcd_chunk);
    });
    if (rc) return rc;
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}

// phl_filter_grad's last stage (see k_slice_grad): columns [k0, k0 + ncols) of grad_ref from wide rows of ncols + 1
// blocks.  All d <= 7 columns at once: k_slice_grad<d + 1>; a feature group: k_slice_grad_group.  P <= 256 (eight
// pixels per 16-lane group).
int phl_launch_slice_grad(const phl_lattice *lat, const float *vertw, int L, const float *y, int64_t y_rs, const float *ref,
                          int64_t ref_rs, int64_t ref_cs, float *grad_ref, int k0, int ncols, int accumulate, float *wx_out,
                          int64_t wx_rs, hipStream_t st)
{
    if (lat->n == 0 || L == 0) return PHL_OK;
    if (k0 != 0 || ncols != lat->d)
        return launch_slice_grad_group(lat, vertw, L, y, y_rs, ref, ref_rs, ref_cs, grad_ref, k0, ncols, accumulate, wx_out, wx_rs, st);
    const int dp1 = lat->d + 1;
    if (dp1 < 2 || dp1 > 8 || lat->P > 256 || lat->nchunks == 0) {
        phl_set_error("fused feature gradient: d = %d not supported in one group (1..7)", lat->d);
        return PHL_ERR_UNSUPPORTED;
    }
    const int64_t fixed = (((int64_t)lat->P * dp1 * 8 + (int64_t)lat->P * 4 + (int64_t)lat->nv_max * 4 + 15) & ~(int64_t)15);
    int64_t lds = fixed + (int64_t)lat->nv_max * dp1 * 128;      // every chunk on 32-channel slabs, if the budget allows
    if (lds > lds_budget()) lds = lds_budget();
    const float rcdiv = 1.0f / (1 + powf(2, -lat->d));      // permutohedral.h:480
    int xcd_chunk;
    const unsigned cgrid = phl_xcd_grid(lat->nchunks, &xcd_chunk);
    int rc = PHL_OK;
    dispatch_int<2, 3, 4, 5, 6, 7, 8>(dp1, [&](auto N) {          // (dp1 outside 2..8 was rejected above)
        constexpr int NS = decltype(N)::value;
        if ((rc = allow_lds(k_slice_grad<NS>, (size_t)lds)) != PHL_OK) return;
        k_slice_grad<NS><<<dim3(cgrid), dim3(TPB), (size_t)lds, st>>>(
            vertw, L, (int)lat->n, lat->P, (int)lds, lat->pix_order, lat->chunk_vptr, lat->slot_vert, lat->lidx, lat->replay, y, y_rs,
            ref, ref_rs, ref_cs, grad_ref, accumulate, wx_out, wx_rs, rcdiv, lat->nchunks, xcd_chunk);
    });
    if (rc) return rc;
    PHL_HIP(hipGetLastError());
    return PHL_OK;
}
