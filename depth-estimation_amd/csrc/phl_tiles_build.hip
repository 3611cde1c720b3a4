// phl_tiles_build.hip -- the chunk build: everything the LDS-staged splat / slice kernels of phl_tiles.hip read, made
// once per lattice (pixel order, locality numbering of the vertices, per-chunk local vertex lists and segments,
// vertex -> slots lists).
//
// Chunks need no image geometry: pixels are ordered by the cell of a uniform 2-D grid laid over
// the two feature dimensions with the widest range (for an image: x/sigma, y/sigma ->
// sqrt(P) x sqrt(P) pixel tiles), then cut into runs of P.  Any other data still works, only
// with less sharing; the host falls back to the gather kernels when sharing is poor.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "phl_device_utils.h"

namespace {

// ---- feature ranges --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_minmax(const float *__restrict__ ref, int64_t rs, int64_t cs, int64_t n, int d,
                                                float *__restrict__ out /* [grid][d][2] */)
{
    // one pass over the pixels, all d features of a pixel by the same thread (pixel-major features: every cache line is
    // touched once, not d times)
    __shared__ float smin[4][PHL_MAX_D], smax[4][PHL_MAX_D];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float lo[PHL_MAX_D], hi[PHL_MAX_D];
#pragma unroll
    for (int i = 0; i < PHL_MAX_D; i++) { lo[i] = INFINITY; hi[i] = -INFINITY; }
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int i = 0; i < PHL_MAX_D; i++)
            if (i < d) {
                const float v = ref[p * rs + i * cs];
                lo[i] = fminf(lo[i], v);
                hi[i] = fmaxf(hi[i], v);
            }
    }
#pragma unroll
    for (int i = 0; i < PHL_MAX_D; i++)
        if (i < d) {
            float a = lo[i], b = hi[i];
            for (int o = 32; o > 0; o >>= 1) {
                a = fminf(a, __shfl_xor(a, o));
                b = fmaxf(b, __shfl_xor(b, o));
            }
            if (lane == 0) { smin[w][i] = a; smax[w][i] = b; }
        }
    __syncthreads();
    if ((int)threadIdx.x < d) {
        float a = smin[0][threadIdx.x], b = smax[0][threadIdx.x];
        for (int k = 1; k < 4; k++) { a = fminf(a, smin[k][threadIdx.x]); b = fmaxf(b, smax[k][threadIdx.x]); }
        out[((int64_t)blockIdx.x * d + threadIdx.x) * 2 + 0] = a;
        out[((int64_t)blockIdx.x * d + threadIdx.x) * 2 + 1] = b;
    }
}

__global__ __launch_bounds__(256) void k_cell_ids(const float *__restrict__ ref, int64_t rs, int64_t cs, int64_t n, int da,
                                                  int db, float lo_a, float lo_b, float inv_t, int nca, int ncb,
                                                  int *__restrict__ cell)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < n;
    const int64_t pc = active ? p : n - 1;
    int ca = (int)((ref[pc * rs + da * cs] - lo_a) * inv_t);
    ca = min(max(ca, 0), nca - 1);
    int cb = 0;
    if (db >= 0) {
        cb = (int)((ref[pc * rs + db * cs] - lo_b) * inv_t);
        cb = min(max(cb, 0), ncb - 1);
    }
    const int c = cb * nca + ca;   // the wider dimension runs fastest inside a row of cells
    if (active) cell[p] = c;
}

// ---- locality renumbering of the vertices ----------------------------------------------------------------
// First-touch ids follow the pixel order: for an image, raster order, so a vertex and the blur neighbours a few
// pixels above / below it are a few image ROWS apart in every [M][vd] array (2 MB at 2048 pixels per row) and
// the 9-row stencil of a blur pass outruns the 4 MiB L2 of an XCD (58 % hits).  Internally the vertices are
// therefore numbered strip by strip: the grid of the two widest feature dimensions is cut into 8 strips along
// the wider one, a vertex's home cell is the cell of its first-touch pixel, and vertices are
// ordered by (strip, cell row, cell inside the strip), first-touch order inside a cell (stable sort).  A blur
// launch gives every XCD a contiguous eighth of the ids = about one strip, walked row by row, so that both the
// own-row stream and the stencil stay local.  Public introspection keeps the reference's first-touch numbering
// (phl_get_keys & co translate); rows of caller-visible vertex buffers are in internal order
// (phl_get_vertex_order).
__global__ __launch_bounds__(256) void k_vertex_home(const phl_replay_t *__restrict__ replay, int N, int dp1,
                                                     const int *__restrict__ cell, int *vhome)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int v = replay[e].vid, c = cell[e / dp1];
    // the value only ever decreases, so a stale read can at worst cause a redundant atomic; in pixel order the
    // first toucher usually already holds the minimum and most candidates skip the atomic
    if (c < *reinterpret_cast<volatile int *>(&vhome[v])) atomicMin(&vhome[v], c);
}

// home cell from the first-touch candidate (the common case: one thread per vertex, no atomics)
__global__ __launch_bounds__(256) void k_vertex_home_first(const int *__restrict__ vfirst, int M, int dp1,
                                                           const int *__restrict__ cell, int *__restrict__ vhome)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < M) vhome[v] = cell[vfirst[v] / dp1];
}

__global__ __launch_bounds__(256) void k_strip_key(const int *__restrict__ vhome, int M, int nca, int ncb, int stripw,
                                                   int *__restrict__ key)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= M) return;
    const int c = vhome[v];
    const int ca = c % nca, cb = c / nca;
    key[v] = ((ca / stripw) * ncb + cb) * stripw + ca % stripw;
}

__global__ __launch_bounds__(256) void k_iota_tail(int *__restrict__ p, int first, int end)
{
    const int i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < end) p[i] = i;
}

__global__ __launch_bounds__(256) void k_invert_perm(const int *__restrict__ perm, int M, int *__restrict__ inv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) inv[perm[i]] = i;
}

__global__ __launch_bounds__(256) void k_permute_keys(const int16_t *__restrict__ in, const int *__restrict__ ft_of_int, int M,
                                                      int d, int16_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * d) return;
    const int v = (int)(i / d), c = (int)(i - (int64_t)v * d);
    out[i] = in[(int64_t)ft_of_int[v] * d + c];
}

__global__ __launch_bounds__(256) void k_relabel_replay(phl_replay_t *__restrict__ replay, int N, const int *__restrict__ int_of_ft)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < N) replay[e].vid = int_of_ft[replay[e].vid];
}

// ---- per-chunk structure: one workgroup groups the chunk's entries by vertex in LDS ----------------
// entry e = k*(d+1)+r of the chunk (k-th pixel in chunk order, remainder r).  Wanted: the entries grouped by vertex
// with ascending e inside a group, i.e. ascending pixel: exactly the per-vertex segment the splat needs.
//   1. the chunk's distinct vertices get dense ids 0..nv-1 through an LDS hash table (slot order);
//   2. a STABLE least-significant-digit radix sort of the entries by dense id, four bits a pass -- ceil(log2 nv)/4
//      passes: two for the ~50-250 local vertices of an image chunk, where a comparison sort of (vertex, entry) keys
//      took 66 compare-exchange stages.  A thread owns PER consecutive entries; its digit histogram is a packed
//      64-bit register (sixteen 4-bit counts), the workgroup-wide prefix per (digit, thread) a wavefront scan on DPP
//      row shifts over four words of four 16-bit fields.
// WRITE=false only counts the distinct vertices.
#define PHL_DPP_ADD(x, ctrl, rowmask) x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)(x), ctrl, rowmask, 0xF, false)
__device__ __forceinline__ unsigned wave_inclusive_scan_u32(unsigned x)
{
    PHL_DPP_ADD(x, 0x111, 0xF);     // row_shr:1
    PHL_DPP_ADD(x, 0x112, 0xF);     // row_shr:2
    PHL_DPP_ADD(x, 0x114, 0xF);     // row_shr:4
    PHL_DPP_ADD(x, 0x118, 0xF);     // row_shr:8
    PHL_DPP_ADD(x, 0x142, 0xA);     // row_bcast:15 into rows 1 and 3
    PHL_DPP_ADD(x, 0x143, 0xC);     // row_bcast:31 into rows 2 and 3
    return x;
}
#undef PHL_DPP_ADD

template <int SORTN, bool WRITE>
__global__ __launch_bounds__(256) void k_chunk_group(const int *__restrict__ pix_order, int n, int P, int dp1,
                                                     const phl_replay_t *__restrict__ replay, int *__restrict__ nv_out,
                                                     const int *__restrict__ vptr, int stride, int *__restrict__ slot_vert,
                                                     int2 *__restrict__ seg_rng, phl_contrib_t *__restrict__ seg,
                                                     unsigned short *__restrict__ lidx, const int *__restrict__ nv_known,
                                                     int skip_le)
{
    // nv_known: the chunks' vertex counts from k_chunk_masks -- chunks with at most skip_le are done already
    if (nv_known && nv_known[blockIdx.x] <= skip_le) return;
    // vptr != null: slots go to their final place vptr[c] + local index.  vptr == null (first and
    // normally only pass): slots go to a scratch area with a fixed `stride` per chunk (local indices
    // beyond it are dropped -- the host then repeats the pass with the real offsets), and the number of
    // local vertices is reported in nv_out.
    constexpr int PER = SORTN / 256;       // consecutive entries owned by a thread
    constexpr int HT = 2 * SORTN;          // hash slots (load <= 1/2)
    constexpr int HB = SORTN == 2048 ? 12 : (SORTN == 1024 ? 11 : 10);
    static_assert(PER <= 8, "the per-thread digit histogram has 4-bit counts");
    __shared__ unsigned keys[SORTN];       // (dense id << 11) | entry
    __shared__ int tab[HT + 8];            // slot -> vertex id, then slot -> dense id; later hpos | newidx (shorts)
    __shared__ int lvid[SORTN];            // dense id -> vertex id
    __shared__ unsigned wtot[4][8];
    __shared__ int lbin[258];              // histogram over segment lengths 1..P (P <= 256)
    const int c = blockIdx.x;
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int i0 = threadIdx.x * PER;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < HT; j += 256) tab[j] = -1;
    int vid[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = i0 + u;
        vid[u] = -1;
        if (e < E) {
            const int k = e / dp1, rr = e - k * dp1;
            const int p = pix_order[base + k];
            vid[u] = replay[(int64_t)p * dp1 + rr].vid;
        }
    }
    __syncthreads();
    int slot[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        slot[u] = 0;
        if (vid[u] >= 0) {
            unsigned h = ((unsigned)vid[u] * 2654435761u) >> (32 - HB);
            for (;;) {
                const int prev = atomicCAS(&tab[h], -1, vid[u]);
                if (prev == -1 || prev == vid[u]) break;
                h = (h + 1) & (HT - 1);
            }
            slot[u] = (int)h;
        }
    }
    __syncthreads();
    int nv;
    {
        constexpr int SPT = HT / 256;      // slots owned by a thread
        int occ = 0;
#pragma unroll
        for (int j = 0; j < SPT; j++) occ += tab[threadIdx.x * SPT + j] >= 0 ? 1 : 0;
        int id = block_exclusive_scan(occ, &nv);
#pragma unroll
        for (int j = 0; j < SPT; j++) {
            const int sidx = threadIdx.x * SPT + j;
            const int v = tab[sidx];
            if (v >= 0) {
                lvid[id] = v;
                tab[sidx] = id++;
            }
        }
    }
    __syncthreads();
    if (nv_out && threadIdx.x == 0) nv_out[c] = nv;
    if (!WRITE) return;
    unsigned r[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) r[u] = vid[u] >= 0 ? (((unsigned)tab[slot[u]] << 11) | (unsigned)(i0 + u)) : ~0u;
    const int bits = nv > 1 ? 32 - __clz(nv - 1) : 0;
    for (int sh = 11; sh < 11 + bits; sh += 4) {
        // digit histogram of the thread's entries (4-bit counts) and every entry's rank among the thread's equal digits
        unsigned long long hist = 0;
        int lr[PER], dg[PER];
#pragma unroll
        for (int u = 0; u < PER; u++) {
            dg[u] = (int)((r[u] >> sh) & 15u);
            lr[u] = (int)((hist >> (4 * dg[u])) & 15ull);
            if (r[u] != ~0u) hist += 1ull << (4 * dg[u]);
        }
        // eight words of two 16-bit counts (digits 2j, 2j+1); inclusive scan over the workgroup's threads
        unsigned own[8], inc[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned x = (unsigned)(hist >> (8 * j)) & 0xFFu;
            own[j] = (x & 15u) | ((x >> 4) << 16);
            inc[j] = wave_inclusive_scan_u32(own[j]);
        }
        if (lane == 63)                                   // (the previous pass's reads of wtot lie behind its last barrier)
#pragma unroll
            for (int j = 0; j < 8; j++) wtot[wv][j] = inc[j];
        __syncthreads();
        unsigned pos[8];
        unsigned run = 0;                                 // exclusive scan over the digits (counts < 2^16)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            unsigned before = 0, tot = 0;
#pragma unroll
            for (int w2 = 0; w2 < 4; w2++) {
                const unsigned t = wtot[w2][j];
                tot += t;
                if (w2 < wv) before += t;
            }
            const unsigned lo = run, hi = run + (tot & 0xFFFFu);
            run = hi + (tot >> 16);
            pos[j] = (inc[j] - own[j]) + before + (lo | (hi << 16));
        }
#pragma unroll
        for (int u = 0; u < PER; u++) {
            if (r[u] == ~0u) continue;
            unsigned q = pos[0];
#pragma unroll
            for (int j = 1; j < 8; j++) q = (dg[u] >> 1) == j ? pos[j] : q;
            const int rank = (int)((q >> (16 * (dg[u] & 1))) & 0xFFFFu) + lr[u];
            keys[rank] = r[u];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; u++) r[u] = (i0 + u) < E ? keys[i0 + u] : ~0u;
    }
    if (bits == 0) {
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (i0 + u < E) keys[i0 + u] = r[u];
    }
    __syncthreads();                                      // (tab is dead from here: hpos | newidx take its place)
    // Local vertices are renumbered by DESCENDING segment length (counting sort in LDS): the
    // splat kernel hands neighbouring local vertices to the lane groups of one wavefront, which
    // then run loops of nearly equal length, and takes groups longest-first.
    unsigned short *hpos = reinterpret_cast<unsigned short *>(tab);   // [nv + 1] start of the segment of dense id j
    unsigned short *newidx = hpos + SORTN + 2;                         // [nv] dense id -> length-order index
    const int total = nv;
    const int64_t vbase = vptr ? (int64_t)vptr[c] : (int64_t)c * stride;
    const int vcap = vptr ? SORTN : stride;
    const int64_t ebase = (int64_t)base * dp1;
    for (int j = threadIdx.x; j < 258; j += 256) lbin[j] = 0;
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int i = i0 + u;
        if (i < E && (i == 0 || (keys[i] >> 11) != (keys[i - 1] >> 11))) hpos[keys[i] >> 11] = (unsigned short)i;
    }
    if (threadIdx.x == 0) hpos[total] = (unsigned short)E;
    __syncthreads();
    for (int j = threadIdx.x; j < total; j += 256) atomicAdd(&lbin[256 - min(hpos[j + 1] - hpos[j], 256)], 1);   // bin 0 = longest
    __syncthreads();
    if (threadIdx.x < 64) {           // exclusive scan of the 257 bins by one wavefront
        int carry = 0;
        for (int b0 = 0; b0 < 257; b0 += 64) {
            const int b = b0 + (int)threadIdx.x;
            const int x = b < 257 ? lbin[b] : 0;
            int incl = x;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if ((int)threadIdx.x >= o) incl += y;
            }
            if (b < 257) lbin[b] = carry + incl - x;
            carry += __shfl(incl, 63);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < total; j += 256)
        newidx[j] = (unsigned short)atomicAdd(&lbin[256 - min(hpos[j + 1] - hpos[j], 256)], 1);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int i = i0 + u;
        if (i >= E) break;
        const int li = (int)(keys[i] >> 11);
        const int e = (int)(keys[i] & 2047u);
        const bool head = (i == 0) || li != (int)(keys[i - 1] >> 11);
        const int k = e / dp1, rr = e - k * dp1;
        const int p = pix_order[base + k];
        if (head && newidx[li] < vcap) {
            const int64_t sl = vbase + newidx[li];
            slot_vert[sl] = lvid[li];
            seg_rng[sl] = make_int2((int)(ebase + i), (int)(ebase + hpos[li + 1]));
        }
        phl_contrib_t sg;
        sg.pixel = k;
        sg.w = replay[(int64_t)p * dp1 + rr].w;
        seg[ebase + i] = sg;
        lidx[ebase + e] = (unsigned short)newidx[li];
    }
}

// The same grouping without a sort, for chunks with at most NVC distinct vertices (every chunk of an image): a pixel
// holds a vertex at most once (the d+1 vertices of a simplex are distinct), so a local vertex's segment is a SET of chunk
// pixels -- one bit per pixel, eight words per vertex (P <= 256), set with one LDS atomic per entry.  An entry's place in
// its segment is the number of set bits below its pixel (a per-word prefix per vertex + one popcount), the segment's
// start the scan of the segment lengths.  ~400 vector instructions a wavefront where the radix passes of k_chunk_group
// take ~1,700 (the kernel is bound by instruction issue).  A chunk with more vertices only reports its count; the host
// then runs k_chunk_group on those chunks.
constexpr int NVC = 256;               // (the kernel waits on LDS / L2 round trips: a small footprint buys workgroups per CU)

template <int SORTN, int HTX>
__global__ __launch_bounds__(256) void k_chunk_masks(const int *__restrict__ pix_order, int n, int P, int dp1,
                                                     const phl_replay_t *__restrict__ replay, int *__restrict__ nv_out,
                                                     const int *__restrict__ vptr, int stride, int *__restrict__ slot_vert,
                                                     int2 *__restrict__ seg_rng, phl_contrib_t *__restrict__ seg,
                                                     unsigned short *__restrict__ lidx)
{
    constexpr int PER = SORTN / 256;       // consecutive entries owned by a thread
    constexpr int HT = HTX * SORTN;        // hash slots: load <= 3/4 (the host picks HTX = 2 where P(d+1) > 3/4 SORTN)
    constexpr int HB = (SORTN == 2048 ? 11 : (SORTN == 1024 ? 10 : 9)) + (HTX == 2 ? 1 : 0);
    constexpr int TABN = (HT > NVC * 8 ? HT : NVC * 8) + 8;
    __shared__ __attribute__((aligned(16))) int tab[TABN];   // slot -> vertex id, then slot -> dense id; then the pixel masks [nv][8]
    __shared__ int lvid[NVC];              // dense id -> vertex id
    __shared__ __attribute__((aligned(8))) unsigned char cum[NVC][8];   // set bits of a vertex's mask below word w (<= 224)
    __shared__ unsigned short startv[NVC + 2];   // segment start of dense id j (entries), [nv] = E
    __shared__ unsigned short newidx[NVC]; // dense id -> length-order index
    __shared__ int lbin[258];              // histogram over segment lengths 1..P (P <= 256)
    const int c = blockIdx.x;
    const int base = c * P;
    const int cnt = min(P, n - base);
    const int E = cnt * dp1;
    const int i0 = threadIdx.x * PER;
    for (int j = threadIdx.x; j < HT; j += 256) tab[j] = -1;
    int vid[PER], kk[PER], rrr[PER];
    float wgt[PER];
    {
        int k = i0 / dp1, rr = i0 - k * dp1;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            vid[u] = -1;
            wgt[u] = 0.f;
            kk[u] = k;
            rrr[u] = rr;
            if (i0 + u < E) {
                const int p = pix_order[base + k];
                const phl_replay_t rp = replay[(int64_t)p * dp1 + rr];
                vid[u] = rp.vid;
                wgt[u] = rp.w;
            }
            if (++rr == dp1) { rr = 0; k++; }
        }
    }
    __syncthreads();
    int slot[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        slot[u] = 0;
        if (vid[u] >= 0) {
            unsigned h = ((unsigned)vid[u] * 2654435761u) >> (32 - HB);
            for (;;) {
                const int prev = atomicCAS(&tab[h], -1, vid[u]);
                if (prev == -1 || prev == vid[u]) break;
                h = (h + 1) & (HT - 1);
            }
            slot[u] = (int)h;
        }
    }
    __syncthreads();
    int nv;
    {
        constexpr int SPT = HT / 256;      // slots owned by a thread
        int occ = 0;
#pragma unroll
        for (int j = 0; j < SPT; j++) occ += tab[threadIdx.x * SPT + j] >= 0 ? 1 : 0;
        int id = block_exclusive_scan(occ, &nv);
#pragma unroll
        for (int j = 0; j < SPT; j++) {
            const int sidx = threadIdx.x * SPT + j;
            const int v = tab[sidx];
            if (v >= 0) {
                if (id < NVC) lvid[id] = v;
                tab[sidx] = id++;
            }
        }
    }
    __syncthreads();
    if (nv_out && threadIdx.x == 0) nv_out[c] = nv;
    if (nv > NVC) return;                  // (workgroup-uniform) left to k_chunk_group
    int id[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) id[u] = vid[u] >= 0 ? tab[slot[u]] : 0;
    __syncthreads();                       // tab is dead: the masks take its place
    unsigned *mask = reinterpret_cast<unsigned *>(tab);
    for (int j = threadIdx.x; j < nv * 8; j += 256) mask[j] = 0u;
    for (int j = threadIdx.x; j < 258; j += 256) lbin[j] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; u++)
        if (vid[u] >= 0) atomicOr(&mask[id[u] * 8 + (kk[u] >> 5)], 1u << (kk[u] & 31));
    __syncthreads();
    // per vertex (thread v): prefix of set bits per word, segment length
    int len = 0;
    if ((int)threadIdx.x < nv) {
        const int v = threadIdx.x;
        const uint4 m0 = *reinterpret_cast<const uint4 *>(mask + v * 8), m1 = *reinterpret_cast<const uint4 *>(mask + v * 8 + 4);
        const unsigned mw[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
        unsigned c4[2] = {0u, 0u};
#pragma unroll
        for (int w = 0; w < 8; w++) {
            c4[w >> 2] |= (unsigned)len << (8 * (w & 3));
            len += __popc(mw[w]);
        }
        *reinterpret_cast<uint2 *>(&cum[v][0]) = make_uint2(c4[0], c4[1]);
        atomicAdd(&lbin[256 - min(len, 256)], 1);          // bin 0 = longest
    }
    {
        int tot;
        const int ex = block_exclusive_scan(len, &tot);
        if ((int)threadIdx.x < nv) startv[threadIdx.x] = (unsigned short)ex;
        if (threadIdx.x == 0) startv[nv] = (unsigned short)E;
    }
    __syncthreads();
    // Local vertices are renumbered by DESCENDING segment length (counting sort in LDS): the
    // splat kernel hands neighbouring local vertices to the lane groups of one wavefront, which
    // then run loops of nearly equal length, and takes groups longest-first.
    if (threadIdx.x < 64) {           // exclusive scan of the 257 bins by one wavefront
        int carry = 0;
        for (int b0 = 0; b0 < 257; b0 += 64) {
            const int b = b0 + (int)threadIdx.x;
            const int x = b < 257 ? lbin[b] : 0;
            int incl = x;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if ((int)threadIdx.x >= o) incl += y;
            }
            if (b < 257) lbin[b] = carry + incl - x;
            carry += __shfl(incl, 63);
        }
    }
    __syncthreads();
    const int64_t vbase = vptr ? (int64_t)vptr[c] : (int64_t)c * stride;
    const int vcap = vptr ? SORTN : stride;
    const int64_t ebase = (int64_t)base * dp1;
    if ((int)threadIdx.x < nv) {
        const int v = threadIdx.x;
        const int ni = atomicAdd(&lbin[256 - min(len, 256)], 1);
        newidx[v] = (unsigned short)ni;
        if (ni < vcap) {
            const int64_t sl = vbase + ni;
            slot_vert[sl] = lvid[v];
            seg_rng[sl] = make_int2((int)(ebase + startv[v]), (int)(ebase + startv[v] + len));
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; u++) {
        if (vid[u] < 0) continue;
        const int v = id[u], k = kk[u];
        const int pos = (int)startv[v] + (int)cum[v][k >> 5] + __popc(mask[v * 8 + (k >> 5)] & ((1u << (k & 31)) - 1u));
        phl_contrib_t sg;
        sg.pixel = k;
        sg.w = wgt[u];
        seg[ebase + pos] = sg;
        lidx[ebase + i0 + u] = newidx[v];
    }
}

// scratch slot records [chunk][stride] -> compact [vptr[chunk] + i]
__global__ __launch_bounds__(256) void k_compact_slots(const int *__restrict__ vptr, int nchunks, int stride,
                                                       const int *__restrict__ t_vert, const int2 *__restrict__ t_rng,
                                                       int *__restrict__ slot_vert, int2 *__restrict__ seg_rng)
{
    const int c = blockIdx.x;
    const int b = vptr[c], nv = vptr[c + 1] - b;
    for (int i = threadIdx.x; i < nv; i += 256) {
        slot_vert[b + i] = t_vert[(int64_t)c * stride + i];
        seg_rng[b + i] = t_rng[(int64_t)c * stride + i];
    }
}

__global__ __launch_bounds__(256) void k_count_slots(const int *__restrict__ slot_vert, int S, int *cnt)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) atomicAdd(&cnt[slot_vert[s]], 1);
}

// the vertex -> slots list entries from the sort's permutation, and the slots' marks: bit 31 of slot_vert = this chunk is
// the vertex's only contributor (sole); the others are flagged for the partial buffer
__global__ __launch_bounds__(256) void k_contrib_and_sole(const int *__restrict__ perm, int *__restrict__ slot_vert, int S,
                                                          const int *__restrict__ vs_ptr, phl_contrib_t *__restrict__ vs,
                                                          int *__restrict__ multi)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    phl_contrib_t c;
    c.pixel = perm[s];
    c.w = 0.f;
    vs[s] = c;
    const int v = slot_vert[s];
    const bool sole = (vs_ptr[v + 1] - vs_ptr[v]) == 1;
    if (sole) slot_vert[s] = v | (int)0x80000000;
    multi[s] = sole ? 0 : 1;
}

// vertices fed by more than `long_list` chunks, appended in any order (k_splat_reduce_long gives each its own
// workgroup; the order only decides which starts first -- lists of more than 64 are sorted by length afterwards)
__global__ __launch_bounds__(256) void k_append_long(const int *__restrict__ vs_ptr, int M, int long_list, int *__restrict__ vlong,
                                                     int *__restrict__ count)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < M && vs_ptr[v + 1] - vs_ptr[v] > long_list) vlong[atomicAdd(count, 1)] = v;
}

// vs[e].w <- partial-buffer row of the slot (bit pattern of an int): saves the reduce kernels one dependent load
__global__ __launch_bounds__(256) void k_fill_vs_rows(phl_contrib_t *__restrict__ vs, int S, const int *__restrict__ slot_pidx)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < S) vs[e].w = __int_as_float(slot_pidx[vs[e].pixel]);
}

// sort key of a long vertex: lists in descending length
__global__ __launch_bounds__(256) void k_long_keys(const int *__restrict__ vlong, int n, const int *__restrict__ vs_ptr, int kmax,
                                                   int *__restrict__ key)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = kmax - min(vs_ptr[vlong[i] + 1] - vs_ptr[vlong[i]], kmax);
}

__global__ __launch_bounds__(256) void k_gather_i32(const int *__restrict__ src, const int *__restrict__ perm, int n, int *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// vertex processing order for the gather splat: vertices sorted by the first chunk that touches
// them, so that vertices summed at the same time read the same few chunks' pixel rows (L2 hits
// instead of Infinity-Cache traffic).  first[s] = 1 iff slot s is the first slot of its vertex.
__global__ __launch_bounds__(256) void k_first_slot(const int *__restrict__ slot_vert, int S, const int *__restrict__ vs_ptr,
                                                    const phl_contrib_t *__restrict__ vs, int *__restrict__ first)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int v = slot_vert[s] & 0x7FFFFFFF;
    first[s] = (vs[vs_ptr[v]].pixel == s) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_fill_vorder(const int *__restrict__ slot_vert, int S, const int *__restrict__ first,
                                                     const int *__restrict__ rank, int M_local, int M,
                                                     int *__restrict__ vorder)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S && first[i]) vorder[rank[i]] = slot_vert[i] & 0x7FFFFFFF;
    if (i >= M_local && i < M) vorder[i] = i;      // ghost vertices (no local contributions) go last
}

__global__ __launch_bounds__(256) void k_strip_marks(int *slot_vert, int S)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) slot_vert[s] &= 0x7FFFFFFF;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// vertex -> slots lists (ascending slot = ascending chunk), sole marks and partial-row indices.
// Also called after ghost vertices were appended (M grew, the slots did not change).
// Vertex processing order of the gather splat (exact arithmetic, shapes the chunk kernels do not take): made on first
// use, under the same lock as the contribution lists (phl_ensure_csr).
int phl_tiles_ensure_vorder(phl_lattice *lat, hipStream_t st)
{
    if (lat->vorder || !lat->vs_ptr || !lat->vs || !lat->slot_vert) return PHL_OK;
    const int M = (int)lat->M, S = (int)lat->S;
    if (M == 0 || S == 0) return PHL_OK;
    phl_dev_block<int32_t> vorder(st);      // (the lattice's only once it is filled)
    temp_pool tmp(st);
    int *first, *frank, *tile_sums;
    PHL_HIP(tmp.get(&first, (size_t)S + 1));
    PHL_HIP(tmp.get(&frank, (size_t)S + 2));
    PHL_HIP(tmp.get(&tile_sums, (size_t)S / SCAN_TILE + 2));
    PHL_TRY(vorder.alloc((size_t)M + 1));
    const unsigned gS = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(k_first_slot, dim3(gS), dim3(256), 0, st, lat->slot_vert, S, lat->vs_ptr, lat->vs, first);
    PHL_HIP(hipGetLastError());
    PHL_TRY(exclusive_scan(first, frank, S, tile_sums, st));
    const int span = S > M ? S : M;
    hipLaunchKernelGGL(k_fill_vorder, dim3((span + 255) / 256), dim3(256), 0, st, lat->slot_vert, S, first, frank,
                       (int)lat->M_local, M, vorder.get());
    PHL_HIP(hipGetLastError());
    PHL_HIP(hipStreamSynchronize(st));      // temporaries go back to the scratch cache
    lat->vorder = vorder.release();
    return PHL_OK;
}

int phl_tiles_link_vertices(phl_lattice *lat, hipStream_t st)
{
    const int M = (int)lat->M, S = (int)lat->S;
    phl_pinned_reset();                       // (callers have synchronised the stream: nothing of the arena is in flight)
    lat->S_multi = 0;
    PHL_HIP(phl_lat_alloc(lat->vs_ptr, (size_t)M + 1));
    PHL_HIP(phl_lat_alloc(lat->vs, (size_t)S + 1));
    PHL_HIP(phl_lat_alloc(lat->slot_pidx, (size_t)S + 1));
    if (S == 0) {
        PHL_HIP(hipMemsetAsync(lat->vs_ptr, 0, sizeof(int) * ((size_t)M + 1), st));
        PHL_HIP(hipStreamSynchronize(st));
        return PHL_OK;
    }
    temp_pool tmp(st);
    int *cnt, *multi, *tile_sums, *sperm;
    PHL_HIP(tmp.get(&cnt, (size_t)M + 1));
    PHL_HIP(tmp.get(&multi, (size_t)S + 1));
    PHL_HIP(tmp.get(&tile_sums, (size_t)(S > M ? S : M) / SCAN_TILE + 2));
    PHL_HIP(tmp.get(&sperm, (size_t)S));
    PHL_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)M + 1), st));
    const unsigned gS = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(k_strip_marks, dim3(gS), dim3(256), 0, st, lat->slot_vert, S);
    hipLaunchKernelGGL(k_count_slots, dim3(gS), dim3(256), 0, st, lat->slot_vert, S, cnt);
    PHL_HIP(hipGetLastError());
    PHL_TRY(exclusive_scan(cnt, lat->vs_ptr, M, tile_sums, st));
    // slots grouped by vertex, ascending slot (= ascending chunk) inside a vertex: a stable sort by vertex id (the
    // marks are stripped: slot_vert itself is the key array)
    PHL_TRY(stable_sort_perm(lat->slot_vert, S, M, sperm, tmp, st));
    hipLaunchKernelGGL(k_contrib_and_sole, dim3(gS), dim3(256), 0, st, sperm, lat->slot_vert, S, lat->vs_ptr, lat->vs, multi);
    PHL_HIP(hipGetLastError());
    PHL_TRY(exclusive_scan(multi, lat->slot_pidx, S, tile_sums, st));
    hipLaunchKernelGGL(k_fill_vs_rows, dim3(gS), dim3(256), 0, st, lat->vs, S, lat->slot_pidx);
    PHL_HIP(hipGetLastError());
    int pageable_counts[2] = {0, 0};
    int *counts = (int *)phl_pinned_alloc(sizeof(int) * 2);          // {S_multi, n_long}
    if (!counts) counts = pageable_counts;
    PHL_HIP(hipMemcpyAsync(&counts[0], lat->slot_pidx + S, sizeof(int), hipMemcpyDeviceToHost, st));
    // vertices with long slot lists (k_splat_reduce_long)
    int n_long = 0;
    lat->n_long = 0;
    {
        int *lcount;
        PHL_HIP(tmp.get(&lcount, 1));
        PHL_HIP(hipMemsetAsync(lcount, 0, sizeof(int), st));
        PHL_HIP(phl_lat_alloc(lat->vlong, (size_t)M + 1));      // worst case; usually almost empty
        hipLaunchKernelGGL(k_append_long, dim3((M + 255) / 256), dim3(256), 0, st, lat->vs_ptr, M, LONG_LIST, lat->vlong, lcount);
        PHL_HIP(hipGetLastError());
        PHL_HIP(hipMemcpyAsync(&counts[1], lcount, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    // (the chunk-major vertex order of the gather splat is made on first use: phl_tiles_ensure_vorder)
    PHL_HIP(phl_lat_free(lat->vorder));
    PHL_HIP(hipStreamSynchronize(st));
    const int s_multi = counts[0];
    n_long = counts[1];
    lat->S_multi = s_multi;
    lat->n_long = n_long;
    if (n_long > 64) {
        // longest lists first: k_splat_reduce_long runs one workgroup per vertex, and a 600-row list that starts
        // last is the launch's tail
        int *lkey, *lperm, *lsorted;
        PHL_HIP(tmp.get(&lkey, (size_t)n_long));
        PHL_HIP(tmp.get(&lperm, (size_t)n_long));
        PHL_HIP(tmp.get(&lsorted, (size_t)n_long));
        const unsigned gl = (unsigned)((n_long + 255) / 256);
        const int kmax = lat->nchunks + 1;
        hipLaunchKernelGGL(k_long_keys, dim3(gl), dim3(256), 0, st, lat->vlong, n_long, lat->vs_ptr, kmax, lkey);
        PHL_HIP(hipGetLastError());
        PHL_TRY(stable_sort_perm(lkey, n_long, (int64_t)kmax + 1, lperm, tmp, st));
        hipLaunchKernelGGL(k_gather_i32, dim3(gl), dim3(256), 0, st, lat->vlong, lperm, n_long, lsorted);
        PHL_HIP(hipGetLastError());
        PHL_HIP(hipMemcpyAsync(lat->vlong, lsorted, sizeof(int) * (size_t)n_long, hipMemcpyDeviceToDevice, st));
        PHL_HIP(hipStreamSynchronize(st));
    }
    return PHL_OK;
}

namespace {
int tile_pixels(int dp1)
{
    int P = 2048 / dp1;
    if (P > 256) P = 256;
    P &= ~15;
    if (const char *e = getenv("PHL_TILE_P")) {   // experiments: smaller chunks leave LDS headroom
        const int v = atoi(e) & ~15;
        if (v >= 16 && v <= P) P = v;
    }
    return P;
}

// 1. feature ranges -> the two widest dimensions -> uniform grid with ~P pixels per cell
// 2. pixels in cell-major order (ascending pixel inside a cell): a stable sort of the pixels by cell id.
//    O(n) whatever the features look like -- a constant or heavily clustered `ref` puts (nearly) all
//    pixels into one cell
// Launches only (given the ranges): lat->pix_order, `cell` [n], the grid's cell counts.
template <typename Pool>
int pixel_order(phl_lattice *lat, const float *ref, int64_t rs, int64_t cs, int P, const float *lo, const float *hi, int *cell,
                int *nca_out, int *ncb_out, Pool &tmp, hipStream_t st)
{
    const int d = lat->d, n = (int)lat->n;
    int da = 0, db = -1;
    for (int i = 1; i < d; i++)
        if (hi[i] - lo[i] > hi[da] - lo[da]) da = i;
    for (int i = 0; i < d; i++)
        if (i != da && (db < 0 || hi[i] - lo[i] > hi[db] - lo[db])) db = i;
    double ra = (double)hi[da] - lo[da], rb = db >= 0 ? (double)hi[db] - lo[db] : 0.0;
    if (!(ra > 0) || !isfinite(ra)) ra = 0;
    if (!(rb > 0) || !isfinite(rb)) { rb = 0; db = -1; }
    int nca = 1, ncb = 1;
    float inv_t = 0.f;
    if (ra > 0 && n > P) {
        double T = rb > 0 ? sqrt((double)P * ra * rb / n) : (double)P * ra / n;
        if (T > 0 && isfinite(T)) {
            nca = (int)fmin(ra / T, 32767.0) + 1;
            ncb = rb > 0 ? (int)fmin(rb / T, 32767.0) + 1 : 1;
            while ((int64_t)nca * ncb > (int64_t)4 * n + 1024) {
                T *= 1.5;
                nca = (int)fmin(ra / T, 32767.0) + 1;
                ncb = rb > 0 ? (int)fmin(rb / T, 32767.0) + 1 : 1;
            }
            inv_t = (float)(1.0 / T);
        }
    }
    const int ncell = nca * ncb;
    const unsigned gn = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_cell_ids, dim3(gn), dim3(256), 0, st, ref, rs, cs, (int64_t)n, da, db, lo[da],
                       db >= 0 ? lo[db] : 0.f, inv_t, nca, ncb, cell);
    PHL_HIP(hipGetLastError());
    PHL_HIP(phl_lat_alloc(lat->pix_order, (size_t)n));
    *nca_out = nca;
    *ncb_out = ncb;
    return stable_sort_perm(cell, n, ncell, lat->pix_order, tmp, st);
}
}  // namespace

size_t phl_tiles_pixel_order_scratch_bytes(int64_t n)
{
    // stable_sort_perm: two [256][blocks] histograms, a scan workspace, three [n] arrays (+ alignment slack)
    const size_t nblocks = ((size_t)n + RS_TILE - 1) / RS_TILE;
    return sizeof(int) * (2 * 256 * nblocks + 256 * nblocks / SCAN_TILE + 3 * (size_t)n) + 16 * 1024;
}

int phl_tiles_pixel_order(phl_lattice *lat, const float *ref, int64_t rs, int64_t cs, void *arena, size_t arena_bytes, hipStream_t st)
{
    const int n = (int)lat->n;
    if (n == 0 || !lat->feat_range_valid || lat->pix_order || lat->bt_cell) return PHL_OK;     // (phl_tiles_build does it)
    arena_pool tmp(arena, arena_bytes);
    PHL_HIP(phl_lat_alloc(lat->bt_cell, (size_t)n));
    return pixel_order(lat, ref, rs, cs, tile_pixels(lat->d + 1), lat->feat_lo, lat->feat_hi, lat->bt_cell, &lat->grid_nca,
                       &lat->grid_ncb, tmp, st);
}

int phl_tiles_build(phl_lattice *lat, const float *ref, int64_t rs, int64_t cs, hipStream_t st)
{
    int *const pix_ready = lat->bt_cell ? std::exchange(lat->pix_order, nullptr) : nullptr;   // made ahead (phl_tiles_pixel_order): keep it
    phl_tiles_free(lat);
    lat->pix_order = pix_ready;
    const int d = lat->d, dp1 = d + 1;
    const int n = (int)lat->n;
    const int P = tile_pixels(dp1);
    lat->P = P;
    if (n == 0) {
        phl_dev_block<uint32_t> scratch(st);        // (stays empty: no vertices, no packed keys)
        PHL_TRY(phl_rebuild_table_and_neighbors(lat, st, scratch));
        return phl_tiles_link_vertices(lat, st);   // (synchronises the stream)
    }
    int sortn = 512;
    while (sortn < P * dp1) sortn <<= 1;

    int rc = PHL_OK;
    int nchunks = 0;
    int64_t S = 0;
    const int64_t N = lat->N;
    // arrays replaced while launches that read them may still be in flight: dropped only behind the stream
    // synchronisation at the end of this phase (the block cache may hand a freed block to another thread's build)
    phl_dev_block<int16_t> vkeys_old(st);
    phl_dev_block<int32_t> vfirst_old(st);
    phl_dev_block<uint32_t> nbr_scratch(st);
    phl_fork_guard nbr_chain;                        // (declared behind the holders: its stream is drained before they wait for `st`)
    {   // temporaries of the chunk build go back to the scratch cache before the vertex lists are linked
    temp_pool tmp(st);
    // 1.-2. the pixel order (pixel_order above), unless it has been made under the table replay already
    int nca = 1, ncb = 1;
    int *cell, *tile_sums;
    PHL_HIP(tmp.get(&tile_sums, (size_t)n / SCAN_TILE + 2));
    if (pix_ready) {
        cell = lat->bt_cell;
        nca = lat->grid_nca;
        ncb = lat->grid_ncb;
    } else {
        std::vector<float> lo(d, INFINITY), hi(d, -INFINITY);
        if (lat->feat_range_valid) {          // found while elevating (phl_build_device)
            for (int i = 0; i < d; i++) { lo[i] = lat->feat_lo[i]; hi[i] = lat->feat_hi[i]; }
        } else {
            constexpr int MMB = 1024;
            float *mm_dev;
            PHL_HIP(tmp.get(&mm_dev, (size_t)MMB * d * 2));
            hipLaunchKernelGGL(k_minmax, dim3(MMB), dim3(256), 0, st, ref, rs, cs, (int64_t)n, d, mm_dev);
            PHL_HIP(hipGetLastError());
            std::vector<float> mm((size_t)MMB * d * 2);
            PHL_HIP(hipMemcpyAsync(mm.data(), mm_dev, sizeof(float) * mm.size(), hipMemcpyDeviceToHost, st));
            PHL_HIP(hipStreamSynchronize(st));
            for (int b = 0; b < MMB; b++)
                for (int i = 0; i < d; i++) {
                    lo[i] = fminf(lo[i], mm[((size_t)b * d + i) * 2]);
                    hi[i] = fmaxf(hi[i], mm[((size_t)b * d + i) * 2 + 1]);
                }
        }
        PHL_HIP(tmp.get(&cell, (size_t)n));
        PHL_TRY(pixel_order(lat, ref, rs, cs, P, lo.data(), hi.data(), cell, &nca, &ncb, tmp, st));
    }
    const int ncell = nca * ncb;

    // 2b. internal vertex numbering (see k_vertex_home), then the key -> vertex table and the blur neighbours
    {
        static const bool renumber = !(getenv("PHL_RENUMBER") && atoi(getenv("PHL_RENUMBER")) == 0);
        const int M_all = (int)lat->M;
        // a band cut out of the whole image's lattice (phl_sub_lattice) comes with ghost vertices behind its own ones:
        // only the own vertices are renumbered, the ghosts keep their rows (and the caller's order)
        const int M = (lat->M_local > 0 && lat->M_local < lat->M) ? (int)lat->M_local : M_all;
        // fresh build (phl_build_device's tables are there): the candidates' vertex ids are written once, below,
        // through the locality numbering -- unless the vertices' homes have to be read off replay[] first
        bool from_tables = lat->bt_slot_of != nullptr;
        bool wrote_vids = false;
        if (from_tables && !lat->vfirst) {
            rc = phl_write_final_vids(lat, st);      // (int_of_ft is null here: first-touch / reference ids)
            if (rc) return rc;
            from_tables = false;
        }
        if (renumber && ncell > 8 && M > 1) {
            int *vhome, *vkey;
            PHL_HIP(tmp.get(&vhome, (size_t)M));
            PHL_HIP(tmp.get(&vkey, (size_t)M));
            if (lat->vfirst) {
                hipLaunchKernelGGL(k_vertex_home_first, dim3((M + 255) / 256), dim3(256), 0, st, lat->vfirst, M, dp1, cell, vhome);
            } else {        // reference-table mode with duplicates: smallest cell among the touching pixels
                hipLaunchKernelGGL(k_fill_i32, dim3(256), dim3(256), 0, st, vhome, (int64_t)M, 0x7FFFFFFF);
                hipLaunchKernelGGL(k_vertex_home, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, lat->replay, (int)N, dp1, cell, vhome);
            }
            static const int nstrips = getenv("PHL_STRIPS") ? atoi(getenv("PHL_STRIPS")) : 8;
            const int stripw = (nca + nstrips - 1) / nstrips;
            hipLaunchKernelGGL(k_strip_key, dim3((M + 255) / 256), dim3(256), 0, st, vhome, M, nca, ncb, stripw, vkey);
            PHL_HIP(hipGetLastError());
            PHL_HIP(phl_lat_alloc(lat->ft_of_int, (size_t)M_all));
            PHL_HIP(phl_lat_alloc(lat->int_of_ft, (size_t)M_all));
            PHL_TRY(stable_sort_perm(vkey, M, (int64_t)(nstrips + 1) * ncb * stripw, lat->ft_of_int, tmp, st));
            if (M_all > M)        // ghosts: identity
                hipLaunchKernelGGL(k_iota_tail, dim3((M_all - M + 255) / 256), dim3(256), 0, st, lat->ft_of_int, M, M_all);
            hipLaunchKernelGGL(k_invert_perm, dim3((M_all + 255) / 256), dim3(256), 0, st, lat->ft_of_int, M_all, lat->int_of_ft);
            phl_dev_block<int16_t> vkeys_new(st);
            PHL_TRY(vkeys_new.alloc((size_t)M_all * d));
            hipLaunchKernelGGL(k_permute_keys, dim3((unsigned)(((int64_t)M_all * d + 255) / 256)), dim3(256), 0, st, lat->vkeys,
                               lat->ft_of_int, M_all, d, vkeys_new.get());
            if (from_tables) {
                PHL_TRY(phl_write_final_vids(lat, st));
                wrote_vids = true;
            } else {
                hipLaunchKernelGGL(k_relabel_replay, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, lat->replay, (int)N,
                                   lat->int_of_ft);
            }
            PHL_HIP(hipGetLastError());
            vkeys_old.adopt(lat->vkeys);             // still being read by the gather above
            lat->vkeys = vkeys_new.release();
        }
        if (from_tables && !wrote_vids) {            // no locality numbering: first-touch (reference) ids as they are
            PHL_TRY(phl_write_final_vids(lat, st));
        }
        vfirst_old.adopt(lat->vfirst);               // build-time only
        // key -> vertex table, packed keys, blur neighbours, composed pairs: ~100 us of small dependent launches that
        // nothing in the chunk build below depends on -- on a forked stream beside it, joined before this phase ends
        static const bool side_nbr = !(getenv("PHL_SIDE_NEIGHBORS") && atoi(getenv("PHL_SIDE_NEIGHBORS")) == 0);
        if (side_nbr) nbr_chain.fork(st);
        PHL_TRY(phl_rebuild_table_and_neighbors(lat, nbr_chain ? nbr_chain.stream() : st, nbr_scratch));
    }

    // 3. per-chunk local vertex lists, segments and local indices
    nchunks = (n + P - 1) / P;
    lat->nchunks = nchunks;
    int *nv;
    PHL_HIP(tmp.get(&nv, (size_t)nchunks + 1));
    PHL_HIP(phl_lat_alloc(lat->chunk_vptr, (size_t)nchunks + 1));
#define PHL_CHUNK_MASKS_X(HTX_, ...)                                                                                    \
    switch (sortn) {                                                                                                     \
        case 512: hipLaunchKernelGGL((k_chunk_masks<512, HTX_>), dim3(nchunks), dim3(256), 0, st, __VA_ARGS__); break;    \
        case 1024: hipLaunchKernelGGL((k_chunk_masks<1024, HTX_>), dim3(nchunks), dim3(256), 0, st, __VA_ARGS__); break;  \
        default: hipLaunchKernelGGL((k_chunk_masks<2048, HTX_>), dim3(nchunks), dim3(256), 0, st, __VA_ARGS__); break;    \
    }
#define PHL_CHUNK_MASKS(...)                                           \
    if (P * dp1 * 4 > sortn * 3) { PHL_CHUNK_MASKS_X(2, __VA_ARGS__) } \
    else { PHL_CHUNK_MASKS_X(1, __VA_ARGS__) }
#define PHL_CHUNK_SORT(WRITE_, ...)                                                                                      \
    switch (sortn) {                                                                                                      \
        case 512: hipLaunchKernelGGL((k_chunk_group<512, WRITE_>), dim3(nchunks), dim3(256), 0, st, __VA_ARGS__); break;   \
        case 1024: hipLaunchKernelGGL((k_chunk_group<1024, WRITE_>), dim3(nchunks), dim3(256), 0, st, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((k_chunk_group<2048, WRITE_>), dim3(nchunks), dim3(256), 0, st, __VA_ARGS__); break;   \
    }
    // One grouping pass: segments and local indices go to their final arrays, the per-chunk slot records to a
    // scratch area with a fixed stride; they are compacted once the chunk offsets are known.  Only when a
    // chunk has more local vertices than the stride (pixels that share next to nothing) the pass is repeated.
    constexpr int SLOT_STRIDE = 384;
    int *t_vert;
    int2 *t_rng;
    PHL_HIP(tmp.get(&t_vert, (size_t)nchunks * SLOT_STRIDE));
    PHL_HIP(tmp.get(&t_rng, (size_t)nchunks * SLOT_STRIDE));
    PHL_HIP(phl_lat_alloc(lat->seg, (size_t)N));
    PHL_HIP(phl_lat_alloc(lat->lidx, (size_t)N));
    // k_chunk_masks does every chunk with at most NVC local vertices; heavier ones only report their count here and
    // are done by k_chunk_group below, once the counts are on the host
    static const bool use_masks = !(getenv("PHL_CHUNK_MASKS") && atoi(getenv("PHL_CHUNK_MASKS")) == 0);
    if (use_masks) {
        PHL_CHUNK_MASKS(lat->pix_order, n, P, dp1, lat->replay, nv, (const int *)nullptr, SLOT_STRIDE, t_vert, t_rng, lat->seg,
                        lat->lidx)
    } else {
        PHL_CHUNK_SORT(true, lat->pix_order, n, P, dp1, lat->replay, nv, (const int *)nullptr, SLOT_STRIDE, t_vert, t_rng,
                       lat->seg, lat->lidx, (const int *)nullptr, 0)
    }
    PHL_HIP(hipGetLastError());
    PHL_TRY(exclusive_scan(nv, lat->chunk_vptr, nchunks, tile_sums, st));
    // (pinned staging where there is some: a copy into pageable memory would block the host twice)
    std::vector<int> nv_pageable, by_nv_pageable;
    int *nv_host = (int *)phl_pinned_alloc(sizeof(int) * (size_t)nchunks);
    int *by_nv = (int *)phl_pinned_alloc(sizeof(int) * (size_t)nchunks);
    if (!nv_host) { nv_pageable.resize((size_t)nchunks); nv_host = nv_pageable.data(); }
    if (!by_nv) { by_nv_pageable.resize((size_t)nchunks); by_nv = by_nv_pageable.data(); }
    PHL_HIP(hipMemcpyAsync(nv_host, nv, sizeof(int) * (size_t)nchunks, hipMemcpyDeviceToHost, st));
    PHL_HIP(hipStreamSynchronize(st));
    int nv_max = 0;
    for (int c = 0; c < nchunks; c++) {
        const int v = nv_host[c];
        S += v;
        if (v > nv_max) nv_max = v;
    }
    lat->S = S;
    lat->nv_max = nv_max;
    // chunk classes (plan_tiles): cumulative histogram of the vertex counts on the host, chunk ids by descending
    // vertex count on the device (counting sort; ascending chunk id among equals)
    {
        lat->nv_cum = (int *)malloc(sizeof(int) * ((size_t)nv_max + 2));
        if (!lat->nv_cum) { phl_set_error("phl_tiles_build: out of host memory"); return PHL_ERR_HIP; }
        std::vector<int> start((size_t)nv_max + 2, 0);
        for (int c = 0; c < nchunks; c++) start[(size_t)(nv_max - nv_host[c]) + 1]++;         // bin 0 = heaviest
        for (int b = 0; b <= nv_max; b++) start[(size_t)b + 1] += start[(size_t)b];
        for (int x = 0; x <= nv_max; x++) lat->nv_cum[x] = nchunks - start[(size_t)(nv_max - x)];   // #chunks with nv <= x
        for (int c = 0; c < nchunks; c++) by_nv[start[(size_t)(nv_max - nv_host[c])]++] = c;
        PHL_HIP(phl_lat_alloc(lat->chunk_by_nv, (size_t)nchunks + 1));
        PHL_HIP(hipMemcpyAsync(lat->chunk_by_nv, by_nv, sizeof(int) * (size_t)nchunks, hipMemcpyHostToDevice, st));
    }
    PHL_HIP(phl_lat_alloc(lat->slot_vert, (size_t)S + 1));
    PHL_HIP(phl_lat_alloc(lat->seg_rng, (size_t)S + 1));
    if (nv_max <= SLOT_STRIDE) {
        if (use_masks && nv_max > NVC) {     // the chunks k_chunk_masks left out (first-pass form: slot records to the scratch)
            PHL_CHUNK_SORT(true, lat->pix_order, n, P, dp1, lat->replay, (int *)nullptr, (const int *)nullptr, SLOT_STRIDE, t_vert,
                           t_rng, lat->seg, lat->lidx, (const int *)nv, NVC)
        }
        hipLaunchKernelGGL(k_compact_slots, dim3(nchunks), dim3(256), 0, st, lat->chunk_vptr, nchunks, SLOT_STRIDE, t_vert,
                           t_rng, lat->slot_vert, lat->seg_rng);
    } else {
        if (use_masks) {
            PHL_CHUNK_MASKS(lat->pix_order, n, P, dp1, lat->replay, (int *)nullptr, lat->chunk_vptr, 0, lat->slot_vert,
                            lat->seg_rng, lat->seg, lat->lidx)
            if (nv_max > NVC) {
                PHL_CHUNK_SORT(true, lat->pix_order, n, P, dp1, lat->replay, (int *)nullptr, lat->chunk_vptr, 0, lat->slot_vert,
                               lat->seg_rng, lat->seg, lat->lidx, (const int *)nv, NVC)
            }
        } else {
            PHL_CHUNK_SORT(true, lat->pix_order, n, P, dp1, lat->replay, (int *)nullptr, lat->chunk_vptr, 0, lat->slot_vert,
                           lat->seg_rng, lat->seg, lat->lidx, (const int *)nullptr, 0)
        }
    }
#undef PHL_CHUNK_SORT
#undef PHL_CHUNK_MASKS
#undef PHL_CHUNK_MASKS_X
    PHL_HIP(hipGetLastError());
    PHL_HIP(nbr_chain.join(st));
    PHL_HIP(hipStreamSynchronize(st));
    }
    phl_release_build_tables(lat);                 // (read by k_final_vid: behind the synchronisation)
    PHL_TRY(phl_tiles_link_vertices(lat, st));
    PHL_TRY(vkeys_old.drop());                     // (the stream has been synchronised since their last readers)
    PHL_TRY(vfirst_old.drop());
    PHL_TRY(nbr_scratch.drop());
    lat->table_bytes = (int64_t)(sizeof(int16_t) * (size_t)lat->M * d + sizeof(phl_replay_t) * (size_t)N +
                                 sizeof(int32_t) * (size_t)lat->M * (d + 1) * 2 + sizeof(int32_t) * (size_t)lat->M * ((d + 1) / 2) * 8 +
                                 sizeof(int) * ((size_t)lat->table_mask + 1) + (lat->int_of_ft ? 2 * sizeof(int) * (size_t)lat->M : 0) +
                                 sizeof(int32_t) * ((size_t)lat->M * (8 * lat->np3 + lat->n3) + (size_t)(lat->nitems3 + 1) * lat->n3));
    lat->tile_bytes = (int64_t)(sizeof(int) * ((size_t)n + nchunks + 1 + 3 * ((size_t)S + 1) + (size_t)lat->M + 1) +
                                sizeof(phl_contrib_t) * ((size_t)N + S + 1) + sizeof(unsigned short) * (size_t)N);
    return PHL_OK;
}

// which chunks hold a slot of any of the listed vertex rows
__global__ __launch_bounds__(256) void k_mark_chunks(const int64_t *__restrict__ rows, int64_t k, const int *__restrict__ vs_ptr,
                                                     const phl_contrib_t *__restrict__ vs, const int *__restrict__ chunk_vptr,
                                                     int nchunks, int *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const int64_t v = rows[i];
    for (int e = vs_ptr[v]; e < vs_ptr[v + 1]; e++) {
        const int slot = vs[e].pixel;
        int lo = 0, hi = nchunks - 1;                     // chunk_vptr[c] <= slot < chunk_vptr[c + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (chunk_vptr[mid] <= slot) lo = mid;
            else hi = mid - 1;
        }
        mask[lo] = 1;
    }
}

int phl_tiles_chunks_touching(phl_lattice *lat, const int64_t *rows_dev, int64_t k, int32_t *mask_host, hipStream_t st)
{
    const int nchunks = lat->nchunks;
    if (nchunks == 0) return PHL_OK;
    temp_pool tmp(st);
    int *mask;
    PHL_HIP(tmp.get(&mask, (size_t)nchunks));
    PHL_HIP(hipMemsetAsync(mask, 0, sizeof(int) * (size_t)nchunks, st));
    if (k > 0) {
        hipLaunchKernelGGL(k_mark_chunks, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, rows_dev, k, lat->vs_ptr, lat->vs,
                           lat->chunk_vptr, nchunks, mask);
        PHL_HIP(hipGetLastError());
    }
    PHL_HIP(hipMemcpyAsync(mask_host, mask, sizeof(int) * (size_t)nchunks, hipMemcpyDeviceToHost, st));
    PHL_HIP(hipStreamSynchronize(st));
    return PHL_OK;
}
