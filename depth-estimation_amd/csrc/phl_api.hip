// phl_api.hip -- host side of the C ABI declared in include/phl.h.
//
// No CPU fallback lives here on purpose: without a HIP device every entry point that would
// compute returns PHL_ERR_NO_DEVICE / PHL_ERR_HIP.  The CPU restatement under oracle/ is test
// infrastructure and is never linked into this library.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <chrono>
#include <mutex>
#include <utility>
#include <vector>

#include "phl_internal.h"

namespace {
thread_local char g_err[512] = "";

struct device_guard {
    int prev = -1;
    bool ok = false;
    explicit device_guard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
    }
    ~device_guard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int grow(float **p, int64_t *cap, int64_t need)
{
    if (need <= *cap) return PHL_OK;
    if (*p) {
        PHL_HIP(hipDeviceSynchronize());      // (rare) the old buffer may still be read by launches in flight
        PHL_HIP(phl_dev_free(*p));
    }
    *p = nullptr;
    *cap = 0;
    PHL_HIP(phl_dev_malloc((void **)p, sizeof(float) * (size_t)need));
    *cap = need;
    return PHL_OK;
}
}  // namespace

// ---- device block cache --------------------------------------------------------------------------------
// hipMalloc / hipFree cost 50-300 us each and hipFree synchronises the device; a lattice owns ~20 device arrays,
// so the reference-shaped call (build, filter, destroy per call: phl_filter_once) spent as long in the allocator
// as in its kernels.  Blocks released by a lattice are kept, by device and size class (sizes rounded up to 1/8 of
// their power of two, so that the arrays of a slightly different image fit the same blocks), and handed to the
// next build.  A caller of phl_dev_free guarantees that no launch still uses the block, or that its next user
// is ordered behind it (phl_destroy synchronises the device first, as hipFree itself would).
// PHL_CACHE_MAX_MB (default 8192, 0 = off) caps the cached bytes; phl_trim_scratch() releases everything.
namespace {
struct dev_cache_t {
    std::mutex mu;
    std::map<std::pair<int, size_t>, std::vector<void *>> free_blocks;
    std::map<void *, std::pair<int, size_t>> live;      // every block handed out: device, class size
    size_t cached = 0;
};
dev_cache_t &dev_cache()
{
    static dev_cache_t *c = new dev_cache_t();          // never destroyed: the HIP runtime may be gone at exit
    return *c;
}
size_t cache_limit()
{
    static const size_t lim = [] {
        const char *e = getenv("PHL_CACHE_MAX_MB");
        return (size_t)(e ? atoll(e) : 8192) << 20;
    }();
    return lim;
}
size_t size_class(size_t bytes)
{
    if (bytes < 4096) return 4096;
    size_t p2 = 1;
    while (p2 * 2 <= bytes) p2 *= 2;
    const size_t step = p2 / 8;
    return (bytes + step - 1) / step * step;
}
void cache_flush_locked(dev_cache_t &c)
{
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (auto &kv : c.free_blocks) {
        (void)hipSetDevice(kv.first.first);
        for (void *p : kv.second) (void)hipFree(p);
    }
    c.free_blocks.clear();
    c.cached = 0;
    if (prev >= 0) (void)hipSetDevice(prev);
}
}  // namespace

hipError_t phl_dev_malloc(void **p, size_t bytes)
{
    dev_cache_t &c = dev_cache();
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const size_t cls = size_class(bytes);
    {
        std::lock_guard<std::mutex> lk(c.mu);
        auto it = c.free_blocks.find({dev, cls});
        if (it != c.free_blocks.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            c.cached -= cls;
            c.live[*p] = {dev, cls};
            return hipSuccess;
        }
    }
    e = hipMalloc(p, cls);
    if (e != hipSuccess) {                               // out of memory: give the cached blocks back and retry once
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(c.mu);
        cache_flush_locked(c);
        e = hipMalloc(p, cls);
        if (e != hipSuccess) return e;
    }
    std::lock_guard<std::mutex> lk(c.mu);
    c.live[*p] = {dev, cls};
    return hipSuccess;
}

hipError_t phl_dev_free(void *p)
{
    if (!p) return hipSuccess;
    dev_cache_t &c = dev_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.live.find(p);
    if (it == c.live.end()) return hipFree(p);           // not ours
    const std::pair<int, size_t> key = it->second;
    c.live.erase(it);
    if (cache_limit() == 0 || key.second > cache_limit()) return hipFree(p);
    if (c.cached + key.second > cache_limit()) cache_flush_locked(c);
    c.free_blocks[key].push_back(p);
    c.cached += key.second;
    return hipSuccess;
}

// test hook: blocks handed out and not yet given back
extern "C" int64_t phl_debug_live_blocks(void)
{
    dev_cache_t &c = dev_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    return (int64_t)c.live.size();
}

// ---- value workspaces --------------------------------------------------------------------------------
// SURVEY 8(b), threading row: "re-entrant; autograd may call from any thread".  A lattice's tables are
// read-only after the build; what a filter call WRITES (the [M][vd] ping-pong pair, partial rows, staging
// copies) lives in a workspace the call takes for the duration of its launches.  A workspace is handed out
// again when (a) it has never carried work, (b) the caller enqueues on the stream that used it last (stream
// order protects it), or (c) the event recorded behind its last launch has completed.  Otherwise a new one is
// allocated: two threads on two streams run concurrently on separate buffers.  A workspace whose launches were
// captured into a HIP graph stays bound to that stream and is never resized (the graph holds its pointers).
struct phl_shared {
    std::mutex mu;                       // guards `ws` and the workspaces' state flags
    std::vector<phl_workspace *> ws;

    std::mutex csr_mu;                   // one-time build of the pixel-sorted lists (phl_ensure_csr)
};

namespace {
void ws_free_buffers(phl_workspace *w)
{
    void *ptrs[] = {w->buf[0], w->buf[1], w->partial, w->stage_in, w->stage_out};
    for (void *p : ptrs)
        if (p) (void)phl_dev_free(p);
    w->buf[0] = w->buf[1] = w->partial = w->stage_in = w->stage_out = nullptr;
    w->buf_elems = w->partial_elems = w->stage_elems = 0;
}

// (no fence needed: the launches it stands behind finished before it started -- stream order -- and the store
//  itself is released to the host at the kernel's end; tools/mark_probe.hip: 2.7 us in-stream, against 3.5 us with
//  a system fence and 4.4 us for hipStreamWriteValue64)
__global__ void k_mark_done(unsigned long long *word, unsigned long long ticket)
{
    *reinterpret_cast<volatile unsigned long long *>(word) = ticket;
}

bool ws_drained(const phl_workspace *w)
{
    return w->done_word && *reinterpret_cast<volatile unsigned long long *>(w->done_word) == w->ticket;
}

bool is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return cs != hipStreamCaptureStatusNone;
}
}  // namespace

std::mutex *phl_csr_mutex(phl_lattice *lat) { return &lat->shared->csr_mu; }

int phl_ws_acquire(phl_lattice *lat, hipStream_t st, int64_t buf_elems, int64_t partial_elems, int64_t stage_elems,
                   phl_workspace **out)
{
    phl_shared *sh = lat->shared;
    phl_workspace *w = nullptr;
    {
        std::lock_guard<std::mutex> lk(sh->mu);
        phl_workspace *fits = nullptr, *any = nullptr;
        for (phl_workspace *c : sh->ws) {
            if (c->in_enqueue) continue;
            if (c->stream_bound && c->last_stream != st) {
                if (c->captured || !ws_drained(c)) continue;
                c->stream_bound = false;       // its work has drained
            }
            const bool big = c->buf_elems >= buf_elems && c->partial_elems >= partial_elems && c->stage_elems >= stage_elems;
            if (big && !fits) fits = c;
            if (!c->captured && !any) any = c;  // may be grown
        }
        w = fits ? fits : any;
        if (!w) {
            w = new phl_workspace();
            memset(w, 0, sizeof(*w));
            // pinned, device-visible host word for the completion mark (cannot be allocated during a capture:
            // such a workspace then simply stays bound to its stream)
            void *hw = nullptr;
            if (hipHostMalloc(&hw, sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess) {
                w->done_word = (unsigned long long *)hw;
                *w->done_word = 0;
            } else {
                (void)hipGetLastError();
            }
            sh->ws.push_back(w);
        }
        w->in_enqueue = true;
    }
    int rc = PHL_OK;
    if (buf_elems > w->buf_elems) {
        int64_t c0 = w->buf_elems, c1 = w->buf_elems;
        rc = grow(&w->buf[0], &c0, buf_elems);
        if (!rc) rc = grow(&w->buf[1], &c1, buf_elems);
        w->buf_elems = rc ? 0 : buf_elems;
    }
    if (!rc && partial_elems > w->partial_elems) {
        rc = grow(&w->partial, &w->partial_elems, partial_elems);
    }
    if (!rc && stage_elems > w->stage_elems) {
        int64_t c0 = w->stage_elems, c1 = w->stage_elems;
        rc = grow(&w->stage_in, &c0, stage_elems);
        if (!rc) rc = grow(&w->stage_out, &c1, stage_elems);
        w->stage_elems = rc ? 0 : stage_elems;
    }
    if (rc) {
        std::lock_guard<std::mutex> lk(sh->mu);
        w->in_enqueue = false;
        return rc;
    }
    *out = w;
    return PHL_OK;
}

void phl_ws_release(phl_lattice *lat, phl_workspace *w, hipStream_t st, bool idle)
{
    if (!idle) {
        // a captured call binds its workspace to the stream for good (the graph keeps the pointers), so nobody will
        // ever ask whether its work has drained: no completion mark inside a graph (one launch of seven saved per
        // replayed Tsukuba-sized filter, where launches are what is being paid for)
        const bool capturing = is_capturing(st);
        if (capturing) w->captured = true;
        w->ticket++;
        if (w->done_word && !capturing) {
            hipLaunchKernelGGL(k_mark_done, dim3(1), dim3(1), 0, st, w->done_word, w->ticket);
            if (hipGetLastError() != hipSuccess) w->ticket += 1ull << 32;   // never reads as drained
        }
    }
    std::lock_guard<std::mutex> lk(lat->shared->mu);
    if (!idle) {
        w->last_stream = st;
        w->stream_bound = true;
    }
    w->in_enqueue = false;
}

// ---- cached scratch block for build temporaries -------------------------------------------------
namespace {
std::mutex g_scratch_mu;
void *g_scratch = nullptr;
size_t g_scratch_cap = 0;
int g_scratch_dev = -1;
bool g_scratch_busy = false;
}  // namespace

namespace {
struct pinned_arena {
    char *base = nullptr;
    size_t cap = 0, off = 0, wanted = 0;
};
thread_local pinned_arena t_pinned;     // (never freed: a thread's exit may come after the runtime has shut down;
                                        //  portable: one thread may build on several devices in turn)
}  // namespace

void phl_pinned_reset()
{
    pinned_arena &a = t_pinned;
    if (a.wanted > a.cap || !a.base) {
        size_t want = a.wanted > ((size_t)1 << 20) ? a.wanted + (a.wanted >> 2) : ((size_t)1 << 20);
        if (want <= ((size_t)256 << 20)) {
            if (a.base) (void)hipHostFree(a.base);
            a.base = nullptr;
            a.cap = 0;
            void *p = nullptr;
            if (hipHostMalloc(&p, want, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess) {
                a.base = (char *)p;
                a.cap = want;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    a.off = 0;
    a.wanted = 0;
}

void *phl_pinned_alloc(size_t bytes)
{
    pinned_arena &a = t_pinned;
    bytes = (bytes + 255) & ~(size_t)255;
    a.wanted += bytes;
    if (!a.base || a.off + bytes > a.cap) return nullptr;
    void *p = a.base + a.off;
    a.off += bytes;
    return p;
}

bool phl_scratch_acquire(void **base, size_t *cap)
{
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    if (g_scratch_busy) return false;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (g_scratch && dev != g_scratch_dev) {   // lattices are being built on another device now
        int prev = dev;
        (void)hipSetDevice(g_scratch_dev);
        (void)hipFree(g_scratch);
        (void)hipSetDevice(prev);
        g_scratch = nullptr;
        g_scratch_cap = 0;
    }
    g_scratch_dev = dev;
    g_scratch_busy = true;
    *base = g_scratch;
    *cap = g_scratch_cap;
    return true;
}

void phl_scratch_release(size_t wanted)
{
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    g_scratch_busy = false;
    static const size_t limit = [] {
        const char *e = getenv("PHL_SCRATCH_MAX_MB");   // 0 disables the cache
        return (size_t)(e ? atoll(e) : 4096) << 20;
    }();
    if (wanted > g_scratch_cap && wanted <= limit) {
        if (g_scratch) (void)hipFree(g_scratch);
        g_scratch = nullptr;
        g_scratch_cap = 0;
        const size_t want = wanted + (wanted >> 3);
        if (hipMalloc(&g_scratch, want) == hipSuccess) g_scratch_cap = want;
        else (void)hipGetLastError();
    }
}

// ---- side streams (phl_fork_guard) ------------------------------------------------------------------------------------
// A chunk class of a few heavy chunks (textured 16x16 tiles of a natural image: 35 us for 0.6 MB at C3) used to run as its
// own launch BEHIND the main grid, the whole chip waiting for a handful of workgroups.  It now runs BESIDE the main grid, on
// a high-priority side stream forked from the caller's (event fork / join: legal inside a stream capture too).  Slots are
// pooled per device; a slot is taken for the duration of the host call only -- later users of the same stream are ordered
// behind the earlier work, and an event wait refers to the record that preceded it, so re-recording an event is safe.
struct phl_fork_slot {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool busy = false;
};
namespace {
std::mutex g_fork_mu;
std::map<int, std::vector<phl_fork_slot *>> g_fork_pool;        // (never destroyed: the runtime may be gone at exit)

phl_fork_slot *fork_acquire()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lk(g_fork_mu);
    for (phl_fork_slot *f : g_fork_pool[dev])
        if (!f->busy) { f->busy = true; return f; }
    if (g_fork_pool[dev].size() >= 16) return nullptr;
    phl_fork_slot *f = new phl_fork_slot();
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);        // hi = the numerically lowest value = the highest priority
    if (hipStreamCreateWithPriority(&f->s, hipStreamNonBlocking, hi) != hipSuccess ||
        hipEventCreateWithFlags(&f->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&f->join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (f->s) (void)hipStreamDestroy(f->s);
        if (f->fork) (void)hipEventDestroy(f->fork);
        if (f->join) (void)hipEventDestroy(f->join);
        delete f;
        return nullptr;
    }
    f->busy = true;
    g_fork_pool[dev].push_back(f);
    return f;
}
void fork_release(phl_fork_slot *f)
{
    if (!f) return;
    std::lock_guard<std::mutex> lk(g_fork_mu);
    f->busy = false;
}
}  // namespace

// fork from `st` (work enqueued on the slot's stream starts behind everything enqueued on st so far)
bool phl_fork_guard::fork(hipStream_t st)
{
    if (f) return true;
    f = fork_acquire();
    if (f && (hipEventRecord(f->fork, st) != hipSuccess || hipStreamWaitEvent(f->s, f->fork, 0) != hipSuccess)) {
        (void)hipGetLastError();
        fork_release(f);
        f = nullptr;
    }
    return f != nullptr;
}
hipStream_t phl_fork_guard::stream() const { return f->s; }
// A forked chain inside a host function with temporaries: on any exit the side stream is drained before they are released.
phl_fork_guard::~phl_fork_guard()
{
    if (!f) return;
    (void)hipStreamSynchronize(f->s);
    fork_release(f);
}
// make `st` wait for the chain, give the slot back
hipError_t phl_fork_guard::join(hipStream_t st)
{
    if (!f) return hipSuccess;
    hipError_t e = hipEventRecord(f->join, f->s);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, f->join, 0);
    if (e == hipSuccess) {
        fork_release(f);
        f = nullptr;
    }
    return e;
}

void phl_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int phl_hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    const char *base = strrchr(file, '/');
    phl_set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, base ? base + 1 : file, line);
    (void)hipGetLastError();  // clear sticky state
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? PHL_ERR_NO_DEVICE : PHL_ERR_HIP;
}

int phl_raise_lds_limit(const void *kernel, size_t bytes)
{
    if (bytes <= 64 * 1024) return PHL_OK;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> allowed;
    int dev = 0;
    PHL_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    size_t &have = allowed[std::make_pair(dev, kernel)];
    if (bytes > have) {
        PHL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    return PHL_OK;
}

// an empty handle: the initial state of every lattice (phl_build_ex and phl_sub_lattice fill it)
phl_lattice *phl_lattice_blank(int device, int d, int64_t n, unsigned build_flags)
{
    phl_lattice *lat = new phl_lattice();
    memset(lat, 0, sizeof(*lat));
    lat->device = device;
    lat->d = d;
    lat->n = n;
    lat->build_flags = build_flags;
    lat->nbr00_override = -2;
    lat->shared = new phl_shared();
    return lat;
}

// ---- the plan of a filter call ----------------------------------------------------------------------------------------
// Every call that runs the splat or the slice makes one decision: the width the kernels run at, which side is staged,
// chunk kernels or gather kernels for each of the two stages, and what that asks of the workspace.  plan_call is the
// only place that makes it -- phl_reserve_ex sizes the workspace from the same plan the next phl_filter will compute,
// which is what "the next filter call allocates nothing" (HIP-graph capture) rests on.
namespace {
// fp32 rows as a call sees them; the default is "none": on the 16-byte grid, pixel-major
struct phl_operand {
    const void *base = nullptr;
    int64_t rs = 0, cs = 1;
};
bool rows16(const phl_operand &o) { return phl_rows16(o.base, o.rs); }

struct phl_call_plan {
    int vdw;                    // the width the kernels run at: vd, or vd rounded up to a multiple of 4 (both sides staged)
    bool stage_src, stage_dst;  // copied into / out of [n][vdw] rows of the workspace
    bool chunk_splat, chunk_slice;      // the chunk kernels (phl_tiles.hip); else the gather kernels (phl_filter.hip)
    int64_t buf_elems, partial_elems, stage_elems;      // floats asked of the workspace (phl_ws_acquire)
};

// src: what the splat reads (and the slice subtracts under PHL_FILTER_SUBTRACT_INPUT); dst: what the slice writes.
// in_place: the stage-level calls hand in vertex rows of their own (phl_filter_grad: its second splat source) -- then
// every operand is used where it lies, nothing is staged or widened, and the workspace holds the partial rows only.
phl_call_plan plan_call(const phl_lattice *lat, int vd, unsigned flags, phl_operand src, phl_operand dst,
                        const phl_operand *in_place = nullptr)
{
    phl_call_plan p = {};
    p.vdw = vd;
    const bool no_chunk_splat = (flags & (PHL_FILTER_EXACT | PHL_FILTER_NO_TILES)) != 0;
    if (!in_place) {
        // pixel-major rows are consumed in place; anything else (e.g. the [n,L] view of an NCHW
        // tensor, gaussian_matrix.py:348) is staged through one coalesced transpose
        p.stage_src = (src.cs != 1) && vd > 1;
        p.stage_dst = (dst.cs != 1) && vd > 1;
        // Rows the chunk kernels cannot take -- a channel count that is not a multiple of 4 (the reference's max_disp = w // 6:
        // 231 at 1390 columns), a row stride or base address off the 16-byte grid (a column slice of a wider tensor) -- used to
        // fall back to the gather kernels (2.4x slower at 1390x1110x231).  From 128 channels on they are staged instead: one
        // copy into / out of a buffer with 16-byte rows, the kernels run at the width rounded up to a multiple of 4.  (Below
        // that the two extra passes over the volume cost more than the gather kernels lose: tools/odd_narrow.py, 1390x1110 --
        // 9 channels 0.46 vs 0.27 ms, 50: 0.87 vs 0.83, 110: 1.29 vs 1.20, 130: 1.48 vs 1.59, 231: 2.59 vs 3.14.)
        if (vd >= 128 && !no_chunk_splat) {
            if (vd % 4) {
                p.vdw = (vd + 3) & ~3;
                p.stage_src = p.stage_dst = true;
            } else {
                p.stage_src = p.stage_src || !rows16(src);
                p.stage_dst = p.stage_dst || !rows16(dst);
            }
        }
        p.buf_elems = lat->M * (int64_t)p.vdw;
        if (p.stage_src || p.stage_dst) p.stage_elems = lat->n * (int64_t)p.vdw;
    }
    if (p.stage_src) src = {nullptr, p.vdw, 1};
    if (p.stage_dst) dst = {nullptr, p.vdw, 1};
    const bool vert16 = !in_place || rows16(*in_place);     // (the workspace's own vertex rows are on the grid)
    // Partial rows cost 2 * S_multi row transfers (written, re-read); staging saves d of the d+1 reads the gather
    // splat makes of every pixel row.  Break-even is far out (S_multi = d/2 * n); beyond 2n the chunks share so
    // little that the gather form is taken (the iid stress case sits at ~0.9n and is still 1.3x faster staged).
    p.chunk_splat = !no_chunk_splat && phl_tiles_lprs(lat, p.vdw, 0) >= 0 && rows16(src) && vert16 && lat->S_multi <= 2 * lat->n;
    const bool sub16 = !(flags & PHL_FILTER_SUBTRACT_INPUT) || rows16(src);
    p.chunk_slice = !(flags & PHL_FILTER_NO_TILES) && phl_tiles_lprs(lat, p.vdw, 1) >= 0 && vert16 && rows16(dst) && sub16 &&
                    lat->S <= 3 * lat->n;
    if (p.chunk_splat) p.partial_elems = lat->S_multi * (int64_t)p.vdw;
    return p;
}
// the operands phl_reserve_ex's flags describe, and phl_tile_stats' "any rows on the grid": aligned pixel-major rows, or
// (strided) a view whose columns are not adjacent, which both sides of a filter call stage
phl_operand described_rows(int vd, bool strided = false) { return {nullptr, (vd + 3) & ~3, strided ? 2 : 1}; }

// A workspace for the duration of a host call: acquired on request, given back by the destructor on every exit (a
// workspace that is never released stays marked in_enqueue for good).  idle: it was sized and carries no work.
struct ws_lease {
    phl_lattice *lat;
    hipStream_t st;
    phl_workspace *w = nullptr;
    bool idle = false;
    ws_lease(phl_lattice *l, hipStream_t s) : lat(l), st(s) {}
    ws_lease(const ws_lease &) = delete;
    ws_lease &operator=(const ws_lease &) = delete;
    ~ws_lease()
    {
        if (w) phl_ws_release(lat, w, st, idle);
    }
    int acquire(int64_t buf_elems, int64_t partial_elems, int64_t stage_elems)
    {
        return phl_ws_acquire(lat, st, buf_elems, partial_elems, stage_elems, &w);
    }
    int acquire(const phl_call_plan &p) { return acquire(p.buf_elems, p.partial_elems, p.stage_elems); }
    phl_workspace *operator->() const { return w; }
};
}  // namespace

extern "C" {

int phl_version(void) { return PHL_VERSION; }
const char *phl_last_error(void) { return g_err; }

const char *phl_status_string(int s)
{
    switch (s) {
        case PHL_OK: return "ok";
        case PHL_ERR_INVALID: return "invalid argument";
        case PHL_ERR_SHAPE: return "incompatible shapes";
        case PHL_ERR_HIP: return "HIP runtime error";
        case PHL_ERR_NO_DEVICE: return "no HIP device";
        case PHL_ERR_KEY_RANGE: return "lattice key outside int16";
        case PHL_ERR_TOO_LARGE: return "problem too large for int32 indexing";
        case PHL_ERR_UNSUPPORTED: return "unsupported";
        default: return "unknown";
    }
}

int phl_trim_scratch(void)
{
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    if (g_scratch_busy) return PHL_OK;
    if (g_scratch) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(g_scratch_dev);
        (void)hipFree(g_scratch);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    g_scratch = nullptr;
    g_scratch_cap = 0;
    {
        dev_cache_t &c = dev_cache();
        std::lock_guard<std::mutex> lk2(c.mu);
        cache_flush_locked(c);
    }
    return PHL_OK;
}

int phl_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int phl_build(phl_lattice **out, const float *ref_dev, int64_t n, int d, int64_t rs, int64_t cs, int device,
              phl_stream stream)
{
    return phl_build_ex(out, ref_dev, n, d, rs, cs, device, stream, PHL_BUILD_DEFAULT);
}

int phl_build_ex(phl_lattice **out, const float *ref_dev, int64_t n, int d, int64_t rs, int64_t cs, int device,
                 phl_stream stream, unsigned build_flags)
{
    if (!out) { phl_set_error("phl_build: out is NULL"); return PHL_ERR_INVALID; }
    *out = nullptr;
    if (n < 0 || d < 1 || (n > 0 && !ref_dev)) { phl_set_error("phl_build: bad arguments (n=%lld d=%d)", (long long)n, d); return PHL_ERR_INVALID; }
    if (d > PHL_MAX_D) { phl_set_error("phl_build: d=%d exceeds PHL_MAX_D=%d", d, PHL_MAX_D); return PHL_ERR_UNSUPPORTED; }
    if (n * (int64_t)(d + 1) > (int64_t)1 << 30) { phl_set_error("phl_build: n*(d+1)=%lld exceeds 2^30", (long long)(n * (d + 1))); return PHL_ERR_TOO_LARGE; }
    if (phl_device_count() <= device || device < 0) { phl_set_error("phl_build: HIP device %d not available (no CPU fallback)", device); return PHL_ERR_NO_DEVICE; }
    device_guard g(device);
    if (!g.ok) { phl_set_error("phl_build: cannot select device %d", device); return PHL_ERR_NO_DEVICE; }

    phl_lattice *lat = phl_lattice_blank(device, d, n, build_flags);
    static const bool dbg_t = getenv("PHL_DEBUG") != nullptr;
    const auto tb0 = std::chrono::steady_clock::now();
    int rc = phl_build_device(lat, ref_dev, rs, cs, (hipStream_t)stream);
    const auto tb1 = std::chrono::steady_clock::now();
    if (rc == PHL_OK) rc = phl_tiles_build(lat, ref_dev, rs, cs, (hipStream_t)stream);
    if (dbg_t)
        fprintf(stderr, "[phl] build: vertices %.2f ms, chunks %.2f ms\n", std::chrono::duration<double, std::milli>(tb1 - tb0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb1).count());
    if (rc != PHL_OK) {
        phl_destroy(lat);
        return rc;
    }
    *out = lat;
    return PHL_OK;
}

int phl_destroy(phl_lattice *lat)
{
    if (!lat) return PHL_OK;
    device_guard g(lat->device);
    (void)hipDeviceSynchronize();      // what hipFree would do: nothing may still be using the arrays (they are cached, not freed)
    phl_tiles_free(lat);
    phl_release_build_tables(lat);                 // (only a build that failed half-way leaves any)
    phl_lat_free_persistent(lat);
    if (lat->shared) {
        for (phl_workspace *w : lat->shared->ws) {
            ws_free_buffers(w);
            if (w->done_word) (void)hipHostFree(w->done_word);
            delete w;
        }
        delete lat->shared;
    }
    delete lat;
    return PHL_OK;
}

int64_t phl_num_pixels(const phl_lattice *lat) { return lat ? lat->n : -1; }
int64_t phl_num_vertices(const phl_lattice *lat) { return lat ? lat->M : -1; }
int phl_num_dims(const phl_lattice *lat) { return lat ? lat->d : -1; }
int phl_device(const phl_lattice *lat) { return lat ? lat->device : -1; }
int64_t phl_device_bytes(const phl_lattice *lat)
{
    if (!lat) return -1;
    int64_t b = lat->table_bytes + lat->tile_bytes;
    std::lock_guard<std::mutex> lk(lat->shared->mu);
    for (const phl_workspace *w : lat->shared->ws)
        b += (w->partial_elems + 2 * w->buf_elems + 2 * w->stage_elems) * (int64_t)sizeof(float);
    return b;
}

int64_t phl_num_local_vertices(const phl_lattice *lat) { return lat ? lat->M_local : -1; }

int phl_add_vertices(phl_lattice *lat, const int16_t *keys_host, int64_t count, int32_t *vid_host, phl_stream stream)
{
    if (!lat || count < 0 || (count > 0 && (!keys_host || !vid_host))) { phl_set_error("phl_add_vertices: bad arguments"); return PHL_ERR_INVALID; }
    if (lat->M + count > ((int64_t)1 << 30)) { phl_set_error("phl_add_vertices: too many vertices"); return PHL_ERR_TOO_LARGE; }
    device_guard g(lat->device);
    const int64_t M_before = lat->M;
    int rc = phl_add_vertices_device(lat, keys_host, count, vid_host, (hipStream_t)stream);
    lat->blur_rows_set = 0;            // row ranges are rows of the old vertex array
    if (rc == PHL_OK && lat->M != M_before) {
        rc = phl_tiles_link_vertices(lat, (hipStream_t)stream);
        // the value workspaces are sized by M and S_multi: drop them (not a concurrent operation: the lattice is
        // still being assembled)
        std::lock_guard<std::mutex> lk(lat->shared->mu);
        for (phl_workspace *w : lat->shared->ws) ws_free_buffers(w);
    }
    return rc;
}

int phl_set_blur_rows(phl_lattice *lat, const int64_t *ranges, int naxes)
{
    if (!lat) { phl_set_error("phl_set_blur_rows: bad arguments"); return PHL_ERR_INVALID; }
    if (!ranges || naxes == 0) {        // back to all rows on every axis
        lat->blur_rows_set = 0;
        return PHL_OK;
    }
    if (naxes != lat->d + 1) { phl_set_error("phl_set_blur_rows: %d axes given, the lattice has %d", naxes, lat->d + 1); return PHL_ERR_INVALID; }
    for (int a = 0; a < naxes; a++) {
        int64_t prev_end = 0;
        for (int k = 0; k < 3; k++) {
            const int64_t b = ranges[(a * 3 + k) * 2], e = ranges[(a * 3 + k) * 2 + 1];
            if (b < prev_end || e < b || e > lat->M) {
                phl_set_error("phl_set_blur_rows: axis %d range %d = [%lld, %lld) is not ascending / inside [0, %lld)", a, k, (long long)b,
                              (long long)e, (long long)lat->M);
                return PHL_ERR_INVALID;
            }
            prev_end = e;
        }
    }
    for (int a = 0; a < naxes; a++)
        for (int k = 0; k < 3; k++) {
            lat->blur_rows[a][k][0] = (int32_t)ranges[(a * 3 + k) * 2];
            lat->blur_rows[a][k][1] = (int32_t)ranges[(a * 3 + k) * 2 + 1];
        }
    lat->blur_rows_set = 1;
    return PHL_OK;
}

int phl_tile_stats(const phl_lattice *lat, int vd, int64_t out[7])
{
    if (!lat || !out) { phl_set_error("phl_tile_stats: bad arguments"); return PHL_ERR_INVALID; }
    out[0] = lat->P; out[1] = lat->nchunks; out[2] = lat->nv_max; out[3] = lat->S; out[4] = lat->S_multi;
    const phl_operand rows = described_rows(vd);
    const phl_call_plan p = plan_call(lat, vd, 0, rows, rows, &rows);
    out[5] = p.chunk_splat;
    out[6] = p.chunk_slice;
    return PHL_OK;
}

int phl_reserve_ex(phl_lattice *lat, int vd, unsigned reserve_flags)
{
    if (!lat || vd < 0) { phl_set_error("phl_reserve: bad arguments"); return PHL_ERR_INVALID; }
    device_guard g(lat->device);
    // the plan phl_filter will compute for this width and operands as the flags describe them.  (Rows off the 16-byte
    // grid at a multiple of 4 channels cannot be known here: PHL_RESERVE_STRIDED_IO sizes the staging buffers for those
    // as for channel-major views.)
    const phl_operand io = described_rows(vd, (reserve_flags & PHL_RESERVE_STRIDED_IO) != 0);
    const phl_call_plan p = plan_call(lat, vd, (reserve_flags & PHL_RESERVE_EXACT) ? PHL_FILTER_EXACT : 0, io, io);
    // the gather splat (exact mode, or shapes the chunk splat does not take) needs its pixel-sorted lists
    if (!p.chunk_splat) {
        const int rc = phl_ensure_csr(lat, nullptr);
        if (rc) return rc;
    }
    ws_lease w(lat, nullptr);
    w.idle = true;      // sized, carries no work: the next call on any stream takes it
    return w.acquire(p);
}

int phl_reserve(phl_lattice *lat, int vd) { return phl_reserve_ex(lat, vd, 0); }

int phl_splat(phl_lattice *lat, const float *src, int vd, int64_t src_rs, float *vert, unsigned flags, phl_stream st)
{
    if (!lat || vd < 0 || (lat->n > 0 && vd > 0 && (!src || !vert))) { phl_set_error("phl_splat: bad arguments"); return PHL_ERR_INVALID; }
    device_guard g(lat->device);
    const phl_operand rows = {vert, vd, 1};
    const phl_call_plan p = plan_call(lat, vd, flags, {src, src_rs, 1}, {}, &rows);
    if (!p.chunk_splat) return phl_launch_splat(lat, src, src_rs, vd, vert, (hipStream_t)st);
    ws_lease w(lat, (hipStream_t)st);       // only the partial rows come from the workspace here
    const int rc = w.acquire(p);
    return rc ? rc : phl_launch_splat_tiled(lat, src, src_rs, vd, vert, w->partial, (hipStream_t)st);
}

int64_t phl_num_chunks(const phl_lattice *lat) { return lat ? lat->nchunks : -1; }
int64_t phl_partial_rows(const phl_lattice *lat) { return lat ? lat->S_multi : -1; }

int phl_chunks_touching(phl_lattice *lat, const int64_t *rows_dev, int64_t k, int32_t *mask_host, phl_stream st)
{
    if (!lat || k < 0 || (k > 0 && !rows_dev) || !mask_host) { phl_set_error("phl_chunks_touching: bad arguments"); return PHL_ERR_INVALID; }
    device_guard g(lat->device);
    return phl_tiles_chunks_touching(lat, rows_dev, k, mask_host, (hipStream_t)st);
}

// what the two subset entry points share, behind their argument checks
static int splat_subset(const char *who, phl_lattice *lat, const float *src, int vd, int64_t src_rs, float *vert, float *partial_dev,
                        const int32_t *chunks_dev, int64_t nchunks_sel, const int32_t *rows_dev, int64_t nrows,
                        const int32_t *pack_pos_dev, float *pack_dev, int64_t pack_rs, phl_stream st)
{
    device_guard g(lat->device);
    const phl_operand rows = {vert, vd, 1};
    if (!plan_call(lat, vd, 0, {src, src_rs, 1}, {}, &rows).chunk_splat || !phl_al16(partial_dev)) {
        phl_set_error("%s: the chunk splat is not available for this shape (vd %% 4, alignment, sharing)", who);
        return PHL_ERR_UNSUPPORTED;
    }
    phl_splat_opts o;
    o.subset = true;
    o.chunk_list = chunks_dev;
    o.nlist = (int)nchunks_sel;
    o.vlist = rows_dev;
    o.nvl = nrows;
    o.pack_pos = pack_pos_dev;
    o.pack = pack_dev;
    o.pack_rs = pack_rs;
    return phl_launch_splat_tiled(lat, src, src_rs, vd, vert, partial_dev, (hipStream_t)st, o);
}

int phl_splat_part(phl_lattice *lat, const float *src, int vd, int64_t src_rs, float *vert, float *partial_dev,
                   const int32_t *chunks_dev, int64_t nchunks_sel, const int32_t *rows_dev, int64_t nrows, phl_stream st)
{
    if (!lat || vd < 0 || nchunks_sel < 0 || nrows < 0 || !src || !vert || (nchunks_sel > 0 && !chunks_dev) || (nrows > 0 && !rows_dev) ||
        (lat->S_multi > 0 && !partial_dev)) {
        phl_set_error("phl_splat_part: bad arguments");
        return PHL_ERR_INVALID;
    }
    return splat_subset("phl_splat_part", lat, src, vd, src_rs, vert, partial_dev, chunks_dev, nchunks_sel, rows_dev, nrows,
                        /*no row packing*/ nullptr, nullptr, 0, st);
}

int phl_splat_part_pack(phl_lattice *lat, const float *src, int vd, int64_t src_rs, float *vert, float *partial_dev,
                        const int32_t *chunks_dev, int64_t nchunks_sel, const int32_t *rows_dev, int64_t nrows,
                        const int32_t *pack_pos_dev, float *pack_dev, int64_t pack_rs, phl_stream st)
{
    if (!lat || vd < 0 || nchunks_sel < 0 || nrows < 0 || !vert || (nchunks_sel > 0 && (!chunks_dev || !src)) || (nrows > 0 && !rows_dev) ||
        (lat->S_multi > 0 && !partial_dev) || (pack_pos_dev && (!pack_dev || pack_rs < vd || pack_rs % 4 || !phl_al16(pack_dev)))) {
        phl_set_error("phl_splat_part_pack: bad arguments");
        return PHL_ERR_INVALID;
    }
    return splat_subset("phl_splat_part_pack", lat, src, vd, src_rs, vert, partial_dev, chunks_dev, nchunks_sel, rows_dev, nrows,
                        pack_pos_dev, pack_dev, pack_rs, st);
}

int phl_blur_axis(phl_lattice *lat, int axis, const float *vin, float *vout, int vd, phl_stream st)
{
    if (!lat || axis < 0 || axis > lat->d || vd < 0 || vin == vout) { phl_set_error("phl_blur_axis: bad arguments"); return PHL_ERR_INVALID; }
    device_guard g(lat->device);
    return phl_launch_blur(lat, axis, vin, vout, vd, (hipStream_t)st);
}

// all blur axes, two per pass where a pair is left; returns the index (0/1) of the buffer holding the result
static int blur_all(const phl_lattice *lat, float *const buf[2], int vd, hipStream_t st, int *cur_out)
{
    static const bool pairs = !(getenv("PHL_BLUR_PAIRS") && atoi(getenv("PHL_BLUR_PAIRS")) == 0);
    static const bool triples = !(getenv("PHL_BLUR_TRIPLES") && atoi(getenv("PHL_BLUR_TRIPLES")) == 0);
    int cur = 0;
    // Three axes per pass where the lattice has the line lists and a wave owns a row: n3 triples (k_blur3), then the
    // pairs behind them from their own tables -- ceil((d+1)/3) launches, same axis order, same bits.  Row-band
    // lattices and narrow rows take the pair route below.
    if (pairs && triples && phl_blur3_takes(lat, buf[0], buf[1], vd)) {
        for (int slot = 0; slot < lat->np3; slot++) {
            const int rc = slot < lat->n3 ? phl_launch_blur3(lat, slot, buf[cur], buf[cur ^ 1], vd, st)
                                          : phl_launch_blur2_slot(lat, slot, buf[cur], buf[cur ^ 1], vd, st);
            if (rc) return rc;
            cur ^= 1;
        }
        *cur_out = cur;
        return PHL_OK;
    }
    for (int axis = 0; axis <= lat->d;) {  // axis order 0..d, Jacobi ping-pong (:498, :530-532)
        int rc;
        if (pairs && axis + 1 <= lat->d && lat->nbr2) {
            rc = phl_launch_blur2(lat, axis / 2, buf[cur], buf[cur ^ 1], vd, st, /*restricted=*/true);
            axis += 2;
        } else {
            rc = phl_launch_blur(lat, axis, buf[cur], buf[cur ^ 1], vd, st, /*restricted=*/true);
            axis += 1;
        }
        if (rc) return rc;
        cur ^= 1;
    }
    *cur_out = cur;
    return PHL_OK;
}

int phl_blur(phl_lattice *lat, float *vert_a, float *vert_b, int vd, int *result_in_b, phl_stream st)
{
    if (!lat || vd < 0 || !result_in_b || vert_a == vert_b || (lat->M > 0 && vd > 0 && (!vert_a || !vert_b))) {
        phl_set_error("phl_blur: bad arguments");
        return PHL_ERR_INVALID;
    }
    device_guard g(lat->device);
    float *const buf[2] = {vert_a, vert_b};
    return blur_all(lat, buf, vd, (hipStream_t)st, result_in_b);
}

int phl_gather_rows(const float *vert, int vd, const int64_t *idx_dev, int64_t k, float *out, int64_t out_rs, phl_stream st)
{
    if (vd < 0 || k < 0 || (k > 0 && vd > 0 && (!vert || !idx_dev || !out))) { phl_set_error("phl_gather_rows: bad arguments"); return PHL_ERR_INVALID; }
    return phl_launch_rows(false, const_cast<float *>(vert), vd, idx_dev, k, out, out_rs, (hipStream_t)st);
}

int phl_scatter_add_rows(float *vert, int vd, const int64_t *idx_dev, int64_t k, const float *in, int64_t in_rs, phl_stream st)
{
    if (vd < 0 || k < 0 || (k > 0 && vd > 0 && (!vert || !idx_dev || !in))) { phl_set_error("phl_scatter_add_rows: bad arguments"); return PHL_ERR_INVALID; }
    return phl_launch_rows(true, vert, vd, idx_dev, k, const_cast<float *>(in), in_rs, (hipStream_t)st);
}

int phl_slice(phl_lattice *lat, const float *vert, int vd, float *out, int64_t out_rs, const float *sub, int64_t sub_rs,
              unsigned flags, phl_stream st)
{
    if (!lat || vd < 0) { phl_set_error("phl_slice: bad arguments"); return PHL_ERR_INVALID; }
    device_guard g(lat->device);
    // (`sub`, where given, is read whatever the flags say)
    const phl_operand rows = {vert, vd, 1};
    if (plan_call(lat, vd, flags | PHL_FILTER_SUBTRACT_INPUT, {sub, sub ? sub_rs : 0, 1}, {out, out_rs, 1}, &rows).chunk_slice)
        return phl_launch_slice_tiled(lat, vert, vd, out, out_rs, sub, sub_rs, flags, (hipStream_t)st);
    return phl_launch_slice(lat, vert, vd, out, out_rs, sub, sub_rs, flags, (hipStream_t)st);
}

int phl_filter(phl_lattice *lat, const float *src, int vd, int64_t src_rs, int64_t src_cs, float *out, int64_t out_rs,
               int64_t out_cs, unsigned flags, phl_stream stream)
{
    if (!lat || vd < 0) { phl_set_error("phl_filter: bad arguments"); return PHL_ERR_INVALID; }
    const int64_t n = lat->n;
    if (n == 0 || vd == 0) return PHL_OK;
    if (!src || !out) { phl_set_error("phl_filter: NULL src/out"); return PHL_ERR_INVALID; }
    if (src == out) { phl_set_error("phl_filter: out may not alias src"); return PHL_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    device_guard g(lat->device);
    const phl_call_plan p = plan_call(lat, vd, flags, {src, src_rs, src_cs}, {out, out_rs, out_cs});
    ws_lease w(lat, st);
    int rc = w.acquire(p);
    if (rc) return rc;
    // the kernels run at vdw channels on the operands or on their staged copies (at a rounded-up width the extra
    // channels hold whatever the staging buffer held: channels never mix, and they are not copied out)
    const int vdw = p.vdw;
    const float *const src_eff = p.stage_src ? w->stage_in : src;
    float *const out_eff = p.stage_dst ? w->stage_out : out;
    const int64_t src_eff_rs = p.stage_src ? vdw : src_rs, out_eff_rs = p.stage_dst ? vdw : out_rs;
    if (p.stage_src) rc = phl_launch_copy2d(src, src_rs, src_cs, w->stage_in, vdw, 1, n, vd, st);
    if (rc) return rc;
    if (p.chunk_splat) rc = phl_launch_splat_tiled(lat, src_eff, src_eff_rs, vdw, w->buf[0], w->partial, st);
    else rc = phl_launch_splat(lat, src_eff, src_eff_rs, vdw, w->buf[0], st);
    if (rc) return rc;
    int cur = 0;
    rc = blur_all(lat, w->buf, vdw, st, &cur);
    if (rc) return rc;
    const float *sub = (flags & PHL_FILTER_SUBTRACT_INPUT) ? src_eff : nullptr;
    if (p.chunk_slice) rc = phl_launch_slice_tiled(lat, w->buf[cur], vdw, out_eff, out_eff_rs, sub, src_eff_rs, flags, st);
    else rc = phl_launch_slice(lat, w->buf[cur], vdw, out_eff, out_eff_rs, sub, src_eff_rs, flags, st);
    if (rc) return rc;
    if (p.stage_dst) rc = phl_launch_copy2d(w->stage_out, vdw, 1, out, out_rs, out_cs, n, vd, st);
    return rc;
}

int phl_filter_grad(phl_lattice *lat, const float *src, int64_t src_rs, const float *g, int64_t g_rs, int L, const float *ref,
                    int64_t ref_rs, int64_t ref_cs, float *grad_ref, float *grad_src, int64_t grad_src_rs, phl_stream stream)
{
    if (!lat || L < 0 || !grad_ref) { phl_set_error("phl_filter_grad: bad arguments"); return PHL_ERR_INVALID; }
    const int64_t n = lat->n;
    const int d = lat->d;
    if (n == 0) return PHL_OK;
    hipStream_t st = (hipStream_t)stream;
    device_guard guard(lat->device);
    if (L == 0) {       // (before the NULL tests: an [n, 0] tensor has no storage, and nothing of src / g / ref is read)
        PHL_HIP(hipMemsetAsync(grad_ref, 0, sizeof(float) * (size_t)n * d, st));
        return PHL_OK;
    }
    if (!src || !g || !ref) { phl_set_error("phl_filter_grad: NULL src / g / ref"); return PHL_ERR_INVALID; }
    // Feature groups: column k of the result needs only block 0 (W x) and block 1 + k (W(x f_k)) of the wide rows, so the
    // d features are contracted in ceil(d / 7) groups of at most 7 columns, as even as possible (8 -> 4+4, 16 -> 6+5+5),
    // each a wide splat / blur / slice of (group size + 1) blocks.  d <= 7 is one group of all features: the kernels with
    // d + 1 built in.  PHL_GRAD_FEATURES_PER_GROUP (1..7, read per call like PHL_GRAD_WS_MB) caps the group size at any d.
    const char *fg_env = getenv("PHL_GRAD_FEATURES_PER_GROUP");
    const int fg_cap = fg_env && atoi(fg_env) >= 1 && atoi(fg_env) <= 7 ? atoi(fg_env) : 7;
    const int ngroups = d > 0 ? (d + fg_cap - 1) / fg_cap : 1;
    const int nb_max = (d + ngroups - 1) / ngroups + 1;             // blocks of the widest group
    const int64_t vdw = (int64_t)L * nb_max;
    const phl_operand g_rows = {g, g_rs, 1};
    if (d < 1 || d > PHL_FILTER_GRAD_MAX_D || L % 4 != 0 || !plan_call(lat, L, 0, {src, src_rs, 1}, {}, &g_rows).chunk_splat ||
        vdw > (1 << 20) || (grad_src && !phl_rows16(grad_src, grad_src_rs))) {
        phl_set_error("phl_filter_grad: shape not covered by the fused path (d <= %d, L %% 4 == 0, 16-byte aligned pixel-major rows, "
                      "chunk splat available); filter the 2L(1+d)-channel operand instead", PHL_FILTER_GRAD_MAX_D);
        return PHL_ERR_UNSUPPORTED;
    }
    // Workspace: the wide vertex rows (two ping-pong buffers) and the wide partial rows, (2M + S_multi) * nb_max * Lg floats
    // for a group of Lg channels.  The contraction is a sum over channels, so the call runs in CHANNEL GROUPS whenever
    // all L at once would exceed the budget (PHL_GRAD_WS_MB, default 24576): features with little sharing push S_multi
    // towards 2n, and (2M + S_multi)(1+d)L floats would then be as large as the reference's wide operand that this
    // path exists to avoid.  Groups are multiples of 64 channels (the wide splat's slab) where L allows.
    const char *ws_env = getenv("PHL_GRAD_WS_MB");      // (read per call: a backward pass is milliseconds, and tests vary it)
    const int64_t ws_budget = (int64_t)(ws_env && atoll(ws_env) > 0 ? atoll(ws_env) : 24576) << 20;
    const int64_t rows_ws = 2 * lat->M + lat->S_multi;
    int Lg = L;
    if (rows_ws * vdw * (int64_t)sizeof(float) > ws_budget) {
        const int64_t per_ch = rows_ws * nb_max * (int64_t)sizeof(float);
        int64_t fit = ws_budget / (per_ch > 0 ? per_ch : 1);
        fit = fit >= 64 ? fit / 64 * 64 : fit / 4 * 4;
        if (fit < 4) {
            phl_set_error("phl_filter_grad: %lld vertex + partial rows do not fit the workspace budget even four channels at a time "
                          "(PHL_GRAD_WS_MB)", (long long)rows_ws);
            return PHL_ERR_UNSUPPORTED;
        }
        Lg = (int)(fit < L ? fit : L);
    }
    const int64_t vdg = (int64_t)Lg * nb_max;
    ws_lease w(lat, st);
    int rc = w.acquire(lat->M * vdg, lat->S_multi * vdg, 0);
    if (rc) return rc;
    // Two passes of the same three stages per feature group, each over (1+cols) L channels instead of the reference's
    // 2 (1+d) L at once:
    //   pass 1  x = g,   y = src:  T  = -2 sum_l src (f Wg - W(g f))      (+ Wg itself = the gradient w.r.t. src)
    //   pass 2  x = src, y = g:    T += -2 sum_l g   (f Ws - W(s f))
    // Feature groups write disjoint columns of grad_ref, so `accumulate` does not depend on the group; W g is block 0 of
    // every group and is written once, by the first.
    const float *xs[2] = {g, src}, *ys[2] = {src, g};
    const int64_t xrs[2] = {g_rs, src_rs}, yrs[2] = {src_rs, g_rs};
    for (int c0 = 0; c0 < L && rc == PHL_OK; c0 += Lg) {
        const int Lc = L - c0 < Lg ? L - c0 : Lg;
        for (int pass = 0; pass < 2 && rc == PHL_OK; pass++) {
            for (int fg = 0, k0 = 0; fg < ngroups && rc == PHL_OK; fg++) {
                const int cols = d / ngroups + (fg < d % ngroups ? 1 : 0);
                const phl_splat_wide wide = {cols + 1, ref + (int64_t)k0 * ref_cs, ref_rs, ref_cs};
                phl_splat_opts o;
                o.wide = &wide;
                rc = phl_launch_splat_tiled(lat, xs[pass] + c0, xrs[pass], Lc, w->buf[0], w->partial, st, o);
                if (rc) break;
                int cur = 0;
                rc = blur_all(lat, w->buf, Lc * (cols + 1), st, &cur);
                if (rc) break;
                rc = phl_launch_slice_grad(lat, w->buf[cur], Lc, ys[pass] + c0, yrs[pass], ref, ref_rs, ref_cs, grad_ref, k0, cols,
                                           (pass || c0) ? 1 : 0, (pass == 0 && fg == 0 && grad_src) ? grad_src + c0 : nullptr,
                                           grad_src_rs, st);
                k0 += cols;
            }
        }
    }
    return rc;
}

int phl_copy2d(const float *src, int64_t src_rs, int64_t src_cs, float *dst, int64_t dst_rs, int64_t dst_cs, int64_t rows,
               int cols, phl_stream stream)
{
    if (rows < 0 || cols < 0 || (rows > 0 && cols > 0 && (!src || !dst))) { phl_set_error("phl_copy2d: bad arguments"); return PHL_ERR_INVALID; }
    if (rows == 0 || cols == 0) return PHL_OK;
    return phl_launch_copy2d(src, src_rs, src_cs, dst, dst_rs, dst_cs, rows, cols, (hipStream_t)stream);
}

int phl_filter_once(const float *src, int vd, int64_t src_rs, int64_t src_cs, const float *ref, int d, int64_t ref_rs,
                    int64_t ref_cs, int64_t n, float *out, int64_t out_rs, int64_t out_cs, unsigned flags, int device,
                    phl_stream stream)
{
    phl_lattice *lat = nullptr;
    int rc = phl_build_ex(&lat, ref, n, d, ref_rs, ref_cs, device, stream,
                          (flags & PHL_FILTER_CLEAN_TABLE) ? PHL_BUILD_DEFAULT : PHL_BUILD_REFERENCE_TABLE);
    if (rc) return rc;
    rc = phl_filter(lat, src, vd, src_rs, src_cs, out, out_rs, out_cs, flags & ~(unsigned)PHL_FILTER_CLEAN_TABLE, stream);
    if (rc == PHL_OK) {
        device_guard g(device);
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);  // workspace dies with the lattice
        if (e != hipSuccess) rc = phl_hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    }
    phl_destroy(lat);
    return rc;
}

// first-touch <-> internal maps on the host (empty vectors: the numberings coincide)
static int fetch_maps(phl_lattice *lat, std::vector<int32_t> &ft_of_int, std::vector<int32_t> &int_of_ft)
{
    ft_of_int.clear();
    int_of_ft.clear();
    if (!lat->int_of_ft || lat->M == 0) return PHL_OK;
    ft_of_int.resize((size_t)lat->M);
    int_of_ft.resize((size_t)lat->M);
    PHL_HIP(hipMemcpy(ft_of_int.data(), lat->ft_of_int, sizeof(int32_t) * (size_t)lat->M, hipMemcpyDeviceToHost));
    PHL_HIP(hipMemcpy(int_of_ft.data(), lat->int_of_ft, sizeof(int32_t) * (size_t)lat->M, hipMemcpyDeviceToHost));
    return PHL_OK;
}

int phl_get_vertex_order(phl_lattice *lat, int32_t *row_of_vertex)
{
    if (!lat || !row_of_vertex) { phl_set_error("phl_get_vertex_order: bad arguments"); return PHL_ERR_INVALID; }
    device_guard g(lat->device);
    PHL_HIP(hipDeviceSynchronize());
    if (lat->int_of_ft) PHL_HIP(hipMemcpy(row_of_vertex, lat->int_of_ft, sizeof(int32_t) * (size_t)lat->M, hipMemcpyDeviceToHost));
    else
        for (int64_t v = 0; v < lat->M; v++) row_of_vertex[v] = (int32_t)v;
    return PHL_OK;
}

int phl_get_pixel_order(phl_lattice *lat, int32_t *pix_order)
{
    if (!lat || !pix_order) { phl_set_error("phl_get_pixel_order: bad arguments"); return PHL_ERR_INVALID; }
    if (lat->n == 0) return PHL_OK;
    if (!lat->pix_order) { phl_set_error("phl_get_pixel_order: the lattice has no chunks"); return PHL_ERR_UNSUPPORTED; }
    device_guard g(lat->device);
    PHL_HIP(hipDeviceSynchronize());
    PHL_HIP(hipMemcpy(pix_order, lat->pix_order, sizeof(int32_t) * (size_t)lat->n, hipMemcpyDeviceToHost));
    return PHL_OK;
}

int phl_get_keys(phl_lattice *lat, int16_t *keys)
{
    if (!lat || !keys) { phl_set_error("phl_get_keys: bad arguments"); return PHL_ERR_INVALID; }
    if (lat->M == 0) return PHL_OK;
    device_guard g(lat->device);
    PHL_HIP(hipDeviceSynchronize());
    std::vector<int32_t> f, r;
    int rc = fetch_maps(lat, f, r);
    if (rc) return rc;
    const int d = lat->d;
    if (r.empty()) {
        PHL_HIP(hipMemcpy(keys, lat->vkeys, sizeof(int16_t) * (size_t)lat->M * d, hipMemcpyDeviceToHost));
        return PHL_OK;
    }
    std::vector<int16_t> h((size_t)lat->M * d);
    PHL_HIP(hipMemcpy(h.data(), lat->vkeys, sizeof(int16_t) * h.size(), hipMemcpyDeviceToHost));
    for (int64_t v = 0; v < lat->M; v++) memcpy(keys + v * d, h.data() + (size_t)r[v] * d, sizeof(int16_t) * d);
    return PHL_OK;
}

int phl_get_replay(phl_lattice *lat, int32_t *vid, float *w)
{
    if (!lat || !vid || !w) { phl_set_error("phl_get_replay: bad arguments"); return PHL_ERR_INVALID; }
    if (lat->N == 0) return PHL_OK;
    device_guard g(lat->device);
    std::vector<phl_replay_t> h((size_t)lat->N);
    PHL_HIP(hipDeviceSynchronize());
    PHL_HIP(hipMemcpy(h.data(), lat->replay, sizeof(phl_replay_t) * h.size(), hipMemcpyDeviceToHost));
    std::vector<int32_t> f, r;
    int rc = fetch_maps(lat, f, r);
    if (rc) return rc;
    for (size_t i = 0; i < h.size(); i++) { vid[i] = f.empty() ? h[i].vid : f[h[i].vid]; w[i] = h[i].w; }
    return PHL_OK;
}

int phl_get_neighbors(phl_lattice *lat, int32_t *nbr)
{
    if (!lat || !nbr) { phl_set_error("phl_get_neighbors: bad arguments"); return PHL_ERR_INVALID; }
    if (lat->M == 0) return PHL_OK;
    device_guard g(lat->device);
    PHL_HIP(hipDeviceSynchronize());
    std::vector<int32_t> f, r;
    int rc = fetch_maps(lat, f, r);
    if (rc) return rc;
    const size_t M = (size_t)lat->M;
    const int axes = lat->d + 1;
    if (r.empty()) {
        PHL_HIP(hipMemcpy(nbr, lat->nbr, sizeof(int32_t) * M * axes * 2, hipMemcpyDeviceToHost));
        return PHL_OK;
    }
    std::vector<int32_t> h(M * axes * 2);
    PHL_HIP(hipMemcpy(h.data(), lat->nbr, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
    for (int a = 0; a < axes; a++)
        for (size_t v = 0; v < M; v++)
            for (int s2 = 0; s2 < 2; s2++) {
                const int32_t x = h[((size_t)a * M + r[v]) * 2 + s2];
                nbr[((size_t)a * M + v) * 2 + s2] = x < 0 ? x : f[x];
            }
    return PHL_OK;
}

int phl_get_blur_lines(phl_lattice *lat, int group, int32_t *vertex, int32_t *flags, int32_t *item_start, int64_t info[3])
{
    if (!lat || !info) { phl_set_error("phl_get_blur_lines: bad arguments"); return PHL_ERR_INVALID; }
    const bool have = lat->lines && lat->line_items && lat->n3 > 0;
    info[0] = have ? lat->n3 : 0;
    info[1] = have ? lat->nitems3 : 0;
    info[2] = have ? lat->line_item_size : 0;
    if (!vertex && !flags && !item_start) return PHL_OK;
    if (!have || group < 0 || group >= lat->n3 || !vertex || !flags || !item_start) {
        phl_set_error("phl_get_blur_lines: no line list for group %d", group);
        return PHL_ERR_INVALID;
    }
    device_guard g(lat->device);
    PHL_HIP(hipDeviceSynchronize());
    std::vector<int32_t> f, r;
    int rc = fetch_maps(lat, f, r);
    if (rc) return rc;
    const size_t M = (size_t)lat->M;
    std::vector<uint32_t> h(M);
    PHL_HIP(hipMemcpy(h.data(), lat->lines + (size_t)group * M, sizeof(uint32_t) * M, hipMemcpyDeviceToHost));
    PHL_HIP(hipMemcpy(item_start, lat->line_items + (size_t)group * (lat->nitems3 + 1), sizeof(int32_t) * (size_t)(lat->nitems3 + 1),
                      hipMemcpyDeviceToHost));
    for (size_t i = 0; i < M; i++) {
        const uint32_t row = h[i] & PHL_LINE_VERTEX;
        vertex[i] = (f.empty() || row >= M) ? (int32_t)row : f[row];
        flags[i] = (int32_t)(h[i] >> 28);
    }
    return PHL_OK;
}

int phl_get_splat_lists(phl_lattice *lat, int32_t *ptr, int32_t *pixel, float *w)
{
    if (!lat || !ptr || !pixel || !w) { phl_set_error("phl_get_splat_lists: bad arguments"); return PHL_ERR_INVALID; }
    if (lat->N == 0) { ptr[0] = 0; return PHL_OK; }
    device_guard g(lat->device);
    const int rc0 = phl_ensure_csr(lat, nullptr);
    if (rc0) return rc0;
    std::vector<phl_contrib_t> h((size_t)lat->N);
    std::vector<int32_t> p((size_t)lat->M + 1);
    PHL_HIP(hipDeviceSynchronize());
    PHL_HIP(hipMemcpy(p.data(), lat->csr_ptr, sizeof(int32_t) * p.size(), hipMemcpyDeviceToHost));
    PHL_HIP(hipMemcpy(h.data(), lat->csr, sizeof(phl_contrib_t) * h.size(), hipMemcpyDeviceToHost));
    std::vector<int32_t> f, r;
    int rc = fetch_maps(lat, f, r);
    if (rc) return rc;
    int64_t o = 0;
    for (int64_t v = 0; v < lat->M; v++) {          // lists in first-touch vertex order
        const int64_t row = r.empty() ? v : r[v];
        ptr[v] = (int32_t)o;
        for (int32_t e = p[row]; e < p[row + 1]; e++, o++) { pixel[o] = h[e].pixel; w[o] = h[e].w; }
    }
    ptr[lat->M] = (int32_t)o;
    return PHL_OK;
}

}  // extern "C"
