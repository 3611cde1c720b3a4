// Device helpers shared by the fused compatibility + softmax kernels (phl_meanfield.hip: k_compat_softmax,
// k_compat_split; phl_compat_wide.hip: k_compat_wide).  Internal: everything sits in an anonymous namespace, so each
// translation unit gets its own copy, exactly as when the helpers were local to phl_meanfield.hip.
#pragma once
#include <type_traits>

#include "phl_internal.h"

namespace {

// 16 bytes global -> LDS without a register in between (global_load_lds_dwordx4): the LDS address is wave-uniform (M0)
// plus lane*16, the global address is scalar base (SGPR pair) + 32-bit per-lane byte offset.
// The DMA is issued through inline assembly, NOT __builtin_amdgcn_global_load_lds: with the builtin the compiler
// knows an LDS write is in flight, cannot tell it from the buffer the ds_reads use, and puts `s_waitcnt vmcnt(0)`
// in front of the first ds_read after every prefetch.  The kernels' own protocol makes that wait unnecessary (a
// buffer is only read behind the barrier that follows the counted wait for its DMA).
__device__ __forceinline__ void glds16(const float *sbase, unsigned voff, unsigned lds_addr)
{
    unsigned keep;                              // m0 is the compiler's: hand it back as found
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_addr));
}
__device__ __forceinline__ void dma_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// VALU helpers of the epilogues.  f32 MFMAs and ordinary VALU instructions do NOT overlap on gfx950
// (tools/mfma_probe.hip: every v_fma slipped between two MFMAs costs its own issue time plus a ~10-cycle bubble,
// SQ_VALU_MFMA_COEXEC_CYCLES reads 0), so every epilogue instruction is paid for in matrix-pipe time: minima
// three at a time and without the compiler's NaN canonicalisation (v_max x,x before every v_min), the one
// cross-lane step as a lane-half swap instead of a ds_bpermute round trip.  (The swap is inline assembly because
// __builtin_amdgcn_permlane16/32_swap hands back its FIRST result twice in this compiler -- ROCm 7.2, checked with
// tools/dpp_probe.hip.)
__device__ __forceinline__ float vmin3(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// v_permlane32_swap_b32 a, b: the upper 32 lanes of a trade places with the lower 32 lanes of b (checked on the GPU:
// with a = b = x on entry, a holds x[lane & 31] and b holds x[32 + (lane & 31)] in every lane afterwards)
#define PHL_HALF_SWAP(a, b) asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b))
// v_permlane16_swap_b32 a, b: the odd 16-lane rows of a trade places with the even rows of b
#define PHL_ROW_SWAP(a, b) asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b))

// compile-time loop: f(integral_constant<int, I>) for I = 0 .. N-1 (slot-dependent wait counts must be immediates)
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>());
        static_for<N, I + 1>(f);
    }
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// two f32 -> the packed bf16 pairs of their three addends (truncation: top 8 significant bits, the next 8, the last 8)
__device__ __forceinline__ void split3(float x0, float x1, unsigned &h, unsigned &m, unsigned &l)
{
    const unsigned b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
    const float r0 = x0 - __uint_as_float(b0 & 0xFFFF0000u), r1 = x1 - __uint_as_float(b1 & 0xFFFF0000u);
    const unsigned c0 = __float_as_uint(r0), c1 = __float_as_uint(r1);
    const float s0 = r0 - __uint_as_float(c0 & 0xFFFF0000u), s1 = r1 - __uint_as_float(c1 & 0xFFFF0000u);
    h = __builtin_amdgcn_perm(b1, b0, 0x07060302u);        // {hi16(x1), hi16(x0)}
    m = __builtin_amdgcn_perm(c1, c0, 0x07060302u);
    l = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
}

}  // namespace
