// rt_wave.h -- the bottom of the device library: the constant-address-space pointer types, V3, and the wave64
// helpers (DPP reductions, lane masks and votes, the wave-local LDS fence). Included by rt_exact.h, and through it
// by every unit that holds device code of the tracer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device.h"

namespace {

// RtFrameAux is read through the CONSTANT address space: the memory does not change while a
// kernel runs, and a load from a wave-uniform address there is a scalar load (s_load into
// SGPRs) wherever it stands -- as a plain global pointer the compiler has to assume the
// kernel's own stores may alias it and uses per-lane vector loads into VGPRs.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const RtFrameAux __attribute__((address_space(4))) *AuxPtr;
typedef const RtFrameConsts __attribute__((address_space(4))) *FcPtr;
typedef const int __attribute__((address_space(4))) *ConstIntPtr;
#else
typedef const int *ConstIntPtr;
typedef const RtFrameAux *AuxPtr;   // host pass over this translation unit (device functions are only parsed there)
typedef const RtFrameConsts *FcPtr;
#endif

struct V3 {
    float x, y, z;
};

// ---------------------------------------------------------------------------
// wave64 helpers
// ---------------------------------------------------------------------------
// Wave-wide reductions on the VALU's DPP path (no LDS round trips): butterfly
// inside each row of 16 lanes, then row_bcast:15 / row_bcast:31 carry the row
// results upward so that lane 63 holds the reduction, which is broadcast back
// through an SGPR (only lane 63 is meaningful after the broadcast steps, which run on all
// rows: lanes without a source get `old`). All 64 lanes must be active (callers are in
// uniform control flow). `old` is the operation's identity, so that the compiler folds each
// move into the operation (one v_max_u32_dpp / v_add_f32_dpp per step, nothing to canonicalise).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_move0(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
// max over the wave of NON-NEGATIVE floats, compared as unsigned integers (same order);
// a NaN compares above +inf and therefore survives into the result.
__device__ __forceinline__ float wave_max(float f)
{
    unsigned v = __builtin_bit_cast(unsigned, f);
#define RT_STEP(CTRL, MASK) { const unsigned m = (unsigned)dpp_move0<CTRL, MASK>((int)v); v = v > m ? v : m; }
    RT_STEP(0xB1, 0xf)    /* quad_perm [1,0,3,2]  */
    RT_STEP(0x4E, 0xf)    /* quad_perm [2,3,0,1]  */
    RT_STEP(0x141, 0xf)   /* row_half_mirror      */
    RT_STEP(0x140, 0xf)   /* row_mirror           */
    RT_STEP(0x142, 0xf)   /* row_bcast:15 -> rows 1,3 */
    RT_STEP(0x143, 0xf)   /* row_bcast:31 -> rows 2,3 */
#undef RT_STEP
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)v, 63));
}
__device__ __forceinline__ float wave_sum(float v)
{
#define RT_STEP(CTRL, MASK) v = v + __builtin_bit_cast(float, dpp_move0<CTRL, MASK>(__builtin_bit_cast(int, v)));
    RT_STEP(0xB1, 0xf) RT_STEP(0x4E, 0xf) RT_STEP(0x141, 0xf) RT_STEP(0x140, 0xf) RT_STEP(0x142, 0xf) RT_STEP(0x143, 0xf)
#undef RT_STEP
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// three sums at once, their steps interleaved (a DPP read needs two wait states after the
// write of its source: with three chains in flight no s_nop is needed)
__device__ __forceinline__ void wave_sum3(float &a, float &b, float &c)
{
#define RT_STEP(CTRL, MASK)                                                                    \
    {                                                                                          \
        const float ta = __builtin_bit_cast(float, dpp_move0<CTRL, MASK>(__builtin_bit_cast(int, a))); \
        const float tb = __builtin_bit_cast(float, dpp_move0<CTRL, MASK>(__builtin_bit_cast(int, b))); \
        const float tc = __builtin_bit_cast(float, dpp_move0<CTRL, MASK>(__builtin_bit_cast(int, c))); \
        a = a + ta; b = b + tb; c = c + tc;                                                    \
    }
    RT_STEP(0xB1, 0xf) RT_STEP(0x4E, 0xf) RT_STEP(0x141, 0xf) RT_STEP(0x140, 0xf) RT_STEP(0x142, 0xf) RT_STEP(0x143, 0xf)
#undef RT_STEP
    a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a), 63));
    b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b), 63));
    c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), 63));
}
// Votes on `bool` (an i1 for the compiler: the compare's own lane mask). HIP's __ballot / __any / __all take an `int`:
// any predicate that is more than a single compare is first made a 0/1 vector register and compared against zero
// again -- two instructions of the slow issue class per vote, and the frame kernel votes a hundred times per tile.
// Cheaper still where it is hot: LM(one comparison) is that compare's own result register, masks combine with scalar
// and/or/andn2, and lane_in(mask) hands a wave-uniform mask back to the lanes as a condition (selects and branches take
// it as it is). The compiler lowers a ballot of anything BUT a single compare -- `a & b`, a flag carried round a loop --
// through a 0/1 vector register (v_cndmask + v_cmp_ne, both of the half-rate issue class): thirty such pairs per tile.
typedef unsigned long long lmask;
#define LM(compare) __builtin_amdgcn_ballot_w64(compare)
__device__ __forceinline__ bool lane_in(lmask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool any64(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
__device__ __forceinline__ bool all64(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }   // (inactive lanes vote 0)
__device__ __forceinline__ float uniform(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ int lane_prefix(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}
// Lanes of one wave exchange data through LDS without a workgroup barrier.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
