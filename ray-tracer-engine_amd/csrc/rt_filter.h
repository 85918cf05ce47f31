// rt_filter.h -- what the image passes share (the a-trous denoisers of rt_denoise.hip, the temporal accumulation of
// rt_temporal.hip): luminance, the packed framebuffer's colour, the floor under a divisor. One copy, so that the
// passes agree to the bit on what they hand one another. Device only; + - * and compares.
#pragma once
#include <stdint.h>

namespace {

constexpr float IM_TINY = 0.0009765625f;   // 2^-10: the floor under an albedo, a depth or a luminance that divides

__device__ __forceinline__ float im_max(float a, float b) { return a > b ? a : b; }   // a NaN `a` gives b
__device__ __forceinline__ float im_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// float -> int as the frame kernel's f2i (v_cvt_i32_f32: truncation, NaN -> 0, saturating) and rgbToInt (kernel.cu:547-556)
__device__ __forceinline__ uint32_t im_pack_colour(float r, float g, float b)
{
    int ir = (int)(r * 254.f), ig = (int)(g * 254.f), ib = (int)(b * 254.f);
    if (ir > 255) ir = 255;
    if (ig > 255) ig = 255;
    if (ib > 255) ib = 255;
    return (uint32_t)(((ir & 0xff) << 16) + ((ig & 0xff) << 8) + (ib & 0xff));
}

}   // namespace
