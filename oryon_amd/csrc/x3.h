// The fp16x3 scheme's shared pieces, one definition each: an fp32 operand is split x = hi + lo (hi = half(x), lo = half(x - hi): 22
// significant bits together) and a product is accumulated in fp32 as lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_f16; the dropped
// lo*lo term is ~2^-22 |a||b|, the size of fp32's own accumulation error.  Used by the towers' linears (gemm_x3.hip), the CLIP attention
// (attention_x3.hip), both window attentions (backbone_ops.hip), the decoder's convolutions (decoder.hip) and the PointDSC encoder
// (pdsc_blocks.h, pdsc_encoder.hip, the weight images of pointdsc.hip).  A change to the split or to its range rule is made here.
// Range: magnitudes must stay below 65504 (fp16 range) or the split overflows to inf (common.h: the range flag).  Precision: an operand
// below 2^-3 has its low half in float16's subnormal range (absolute split error <= 2^-25 instead of the relative 2^-22).
#pragma once
#include "common.h"

namespace oryon {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));      // an A or B fragment of v_mfma_f32_32x32x16_f16
typedef float f32x16 __attribute__((ext_vector_type(16)));       // its 32x32 accumulator block
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// row of a 32x32 accumulator block held by register r in lane half hi (the column is lane & 31)
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__host__ __device__ __forceinline__ void split1(float x, _Float16 &hi, _Float16 &lo)
{
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// Two values at a time, the same bits as split1 (tools/probe_cvt_pk_f16.hip): packed conversions (v_cvt_pk_f16_f32 on gfx950,
// round-to-nearest-even) and the residuals x - float(hi) as one v_fma_mix_f32 each (hi's half read as the f16 source of an fp32 fma:
// float(hi) * -1 + x, one rounding of an exactly representable difference - the bits of the subtraction it replaces): four
// instructions per pair instead of six.  VALU and MFMA do not overlap on this part, so the split is wave time.
__device__ __forceinline__ void split2(float x, float y, unsigned &hi, unsigned &lo)
{
    const f32x2 a = {x, y};
    const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector(a, f16x2));
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hb), "v"(x));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hb), "v"(y));
    const f32x2 lv = {l0, l1};
    hi = hb;
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(lv, f16x2));
}
__device__ __forceinline__ void split4(const float4 v, uint2 &hi, uint2 &lo)
{
    split2(v.x, v.y, hi.x, lo.x);
    split2(v.z, v.w, hi.y, lo.y);
}
// eight values as scalar splits (the window attentions; not the packed form: that would be a change with its own measurement)
__device__ __forceinline__ void split8(const float (&x)[8], f16x8 &hi, f16x8 &lo)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        _Float16 h, l;
        split1(x[e], h, l);
        hi[e] = h;
        lo[e] = l;
    }
}

// The three products on one accumulator, smallest terms first.  Only for kernels that issue them together in this order: the stream
// linear, the CLIP attention and the encoder kernels issue term-major or between sched_barriers, which is part of what was measured.
__device__ __forceinline__ void mfma_x3(f32x16 &acc, const f16x8 ah, const f16x8 al, const f16x8 bh, const f16x8 bl)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

}  // namespace oryon
