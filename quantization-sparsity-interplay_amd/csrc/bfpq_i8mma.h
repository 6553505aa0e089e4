// bfpq_i8mma.h -- the int8 block product that bfpq_i8gemm.hip, bfpq_bmm.hip and bfpq_sp24.hip share: one HBFP block of both operands
// (int8 codes, one int8 exponent per block of 64, 32 or 16, mantissa widths xm, wm in 1..7) -> its term of the fp32 accumulators.
//
// Arithmetic: inside a block the dot product is an exact integer sum on the int8 matrix unit (v_mfma_i32_16x16x64_i8, K = 64 = one
// block, or v_mfma_i32_16x16x32_i8 for a block of 32 or 16; |sum| <= 64 * 127^2 < 2^20), multiplied once by 2^(ex - xm) * 2^(ew - wm)
// and added to fp32 accumulators in block order.
//
// The rescale is the VALU cost a block-scaled instruction does not have.  It is kept to two packed fp32 ops per pair of outputs:
//   - the MFMA's C operand is the integer 0x4B400000 (the bits of 1.5 * 2^23), so its int32 result, read as a float, is exactly
//     1.5 * 2^23 + sum (floats in [2^23, 2^24) step by 1): no int -> float conversion;
//   - u = fma(f, sx, -1.5 * 2^23 * sx) = sum * 2^(ex - xm) (exact: both products are exact, the difference is an integer < 2^20 times
//     a power of two);
//   - acc = fma(u, sw, acc), with sw = 2^(ew - wm).
// Both are v_pk_fma_f32 on two outputs; one 16x16 MFMA leaves 4 outputs per lane, i.e. 4 packed ops.  A block exponent of -128 (the NaN
// block marker) makes its scale NaN, so the block contributes NaN.  (Scales are exact powers of two down to fp32's subnormal 2^-149;
// products below that flush, as the fp32 product of the fake-quantised values would.)
//
// Lane map of v_mfma_i32_16x16x64_i8: A lane l = row l & 15, bytes k = 16 (l >> 4) .. +15; B lane l = column l & 15, same k; D lane l
// holds rows 4 (l >> 4) + j (j = 0..3) of column l & 15.  A = weight rows, B = tokens, so a lane's four results are four consecutive
// output features of one token (one 8- or 16-byte store: store4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "bfpq.h"
#include "bfpq_common.h"

namespace bfpq {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int MAGIC_I = 0x4B400000;                       // bits of 1.5 * 2^23: the MFMA's C operand
constexpr float MAGIC_F = 12582912.0f;

__device__ __forceinline__ float pow2_scale(int e, int m)    // 2^(e - m); NaN for the NaN block marker
{
    return e == -128 ? __builtin_nanf("") : ldexpf(1.0f, e - m);
}

// What depends on the block: the lane's operand (its first byte of the block), whether the weight operand is live, and the instruction.
// Block 64: 16 bytes k = 16 (l >> 4) .. +15 of v_mfma_i32_16x16x64_i8.  Blocks 32 / 16: v_mfma_i32_16x16x32_i8, whose A lane l = row
// l & 15, bytes k = 8 (l >> 4) .. +7 (B: column l & 15, same k; D as for 16x16x64, so the store and the rescale are shared).  Block 32
// fills all 32 k; block 16 puts its 16 bytes in lanes l >> 4 = 0, 1 and zeros in the A operand of lanes 2, 3 (the only K = 16 int8 shape,
// 32x32x16, gives 16 outputs per lane to rescale: the same VALU work per output, which is what bounds these blocks).  Only the pairing of
// A and B bytes matters inside a block (the sum is exact), so a lane's 8 bytes are just its share of the block.
template <int BLK> struct I8Blk {
    static_assert(BLK == 16 || BLK == 32 || BLK == 64, "blocks of 16, 32 or 64");
    using op_t = std::conditional_t<BLK == 64, v4i, long>;
    __device__ __forceinline__ static int lane(int q) { return BLK == 64 ? 16 * q : 8 * (BLK == 32 ? q : (q & 1)); }
    __device__ __forceinline__ static bool a_live(int q) { return BLK != 16 || q < 2; }
    __device__ __forceinline__ static v4i mfma(op_t a, op_t b, v4i c)
    {
        if constexpr (BLK == 64) return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0);
    }
};

// four exponent bytes p[0..3] as a dword (byte i = p[i]): one load where the caller knows p is 4-byte aligned (dw), else byte by byte,
// the bytes from `left` on (past the row's end) reading as 0
__device__ __forceinline__ uint32_t exp4(const int8_t* __restrict__ e, uint32_t off, int left, bool dw)
{
    if (dw) return *reinterpret_cast<const uint32_t*>(e + off);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (i < left) v |= (uint32_t)(uint8_t)e[off + i] << (8 * i);
    return v;
}

__device__ __forceinline__ int exp_byte(uint32_t d, int sh) { return (int)(int8_t)(d >> sh); }      // the byte at bit sh = 8 i of an exp4 dword

// the token side of the rescale from its block exponent: sx = 2^(e - m) on both outputs of a pair, nm = -1.5 * 2^23 * sx
__device__ __forceinline__ void token_scale(int e, int m, v2f& sx, v2f& nm)
{
    const float s = pow2_scale(e, m);
    sx = v2f{s, s};
    nm = v2f{-MAGIC_F * s, -MAGIC_F * s};
}

// the weight side: sw01 / sw23 = 2^(e - m) of the lane's features 0, 1 / 2, 3 from their block exponents, or from the four bytes of an
// exp4 dword
__device__ __forceinline__ void weight_scales(int e0, int e1, int e2, int e3, int m, v2f& sw01, v2f& sw23)
{
    sw01 = v2f{pow2_scale(e0, m), pow2_scale(e1, m)};
    sw23 = v2f{pow2_scale(e2, m), pow2_scale(e3, m)};
}
__device__ __forceinline__ void weight_scales(uint32_t ew, int m, v2f& sw01, v2f& sw23)
{
    weight_scales(exp_byte(ew, 0), exp_byte(ew, 8), exp_byte(ew, 16), exp_byte(ew, 24), m, sw01, sw23);
}

// a01, a23 += (d - 1.5 * 2^23) * sx * sw for the MFMA result d (C = MAGIC_I): sw01 / sw23 the weight scales of the lane's features 0, 1 / 2, 3
__device__ __forceinline__ void rescale(v4i d, v2f sx, v2f nm, v2f sw01, v2f sw23, v2f& a01, v2f& a23)
{
    const v4f f = __builtin_bit_cast(v4f, d);
    const v2f f01 = f.xy, f23 = f.zw;
    const v2f u01 = __builtin_elementwise_fma(f01, sx, nm);
    const v2f u23 = __builtin_elementwise_fma(f23, sx, nm);
    a01 = __builtin_elementwise_fma(u01, sw01, a01);
    a23 = __builtin_elementwise_fma(u23, sw23, a23);
}

// a lane's four consecutive output features to out[o .. o + 3] (o % 4 == 0), rounded to OUT_DT: one 16- or 8-byte store.  An fp32 slab
// of partial sums is the BFPQ_F32 form.  (The tile kernel's biased store stays in bfpq_i8gemm.hip: see I8Tile::store.)
template <int OUT_DT>
__device__ __forceinline__ void store4(void* out, size_t o, v2f a01, v2f a23)
{
    if constexpr (OUT_DT == BFPQ_F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + o) = make_float4(a01.x, a01.y, a23.x, a23.y);
    } else {
        const uint32_t lo = f32_to_raw<OUT_DT>(a01.x) | (f32_to_raw<OUT_DT>(a01.y) << 16);
        const uint32_t hi = f32_to_raw<OUT_DT>(a23.x) | (f32_to_raw<OUT_DT>(a23.y) << 16);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + o) = make_uint2(lo, hi);
    }
}

// the int8 codes of NE elements (raw bits of the dtype) under their block's scale, four to a word in element order: quant_elem for the
// first n, zero codes for the rest
template <int DT, int NE>
__device__ __forceinline__ void pack_codes(const uint32_t (&raw)[NE], int n, const BlockScale& bs, uint32_t (&pk)[NE / 4])
{
#pragma unroll
    for (int e = 0; e < NE / 4; e++) pk[e] = 0u;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        float c = 0.f;
        if (e < n) quant_elem<DT>(raw_to_f32<DT>(raw[e]), bs, false, 0.f, &c);
        pk[e >> 2] |= ((uint32_t)(int)c & 0xffu) << (8 * (e & 3));
    }
}

// 8 two's-complement nibbles (value j in nibble j: element 2 k in the low nibble of byte k, 2 k + 1 in its high one) -> 8 int8 bytes in
// order (the A operand).  Shared by the 2:4 kernels and the 4-bit KV cache
__device__ __forceinline__ v2i nibbles_to_i8(uint32_t w)
{
    // per byte: n -> ((n ^ 8) + 0x78) ^ 0x80 is n sign-extended (no carry leaves the byte: (n ^ 8) + 0x78 <= 0x87)
    const uint32_t lo = (((w & 0x0f0f0f0fu) ^ 0x08080808u) + 0x78787878u) ^ 0x80808080u;          // values 0, 2, 4, 6
    const uint32_t hi = ((((w >> 4) & 0x0f0f0f0fu) ^ 0x08080808u) + 0x78787878u) ^ 0x80808080u;   // values 1, 3, 5, 7
    return v2i{(int)__builtin_amdgcn_perm(hi, lo, 0x05010400u), (int)__builtin_amdgcn_perm(hi, lo, 0x07030602u)};
}

// ... and back: 8 int8 codes in -8..7, four to a word in order (pack_codes), as one word of nibbles.  The even elements' bytes go side
// by side into one word and the odd ones' into another; the low nibble of every byte comes from the first, the high one from the second
__device__ __forceinline__ uint32_t i8_to_nibbles(uint32_t c0123, uint32_t c4567)
{
    const uint32_t ev = __builtin_amdgcn_perm(c4567, c0123, 0x06040200u), od = __builtin_amdgcn_perm(c4567, c0123, 0x07050301u);
    return (ev & 0x0f0f0f0fu) | ((od << 4) & 0xf0f0f0f0u);
}

// host side: f(std::integral_constant<int, BLK>{}) for a block of 16, 32 or 64, and the argument checks of the entries
template <class F> void with_block(int block_size, F&& f)
{
    if (block_size == 32) f(std::integral_constant<int, 32>{});
    else if (block_size == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 64>{});
}
inline bool i8_block_ok(int block_size) { return block_size == 16 || block_size == 32 || block_size == 64; }
inline bool i8_mant_ok(int mant_bits) { return mant_bits >= 1 && mant_bits <= 7; }

}  // namespace bfpq
