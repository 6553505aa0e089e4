// bfpq_sp24.hip -- 2:4-compressed packed HBFP weights (format sp24) and their few-token consumer on the sparse int8 matrix instruction:
// out[t][n] = sum_k x[t][k] W[n][k] (+ bias[n]), W held as the two kept codes of every group of 4 along K (N:M pruning with M = 4,
// N <= 2) + their 2-bit positions + the [N, K/64] int8 block exponents of the dense packed weight.  Replaces F.linear on the two
// fake-quantised operands (bfp_ops.py:187-190) for a weight pruned by _structured_N_M_sparsity (bfp_ops.py:73-91).
//
// v_smfmac_i32_16x16x64_i8 (lane maps measured by tools_dev/smfmacprobe):
//   A (sparse, 16 rows x 64 K): lane l = row l & 15, K 16 (l >> 4) .. +15 = 4 groups of 4, compressed to 8 int8 values (2 dwords),
//     value j belongs to group j >> 1; its position in the group is the 2-bit field j of the index half-word (bits 2j, 2j + 1);
//     abid 0 reads the low half-word of the index VGPR, abid 1 the high one.  Positions of a group: two distinct, ascending.
//   B (dense, 64 K x 16 columns): lane l = column l & 15, bytes k = 16 (l >> 4) .. +15, as v_mfma_i32_16x16x64_i8.
//   D: lane l holds rows 4 (l >> 4) + j (j = 0..3) of column l & 15, as v_mfma_i32_16x16x64_i8.
// K = 64 is one HBFP block, so every block's dot product is one instruction and an exact integer sum (|sum| <= 32 * 127^2 < 2^20);
// the rescale is that of bfpq_i8mma.h (C operand 0x4B400000, two packed fp32 FMAs per pair of outputs, exponent -128 -> NaN).
//
// Layout (tiles of 16 rows; lane l = r + 16 q of tile rt holds row 16 rt + r, K 64 b + 16 q .. +15 of block b):
//   per lane and block U bytes of values (4-bit codes: 8 nibbles, value j in nibble j, low first, U = 4; 8-bit codes: 8 bytes,
//   U = 8) and 2 bytes of positions (value j in bits 2j, 2j + 1).  Each array is tile-major; inside a tile the blocks go in chunks of
//   CH = 16 / U blocks (values) or 8 blocks (positions), and inside a chunk lane-major: lane l's bytes of the chunk are contiguous, so
//   one 16-byte load per lane fetches several blocks and a wave's load is 1 KiB in one piece.  The last chunk of a row of tiles holds
//   the remaining nb % CH blocks (nb = K / 64) with the lane stride shrunk to match: no padding, exactly 0.25 (4-bit) or 0.5 (8-bit)
//   + 0.125 B per weight, + 1/64 for the exponents.  sp24_off() is the one formula.
//
// Kernels:
//   k_sp24_pack<CB>    dense codes (as bfpq_quantize_nm writes them) -> values + positions; a group with more than 2 non-zero codes
//                      sets the status word.  A group with fewer keeps the lowest free positions with zero values.
//   k_sp24_unpack<CB>  the exact inverse, to codes of the same width and / or int8 codes.
//   k_sp24_decode<CB>  few tokens: a wave owns 16 output features x up to 16 tokens (token group blockIdx.y) x a slice of K in groups of
//                      8 blocks; per group one 16-byte load of positions, 2 (4-bit) or 4 (8-bit) of values; one instruction per block;
//                      fp32 slabs [slice][T][N] added in slice order by k_slab_reduce (bfpq_common.h), which also adds the bias.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfpq.h"
#include "bfpq_common.h"
#include "bfpq_i8mma.h"

using namespace bfpq;

namespace {

constexpr int IDX_CH = 8;                                 // blocks per 16-byte chunk of positions (2 bytes per lane and block)
constexpr int GROUP = 8;                                  // blocks per step of the decode kernel (one chunk of positions)

template <int CB> struct Sp {
    static constexpr int U = CB == 4 ? 4 : 8;             // value bytes per lane and block
    static constexpr int CH = 16 / U;                     // blocks per 16-byte chunk of values
};

// byte offset of lane l's share of block b, in an array of tiles of nb blocks with U bytes per lane and block, chunks of CH blocks
__device__ __forceinline__ size_t sp24_off(int rt, int nb, int b, int l, int CH, int U)
{
    const int c0 = b - b % CH, nbc = nb - c0 < CH ? nb - c0 : CH;
    return ((size_t)rt * nb + c0) * (size_t)(U * 64) + (size_t)l * (nbc * U) + (size_t)(b - c0) * U;
}

// one group of 4 codes (c[0..3]) -> the two kept positions p0 < p1 (bfpq_int.hip's compact_group rule); *bad when more than 2 are non-zero
__device__ __forceinline__ void keep2(const int (&c)[4], int& p0, int& p1, uint32_t& bad)
{
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) nz |= (uint32_t)(c[i] != 0) << i;
    const int cnt = __builtin_popcount(nz);
    if (cnt > 2) bad = 1u;
    if (cnt >= 2) { p0 = __builtin_ctz(nz); p1 = __builtin_ctz(nz & (nz - 1u)); }
    else if (cnt == 1) { const int p = __builtin_ctz(nz), o = p == 0 ? 1 : 0; p0 = p < o ? p : o; p1 = p < o ? o : p; }
    else { p0 = 0; p1 = 1; }
}

// one thread = one lane's share of one block: 16 codes -> 8 values + 16 position bits
template <int CB>
__global__ void __launch_bounds__(256) k_sp24_pack(const uint8_t* __restrict__ codes, uint8_t* __restrict__ vals, uint8_t* __restrict__ idx,
                                                   int N, int K, int32_t* __restrict__ status)
{
    constexpr int U = Sp<CB>::U, CH = Sp<CB>::CH;
    const int nb = K / 64;
    const int64_t items = (int64_t)(N / 16) * nb * 64;
    uint32_t bad = 0;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int l = (int)(it & 63), b = (int)((it >> 6) % nb), rt = (int)((it >> 6) / nb);
        const int n = rt * 16 + (l & 15), k0 = 64 * b + 16 * (l >> 4);
        int c[16];
        if constexpr (CB == 4) {
            const uint2 w = *reinterpret_cast<const uint2*>(codes + (size_t)n * (K / 2) + k0 / 2);
#pragma unroll
            for (int i = 0; i < 16; i++) c[i] = (int)(((i < 8 ? w.x : w.y) >> (4 * (i & 7))) & 15u);      // (zero test only: raw nibbles)
        } else {
            const uint4 w = *reinterpret_cast<const uint4*>(codes + (size_t)n * K + k0);
            const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 16; i++) c[i] = (int)((wd[i >> 2] >> (8 * (i & 3))) & 255u);
        }
        uint32_t v0 = 0, v1 = 0, ix = 0;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int grp[4] = {c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
            int p0, p1;
            keep2(grp, p0, p1, bad);
            const uint32_t a = (uint32_t)grp[p0], bb = (uint32_t)grp[p1];
            ix |= (uint32_t)(p0 | (p1 << 2)) << (4 * g);
            if constexpr (CB == 4) v0 |= (a | (bb << 4)) << (8 * g);
            else if (g < 2) v0 |= (a | (bb << 8)) << (16 * g);
            else v1 |= (a | (bb << 8)) << (16 * (g - 2));
        }
        uint8_t* vp = vals + sp24_off(rt, nb, b, l, CH, U);
        if constexpr (CB == 4) *reinterpret_cast<uint32_t*>(vp) = v0;
        else *reinterpret_cast<uint2*>(vp) = make_uint2(v0, v1);
        *reinterpret_cast<uint16_t*>(idx + sp24_off(rt, nb, b, l, IDX_CH, 2)) = (uint16_t)ix;
    }
    if (bad) atomicOr(reinterpret_cast<unsigned int*>(status), 1u);
}

// the inverse: codes of width CB (nullable) and / or int8 codes (nullable)
template <int CB>
__global__ void __launch_bounds__(256) k_sp24_unpack(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ idx, uint8_t* __restrict__ codes,
                                                     int8_t* __restrict__ codes8, int N, int K)
{
    constexpr int U = Sp<CB>::U, CH = Sp<CB>::CH;
    const int nb = K / 64;
    const int64_t items = (int64_t)(N / 16) * nb * 64;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int l = (int)(it & 63), b = (int)((it >> 6) % nb), rt = (int)((it >> 6) / nb);
        const int n = rt * 16 + (l & 15), k0 = 64 * b + 16 * (l >> 4);
        const uint8_t* vp = vals + sp24_off(rt, nb, b, l, CH, U);
        uint32_t v[8];
        if constexpr (CB == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(vp);
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = (w >> (4 * j)) & 15u;
        } else {
            const uint2 w = *reinterpret_cast<const uint2*>(vp);
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = ((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 255u;
        }
        const uint32_t ix = *reinterpret_cast<const uint16_t*>(idx + sp24_off(rt, nb, b, l, IDX_CH, 2));
        uint32_t c[16];
#pragma unroll
        for (int i = 0; i < 16; i++) c[i] = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int pos = (int)((ix >> (2 * j)) & 3u), g = j >> 1;
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p == pos) c[4 * g + p] = v[j];
        }
        if (codes) {
            if constexpr (CB == 4) {
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) { lo |= c[i] << (4 * i); hi |= c[8 + i] << (4 * i); }
                *reinterpret_cast<uint2*>(codes + (size_t)n * (K / 2) + k0 / 2) = make_uint2(lo, hi);
            } else {
                uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 16; i++) wd[i >> 2] |= c[i] << (8 * (i & 3));
                *reinterpret_cast<uint4*>(codes + (size_t)n * K + k0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
        }
        if (codes8) {
            uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t byte = CB == 4 ? (c[i] >= 8 ? c[i] + 0xf0u : c[i]) : c[i];     // sign-extend a nibble to a byte
                wd[i >> 2] |= byte << (8 * (i & 3));
            }
            *reinterpret_cast<uint4*>(codes8 + (size_t)n * K + k0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        }
    }
}

// 8 exponent bytes p[0..7] of a row as two exp4 dwords (cnt < 8: the bytes from cnt on are not read and give 0)
__device__ __forceinline__ void exps8(const int8_t* p, bool dwords, int cnt, uint32_t (&d)[2])
{
    if (dwords) {
        d[0] = exp4(p, 0, 4, true);
        d[1] = cnt > 4 ? exp4(p, 4, 4, true) : 0u;
    } else {
        d[0] = exp4(p, 0, cnt, false);
        d[1] = exp4(p, 4, cnt - 4, false);
    }
}

// few tokens: wave = 16 features x 16 tokens (token group blockIdx.y) x `gps` groups of 8 blocks; fp32 slab [slice][T][N]
template <int CB>
__global__ void __launch_bounds__(256) k_sp24_decode(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ idx, const int8_t* __restrict__ we,
                                                     const int8_t* __restrict__ xc, const int8_t* __restrict__ xe, float* __restrict__ slabs,
                                                     int T, int N, int K, int gps, int slices, int wm, int xm)
{
    constexpr int U = Sp<CB>::U, CH = Sp<CB>::CH;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int row_tiles = N / 16;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int rt = wave % row_tiles, slice = wave / row_tiles;
    if (slice >= slices) return;                                 // grid rounded up to whole workgroups
    const int nb = K / 64;
    const int b0 = slice * gps * GROUP;
    const int b1 = b0 + gps * GROUP < nb ? b0 + gps * GROUP : nb;
    const int n0 = rt * 16, tok = blockIdx.y * 16 + r;
    const int tx = tok < T ? tok : T - 1;                        // token columns past T repeat the last token (results dropped)
    const int8_t* xrow = xc + (size_t)tx * K + 16 * q;
    const int8_t* xer = xe + (size_t)tx * nb;
    const int8_t* wer = we + (size_t)(n0 + 4 * q) * nb;
    // exponent rows as dwords when every row starts 4-aligned (the base pointers are 4-aligned when the entry lets this through)
    const bool dwords = (nb & 3) == 0 && !((reinterpret_cast<uintptr_t>(we) | reinterpret_cast<uintptr_t>(xe)) & 3u);
    v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};

    for (int g0 = b0; g0 < b1; g0 += GROUP) {
        const int cnt = b1 - g0 < GROUP ? b1 - g0 : GROUP;      // blocks in this step (< 8 only at the row's end: b0 is a multiple of 8)
        uint32_t ixs[GROUP];
        uint32_t vw[GROUP][2];
        if (cnt == GROUP) {
            const uint4 iv = *reinterpret_cast<const uint4*>(idx + sp24_off(rt, nb, g0, lane, IDX_CH, 2));
            const uint32_t id[4] = {iv.x, iv.y, iv.z, iv.w};
#pragma unroll
            for (int i = 0; i < GROUP; i++) ixs[i] = (id[i >> 1] >> (16 * (i & 1))) & 0xffffu;
#pragma unroll
            for (int c = 0; c < GROUP / CH; c++) {
                const uint4 v = *reinterpret_cast<const uint4*>(vals + sp24_off(rt, nb, g0 + c * CH, lane, CH, U));
                const uint32_t vd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    vw[c * CH + i][0] = CB == 4 ? vd[i] : vd[2 * i];
                    vw[c * CH + i][1] = CB == 4 ? 0u : vd[2 * i + 1];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < GROUP; i++) {
                const int b = g0 + (i < cnt ? i : cnt - 1);
                ixs[i] = *reinterpret_cast<const uint16_t*>(idx + sp24_off(rt, nb, b, lane, IDX_CH, 2));
                const uint8_t* vp = vals + sp24_off(rt, nb, b, lane, CH, U);
                if constexpr (CB == 4) { vw[i][0] = *reinterpret_cast<const uint32_t*>(vp); vw[i][1] = 0u; }
                else { const uint2 v = *reinterpret_cast<const uint2*>(vp); vw[i][0] = v.x; vw[i][1] = v.y; }
            }
        }
        uint32_t exx[2], ew[4][2];
        exps8(xer + g0, dwords, cnt, exx);
#pragma unroll
        for (int j = 0; j < 4; j++) exps8(wer + (size_t)j * nb + g0, dwords, cnt, ew[j]);
#pragma unroll
        for (int i = 0; i < GROUP; i++) {
            if (i >= cnt) break;
            const v4i bx = *reinterpret_cast<const v4i*>(xrow + (size_t)(g0 + i) * 64);
            const v2i a = CB == 4 ? nibbles_to_i8(vw[i][0]) : v2i{(int)vw[i][0], (int)vw[i][1]};
            // the C operand is also the destination.  hipcc (ROCm 7.2) re-initialises only part of the destination between two
            // instructions when C is a splat constant, so C is built from four opaque registers every time
            int m0 = MAGIC_I, m1 = MAGIC_I, m2 = MAGIC_I, m3 = MAGIC_I;
            asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3));
            const v4i c = {m0, m1, m2, m3};
            const v4i d = __builtin_amdgcn_smfmac_i32_16x16x64_i8(a, bx, c, (int)ixs[i], 0, 0);
            const int e = i >> 2, sh = 8 * (i & 3);
            v2f sx, nm;
            token_scale(exp_byte(exx[e], sh), xm, sx, nm);
            const v2f sw01 = {pow2_scale(exp_byte(ew[0][e], sh), wm), pow2_scale(exp_byte(ew[1][e], sh), wm)};
            const v2f sw23 = {pow2_scale(exp_byte(ew[2][e], sh), wm), pow2_scale(exp_byte(ew[3][e], sh), wm)};
            rescale(d, sx, nm, sw01, sw23, acc01, acc23);
        }
    }
    if (tok < T) store4<BFPQ_F32>(slabs, ((size_t)slice * T + tok) * N + n0 + 4 * q, acc01, acc23);
}

bool sp24_shape_ok(int64_t N, int64_t K) { return N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 && N * K < ((int64_t)1 << 32); }

int64_t grid_items(int64_t N, int64_t K)
{
    const int64_t g = ((N / 16) * (K / 64) * 64 + 255) / 256;
    return g < 8192 ? g : 8192;
}

// the K split: groups of 8 blocks per slice, aiming at ~4096 waves on the chip
void sp24_plan(int64_t T, int64_t N, int64_t K, int* gps, int* slices)
{
    const int64_t ng = (K / 64 + GROUP - 1) / GROUP, waves = (N / 16) * ((T + 15) / 16);
    int64_t s = (4096 + waves - 1) / waves;
    if (s > ng) s = ng;
    if (s < 1) s = 1;
    const int64_t per = (ng + s - 1) / s;
    *gps = (int)per;
    *slices = (int)((ng + per - 1) / per);
}

}  // namespace

extern "C" {

int bfpq_sp24_pack(const void* codes, void* vals, void* idx, int64_t N, int64_t K, int code_bits, int32_t* status, void* stream)
{
    if (code_bits != 4 && code_bits != 8) return BFPQ_E_ARG;
    if (N < 0 || K < 0) return BFPQ_E_ARG;
    if (N == 0 || K == 0) return 0;
    if (!sp24_shape_ok(N, K)) return BFPQ_E_UNSUPPORTED;
    if (!codes || !vals || !idx || !status) return BFPQ_E_ARG;
    if (!aligned16(codes, vals, idx) || (reinterpret_cast<uintptr_t>(status) & 3u)) return BFPQ_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)grid_items(N, K));
    if (code_bits == 4) hipLaunchKernelGGL(k_sp24_pack<4>, grid, dim3(256), 0, s, (const uint8_t*)codes, (uint8_t*)vals, (uint8_t*)idx, (int)N, (int)K, status);
    else hipLaunchKernelGGL(k_sp24_pack<8>, grid, dim3(256), 0, s, (const uint8_t*)codes, (uint8_t*)vals, (uint8_t*)idx, (int)N, (int)K, status);
    return (int)hipGetLastError();
}

int bfpq_sp24_unpack(const void* vals, const void* idx, void* codes, void* codes8, int64_t N, int64_t K, int code_bits, void* stream)
{
    if (code_bits != 4 && code_bits != 8) return BFPQ_E_ARG;
    if (N < 0 || K < 0) return BFPQ_E_ARG;
    if (N == 0 || K == 0) return 0;
    if (!sp24_shape_ok(N, K)) return BFPQ_E_UNSUPPORTED;
    if (!vals || !idx || (!codes && !codes8)) return BFPQ_E_ARG;
    if (!aligned16(vals, idx, codes, codes8)) return BFPQ_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)grid_items(N, K));
    if (code_bits == 4) hipLaunchKernelGGL(k_sp24_unpack<4>, grid, dim3(256), 0, s, (const uint8_t*)vals, (const uint8_t*)idx, (uint8_t*)codes, (int8_t*)codes8, (int)N, (int)K);
    else hipLaunchKernelGGL(k_sp24_unpack<8>, grid, dim3(256), 0, s, (const uint8_t*)vals, (const uint8_t*)idx, (uint8_t*)codes, (int8_t*)codes8, (int)N, (int)K);
    return (int)hipGetLastError();
}

int64_t bfpq_hbfp_linear_sp24_ws(int64_t T, int64_t N, int64_t K)
{
    if (T < 1 || T > BFPQ_SP24_MAX_TOKENS || !sp24_shape_ok(N, K) || T * K >= ((int64_t)1 << 32)) return BFPQ_E_UNSUPPORTED;
    int gps, slices;
    sp24_plan(T, N, K, &gps, &slices);
    return (int64_t)slices * T * N;
}

int bfpq_hbfp_linear_sp24(const void* xcodes, const int8_t* xexp, const void* wvals, const void* widx, const int8_t* wexp, const void* bias,
                          void* out, float* slabs, int64_t T, int64_t N, int64_t K, int code_bits, int out_dtype, int w_mant_bits,
                          int x_mant_bits, void* stream)
{
    if (!dtype_ok(out_dtype) || (code_bits != 4 && code_bits != 8) || !codes_fit(code_bits, w_mant_bits) || !i8_mant_ok(w_mant_bits) ||
        !i8_mant_ok(x_mant_bits) || T < 1 || N < 1 || K < 1)
        return BFPQ_E_ARG;
    if (bfpq_hbfp_linear_sp24_ws(T, N, K) < 0) return BFPQ_E_UNSUPPORTED;
    if (!xcodes || !xexp || !wvals || !widx || !wexp || !out || !slabs) return BFPQ_E_ARG;
    if (!aligned16(xcodes, wvals, widx, slabs)) return BFPQ_E_ARG;
    int gps, slices;
    sp24_plan(T, N, K, &gps, &slices);
    const int64_t waves = (N / 16) * slices, groups = (T + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((waves + 3) / 4), (unsigned)groups);
    if (code_bits == 4)
        hipLaunchKernelGGL(k_sp24_decode<4>, grid, dim3(256), 0, s, (const uint8_t*)wvals, (const uint8_t*)widx, wexp, (const int8_t*)xcodes, xexp,
                           slabs, (int)T, (int)N, (int)K, gps, slices, w_mant_bits, x_mant_bits);
    else
        hipLaunchKernelGGL(k_sp24_decode<8>, grid, dim3(256), 0, s, (const uint8_t*)wvals, (const uint8_t*)widx, wexp, (const int8_t*)xcodes, xexp,
                           slabs, (int)T, (int)N, (int)K, gps, slices, w_mant_bits, x_mant_bits);
    launch_slab_reduce(out_dtype, slabs, (size_t)(T * N), bias, out, T * N, N, slices, s);
    return (int)hipGetLastError();
}

}  // extern "C"
