// bfpq_bmm.hip -- the batched contraction of two activations, both HBFP: out[b][t][n] = sum_k x[b][t][k] w[b][n][k], b < B, with x and w
// int8 codes + one int8 exponent per block of 64, 32 or 16, mantissa widths xm, wm in 1..7.  Replaces torch.matmul on the two
// fake-quantised operands of F_matmul_bfp (reference bfp_ops.py:240-245 through :187-190), the attention matmuls of the reference's
// GPT-2 (modeling_gpt2.py:207, 243, 297).  Neither operand is a weight: both sets of codes are made per call -- or, decoding with
// layer_past (modeling_gpt2.py:345-348), w's are the codes of a KV cache (bfpq_kvcache.hip): bfpq_hbfp_bmm_i8_strided gives w a row pitch,
// an exponent pitch, a batch stride and a count of valid rows of its own.
//
// Arithmetic: the int8 block product of bfpq_i8mma.h (exactness argument, NaN marker and lane map are there).  One
// v_mfma_i32_16x16x64_i8 per block of 64 (v_mfma_i32_16x16x32_i8 per block of 32 or 16), an exact integer block sum, one rescale by
// 2^(ex - xm) * 2^(ew - wm), fp32 accumulation across blocks in block order.
//
// Layout: code rows have a pitch ldk (a multiple of 64, >= K) with zero codes in the pad, so K is walked in 64-byte chunks whatever
// K % 64 is (K = 32 and K = 64 take the same path; blocks past K / BLK are skipped, their exponents do not exist).  Exponent rows are
// dense, [rows, K / BLK]; they are read a dword = 4 blocks at a time where the rows are 4-byte aligned, byte by byte elsewhere.  No
// K % 256 requirement, no split-K, no LDS: the two shape families of attention leave nothing for a staged tile to re-use --
//   Q K^T: K = 64 or 128 is one or two chunks, the time goes to the [T, N] output write;
//   P V:   N = 64 or 128 is one tile row, x = P's codes are read exactly once, w = V's codes ([N, ldk], 64-256 KB) stay in L2 / L1.
// A wave owns 16 TM output features (w rows, the MFMA's A) x 16 TN tokens (x rows, B) and reads its operands straight from global
// memory, 16 bytes per lane and row (no register double buffer: it spilled; 2-4 waves per SIMD cover the latency).  The four waves of a workgroup are neighbours along T (they share
// the w rows, so those hit in L1).  Batch is gridDim.y (a grid-stride loop past 65535).  A lane ends with four consecutive
// output features of one token -- one 8- or 16-byte store.
//
// k_codes_t: the quantizer for an operand whose blocks run along its second-to-last dimension (V in P V): reads v[B, S, D] once and
// writes int8 codes [B, D, ldk] + int8 exponents [B, D, S / BLK], the operand float_to_bfp_blocked(v.transpose(-1, -2)) as codes
// (reference bfp_ops.py:153: the transposed copy, the quantizer launch and the transpose back).  A workgroup transposes a tile of
// 64 s x 64 d through LDS: 16-byte loads along d, the block maximum and the step-by-step scale of bfpq_common.h per (d, block), 16 codes
// of one d per thread, and 16-byte stores along s from a second LDS tile.  Rows s >= S of a tile read as zeros and quantize to zero
// codes: that is the pad up to ldk.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfpq.h"
#include "bfpq_common.h"
#include "bfpq_device.h"
#include "bfpq_i8mma.h"

using namespace bfpq;

namespace {

constexpr int kWaves = 4;                                 // waves of a workgroup, neighbours along T

// (the second launch bound is waves per SIMD: without it the compiler spends the whole register file on hoisted loads at occupancy 1)
template <int BLK, int OUT_DT, int TM, int TN>
__global__ void __launch_bounds__(64 * kWaves, TN == 4 ? 2 : 3) k_bmm_i8(const int8_t* __restrict__ xc, const int8_t* __restrict__ xe, const int8_t* __restrict__ wc,
                                                        const int8_t* __restrict__ we, void* __restrict__ out, int B, int T, int N, int K, int ldk,
                                                        int tiles_t, int xm, int wm, int ldw, int ldwe, int wbs, int nv)
{
    using Blk = I8Blk<BLK>;
    using op_t = typename Blk::op_t;
    constexpr int NBS = 64 / BLK;                                // blocks per 64-byte chunk
    constexpr int CPG = 4 / NBS > 0 ? 4 / NBS : 1;               // chunks per exponent dword (4 blocks)
    constexpr int BN = 16 * TM, BT = 16 * TN;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 15, q = l >> 4;
    const int t0 = (((int)blockIdx.x % tiles_t) * kWaves + w) * BT, n0 = ((int)blockIdx.x / tiles_t) * BN;
    if (t0 >= T) return;                                         // (wave-uniform; the kernel has no barrier)
    const int nb = K / BLK, nch = (K + 63) >> 6;
    const bool dw = !((nb | ldwe) & 3) && !((reinterpret_cast<uintptr_t>(xe) | reinterpret_cast<uintptr_t>(we)) & 3u);

    // w: code rows of pitch ldw, exponent rows of pitch ldwe, wbs rows from one batch to the next, nv of them valid (dense: ldk, K / BLK, N, N).
    // rows past nv / T repeat the last row (their results are not stored, or are the caller's to drop)
    uint32_t offW[TM], offX[TN], ewo[TM][4], exo[TN];
#pragma unroll
    for (int i = 0; i < TM; i++) {
        const int n = n0 + 16 * i + r;
        offW[i] = (uint32_t)(n < nv ? n : nv - 1) * (uint32_t)ldw + Blk::lane(q);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int ne = n0 + 16 * i + 4 * q + j;
            ewo[i][j] = (uint32_t)(ne < nv ? ne : nv - 1) * (uint32_t)ldwe;
        }
    }
#pragma unroll
    for (int jt = 0; jt < TN; jt++) {
        const int t = t0 + 16 * jt + r;
        offX[jt] = (uint32_t)(t < T ? t : T - 1) * (uint32_t)ldk + Blk::lane(q);
        exo[jt] = (uint32_t)(t < T ? t : T - 1) * (uint32_t)nb;
    }
    const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};

    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int8_t* const xcb = xc + (size_t)b * T * ldk;
        const int8_t* const wcb = wc + (size_t)b * wbs * ldw;
        const int8_t* const xeb = xe + (size_t)b * T * nb;
        const int8_t* const web = we + (size_t)b * wbs * ldwe;

        // the lane's operands of chunk c: NBS pieces per row (one 16-byte piece at block 64, 8-byte pieces at blocks 32 / 16)
        auto codes = [&](int c, op_t (&aF)[TM][NBS], op_t (&bF)[TN][NBS]) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int s = 0; s < NBS; s++) {
                    aF[i][s] = *reinterpret_cast<const op_t*>(wcb + offW[i] + (c << 6) + s * BLK);
                    if (!Blk::a_live(q)) aF[i][s] = op_t{};
                }
#pragma unroll
            for (int jt = 0; jt < TN; jt++)
#pragma unroll
                for (int s = 0; s < NBS; s++) bF[jt][s] = *reinterpret_cast<const op_t*>(xcb + offX[jt] + (c << 6) + s * BLK);
        };
        auto exps = [&](int g, uint32_t (&ewd)[TM][4], uint32_t (&exd)[TN]) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) ewd[i][j] = exp4(web, ewo[i][j] + 4 * g, nb - 4 * g, dw);
#pragma unroll
            for (int jt = 0; jt < TN; jt++) exd[jt] = exp4(xeb, exo[jt] + 4 * g, nb - 4 * g, dw);
        };

        v2f acc[TM][TN][2];
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int jt = 0; jt < TN; jt++) acc[i][jt][0] = acc[i][jt][1] = v2f{0.f, 0.f};

        op_t aF[TM][NBS], bF[TN][NBS];
        uint32_t ewd[TM][4], exd[TN];
#pragma unroll 1
        for (int c = 0; c < nch; c++) {
            if (c % CPG == 0) exps(c / CPG, ewd, exd);           // a new exponent dword
            codes(c, aF, bF);
#pragma unroll
            for (int s = 0; s < NBS; s++) {
                const int blk = c * NBS + s;
                if (blk < nb) {                                  // (K % 64 != 0: the tail of the last chunk is pad)
                    const int sh = 8 * (blk & 3);                // its byte of the exponent dwords
                    v2f sx[TN], nm[TN];
#pragma unroll
                    for (int jt = 0; jt < TN; jt++) token_scale(exp_byte(exd[jt], sh), xm, sx[jt], nm[jt]);
#pragma unroll
                    for (int i = 0; i < TM; i++) {
                        const v2f sw01 = v2f{pow2_scale(exp_byte(ewd[i][0], sh), wm), pow2_scale(exp_byte(ewd[i][1], sh), wm)};
                        const v2f sw23 = v2f{pow2_scale(exp_byte(ewd[i][2], sh), wm), pow2_scale(exp_byte(ewd[i][3], sh), wm)};
#pragma unroll
                        for (int jt = 0; jt < TN; jt++)
                            rescale(Blk::mfma(aF[i][s], bF[jt][s], magic), sx[jt], nm[jt], sw01, sw23, acc[i][jt][0], acc[i][jt][1]);
                    }
                }
            }
        }

        // the lane holds features n .. n + 3 of token t
        const size_t ob = (size_t)b * T * N;
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const int n = n0 + 16 * i + 4 * q;
            if (n >= N) continue;                                // (N % 16 == 0: all four or none)
#pragma unroll
            for (int jt = 0; jt < TN; jt++) {
                const int t = t0 + 16 * jt + r;
                if (t >= T) continue;
                store4<OUT_DT>(out, ob + (size_t)t * N + n, acc[i][jt][0], acc[i][jt][1]);
            }
        }
    }
}

// ---- the transposed quantizer ----------------------------------------------------------------------------------------------------
constexpr int kTS = 64, kTD = 64;                            // tile: s x d
constexpr int kPitch = kTD + 1;                              // words per s row of the value tile (column reads hit 64 banks)

template <int DT>
__global__ void __launch_bounds__(256) k_codes_t(const void* __restrict__ in, int8_t* __restrict__ codes, int8_t* __restrict__ exps, int B, int S,
                                                 int D, int ldk, int block, int mant_bits, float eps_dt, const uint8_t* __restrict__ exp_win)
{
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    constexpr int VEC = Tr::VEC, LPR = kTD / VEC, RPP = 256 / LPR;        // lanes per tile row, rows per pass
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    __shared__ uint32_t s_val[kTS * kPitch];                              // raw values, [s][d]
    __shared__ uint32_t s_max[4 * kTD];                                   // magnitude maximum of each wave's 16 s, per d
    __shared__ __attribute__((aligned(16))) int8_t s_code[kTD * kTS];     // codes, [d][s]
    const int tid = threadIdx.x;
    for (int i = tid; i < BFPQ_EXP_WIN_ENTRIES; i += 256) s_win[i] = exp_win[i];
    const int s0 = blockIdx.x * kTS, d0 = blockIdx.y * kTD;
    const int nb = S / block;
    const int d = tid & 63, sq = tid >> 6;                                // this thread's column and its 16 rows sq * 16 .. +15
    const int per = block >> 4;                                           // waves that share a block (1, 2 or 4)
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const raw_t* const src = reinterpret_cast<const raw_t*>(in) + (size_t)b * S * D;
        __syncthreads();                                                  // (the previous batch's tiles are read; s_win is written)
        // load: 16 bytes per lane along d; rows past S and columns past D read as zeros
#pragma unroll
        for (int p = 0; p < kTS / RPP; p++) {
            const int row = p * RPP + tid / LPR, col = (tid % LPR) * VEC;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (s0 + row < S && d0 + col < D) v = *reinterpret_cast<const uint4*>(src + (size_t)(s0 + row) * D + d0 + col);
            uint32_t* const dst = s_val + row * kPitch + col;
            if constexpr (VEC == 4) {
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            } else {
                dst[0] = v.x & 0xffffu; dst[1] = v.x >> 16; dst[2] = v.y & 0xffffu; dst[3] = v.y >> 16;
                dst[4] = v.z & 0xffffu; dst[5] = v.z >> 16; dst[6] = v.w & 0xffffu; dst[7] = v.w >> 16;
            }
        }
        __syncthreads();
        uint32_t raw[16], mx = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            raw[i] = s_val[(sq * 16 + i) * kPitch + d];
            const uint32_t k = raw[i] & Tr::ABS;
            mx = k > mx ? k : mx;
        }
        s_max[sq * kTD + d] = mx;
        __syncthreads();
        const int first = sq & ~(per - 1);                                // first wave of this thread's block
        for (int o = 0; o < per; o++) { const uint32_t k = s_max[(first + o) * kTD + d]; mx = k > mx ? k : mx; }
        const BlockScale bs = block_scale<DT>(mx, mant_bits, eps_dt, s_win);
        uint32_t pk[4];
        pack_codes<DT>(raw, 16, bs, pk);
        *reinterpret_cast<uint4*>(s_code + d * kTS + sq * 16) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        const int s = s0 + sq * 16;
        if (sq == first && s < S && d0 + d < D) exps[((size_t)b * D + d0 + d) * nb + s / block] = sat_exp(bs);
        __syncthreads();
        // store: 16 bytes per lane along s, four lanes per d row
        const int dr = tid >> 2, piece = (tid & 3) * 16;
        if (d0 + dr < D && s0 + piece < ldk)
            *reinterpret_cast<uint4*>(codes + ((size_t)b * D + d0 + dr) * ldk + s0 + piece) = *reinterpret_cast<const uint4*>(s_code + dr * kTS + piece);
    }
}

// tokens per wave: 16 TN.  The widest tile that still gives every SIMD of the chip two waves, else the narrowest (P V at batch 1 has
// few tiles; Q K^T has thousands)
int bmm_tn(int64_t B, int64_t T, int64_t N)
{
    const int64_t rows = (N + 63) / 64;
    for (int tn = 4; tn > 1; tn >>= 1)
        if (B * rows * ((T + 16 * tn - 1) / (16 * tn)) >= 2048) return tn;
    return 1;
}

}  // namespace

extern "C" {

int bfpq_hbfp_bmm_i8_ok(int64_t B, int64_t T, int64_t N, int64_t K, int64_t ldk, int block_size)
{
    const int64_t lim = (int64_t)1 << 31;
    return i8_block_ok(block_size) && B >= 1 && T >= 1 && N >= 16 && N % 16 == 0 && K >= block_size && K % block_size == 0 && ldk >= K &&
           ldk % 64 == 0 && T * ldk < lim && N * ldk < lim && T * N < lim && ((T + 15) / 16) * ((N + 63) / 64) < lim / 4;
}

int bfpq_hbfp_bmm_i8_strided(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, void* out, int64_t B, int64_t T,
                             int64_t N, int64_t K, int64_t ldk, int64_t w_ld, int64_t w_exp_ld, int64_t w_bstride, int64_t w_rows, int block_size,
                             int out_dtype, int w_mant_bits, int x_mant_bits, void* stream)
{
    if (!dtype_ok(out_dtype) || !i8_block_ok(block_size) || !i8_mant_ok(w_mant_bits) || !i8_mant_ok(x_mant_bits) || B < 0 ||
        T < 0 || N < 0)
        return BFPQ_E_ARG;
    if (B == 0 || T == 0 || N == 0) return 0;
    if (!bfpq_hbfp_bmm_i8_ok(B, T, N, K, ldk, block_size)) return BFPQ_E_UNSUPPORTED;
    const int64_t lim = (int64_t)1 << 31;
    if (w_ld % 64 != 0 || w_ld < (K + 63) / 64 * 64 || w_exp_ld < K / block_size || w_rows < 1 || w_rows > N || w_bstride < w_rows ||
        w_bstride * w_ld >= lim || w_bstride * w_exp_ld >= lim)
        return BFPQ_E_UNSUPPORTED;
    if (!xcodes || !xexp || !wcodes || !wexp || !out || !aligned16(xcodes, wcodes, out)) return BFPQ_E_ARG;
    const int tn = bmm_tn(B, T, N);
    const int tiles_t = (int)((T + 16 * tn * kWaves - 1) / (16 * tn * kWaves));
    const dim3 grid((unsigned)(tiles_t * ((N + 63) / 64)), (unsigned)(B < 65535 ? B : 65535));
    hipStream_t s = (hipStream_t)stream;
    with_block(block_size, [&](auto blk) {
        with_dtype(out_dtype, [&](auto dt) {
            auto go = [&](auto tnc) {
                hipLaunchKernelGGL((k_bmm_i8<decltype(blk)::value, decltype(dt)::value, 4, decltype(tnc)::value>), grid, dim3(64 * kWaves), 0, s,
                                   (const int8_t*)xcodes, xexp, (const int8_t*)wcodes, wexp, out, (int)B, (int)T, (int)N, (int)K, (int)ldk, tiles_t,
                                   x_mant_bits, w_mant_bits, (int)w_ld, (int)w_exp_ld, (int)w_bstride, (int)w_rows);
            };
            if (tn == 4) go(std::integral_constant<int, 4>{});
            else if (tn == 2) go(std::integral_constant<int, 2>{});
            else go(std::integral_constant<int, 1>{});
        });
    });
    return (int)hipGetLastError();
}

int bfpq_hbfp_bmm_i8(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, void* out, int64_t B, int64_t T, int64_t N,
                     int64_t K, int64_t ldk, int block_size, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream)
{
    // w dense: the pitch of x, K / block exponents per row, N rows per batch, all of them valid
    return bfpq_hbfp_bmm_i8_strided(xcodes, xexp, wcodes, wexp, out, B, T, N, K, ldk, ldk, i8_block_ok(block_size) ? K / block_size : 0, N, N,
                                    block_size, out_dtype, w_mant_bits, x_mant_bits, stream);
}

int bfpq_hbfp_codes_t(const void* in, void* codes, int8_t* exps, int64_t B, int64_t S, int64_t D, int64_t ldk, int dtype, int block_size,
                      int mant_bits, double epsilon, const uint8_t* exp_win, void* stream)
{
    if (!dtype_ok(dtype) || !i8_block_ok(block_size) || !i8_mant_ok(mant_bits) || B < 0 || S < 0 || D < 0) return BFPQ_E_ARG;
    if (B == 0 || S == 0 || D == 0) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if (S % block_size != 0 || D % 16 != 0 || ldk < S || ldk % 64 != 0 || S * D >= lim || D * ldk >= lim || ldk / 64 >= lim ||
        (D + kTD - 1) / kTD > 65535)
        return BFPQ_E_UNSUPPORTED;
    if (!in || !codes || !exps || !exp_win || !aligned16(in, codes)) return BFPQ_E_ARG;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    const dim3 grid((unsigned)(ldk / kTS), (unsigned)((D + kTD - 1) / kTD), (unsigned)(B < 65535 ? B : 65535));
    with_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_codes_t<decltype(dt)::value>), grid, dim3(256), 0, (hipStream_t)stream, in, (int8_t*)codes, exps, (int)B, (int)S,
                           (int)D, (int)ldk, block_size, mant_bits, eps_dt, exp_win);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
