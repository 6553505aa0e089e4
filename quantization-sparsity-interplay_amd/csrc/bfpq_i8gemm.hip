// bfpq_i8gemm.hip -- consumer of packed HBFP with mantissas of up to 7 bits (HBFP5-HBFP8): out[t][n] = sum_k x[t][k] W[n][k] (+ bias[n])
// with x and W both int8 codes + one int8 exponent per block of 64, mantissa widths xm, wm in 1..7.  Replaces F.linear on the two
// fake-quantised operands (bfp_ops.py:187-190).
//
// Arithmetic: the int8 block product of bfpq_i8mma.h -- an exact integer sum per block on the int8 matrix unit, one rescale by
// 2^(ex - xm) * 2^(ew - wm) in two packed fp32 FMAs per pair of outputs, fp32 across blocks in block order; the exactness argument, the
// NaN block marker and the lane map are written down there.  The e4m3 route of bfpq_mxgemm.hip does not apply above 4-bit mantissas (a
// 7-bit code is not exact in e4m3).
//
// Kernels (BLK = 64, 32 or 16; blocks 16 and 32 serve bfpq_hbfp_linear_i8b* and bfpq_hbfp_linear_decode8b*):
//   k_i8_gemm<BLK>  prefill tile: WM x WN waves, each TM x TN instruction tiles; K staged global -> LDS by 16-byte LDS-DMA, two LDS
//                 stages of 128 bytes of K each (double buffered: the next stage's DMA is in flight during the current stage's matrix
//                 work), LDS rows of 128 bytes with the 16-byte slot XOR-swizzled by ((row >> 1) & 7).  K % 256 == 0.  Block 64 reads
//                 its exponents one dword = 4 blocks per trip ahead, blocks 16 / 32 one stage (4 or 8 blocks) ahead.  SPLIT: part p of
//                 K goes to fp32 slab p (plain stores) and k_slab_reduce (bfpq_common.h) adds the slabs in part order.
//   k_i8_decode<BLK>  few tokens: a wave owns 16 output features x up to 16 tokens x a slice of K (any K % 64 == 0), slabs reduced as above.
//   k_codes4_to_i8  4-bit two's-complement nibbles (low first) -> int8 codes.
// Blocks 16 and 32 take one v_mfma_i32_16x16x32_i8 per block (I8Blk of bfpq_i8mma.h), 8-byte operands read from the same LDS stages.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfpq.h"
#include "bfpq_common.h"
#include "bfpq_i8mma.h"

using namespace bfpq;

namespace {

constexpr int BK = 128;                                   // bytes of K per LDS stage: two blocks

__device__ __forceinline__ v4i read16(const uint8_t* tile, int row, int c)      // logical 16-byte slot c of an LDS row
{
    return *reinterpret_cast<const v4i*>(tile + row * BK + ((c ^ ((row >> 1) & 7)) << 4));
}

__device__ __forceinline__ long read8(const uint8_t* tile, int row, int o)     // logical bytes o .. o + 7 (o % 8 == 0) of an LDS row
{
    return *reinterpret_cast<const long*>(tile + row * BK + ((((o >> 4) ^ ((row >> 1) & 7))) << 4) + (o & 8));
}

__device__ __forceinline__ void landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }

// What the tile kernel does the same at every block: one lane's share of an output tile of BN output features (weight rows) x BT tokens,
// trips [ta, tb) of K (256 each).  SPLIT: the part's trips go to fp32 slab `part`.
template <int BLK, int WM, int WN, int TM, int TN, bool SPLIT>
struct I8Tile {
    static constexpr int NW = WM * WN, BN = 16 * WM * TM, BT = 16 * WN * TN, STAGE = (BN + BT) * BK;
    static constexpr int GW = BN / 8 / NW, GX = BT / 8 / NW;            // LDS-DMA instructions per wave and stage (8 rows = 1 KB each)
    static_assert(BN % (8 * NW) == 0 && BT % (8 * NW) == 0, "tile rows must split evenly over the waves");
    int w, r, q, part, t0, n0, ta, tb, rowW, rowX;
    uint32_t offW[GW], offX[GX];
    uint32_t ewo[TM][4], exo[TN];                                // first exponent dword of each row the lane scales
    v2f acc[TM][TN][2];

    __device__ __forceinline__ I8Tile(int T, int N, int K, int tiles_t, int tiles, int trips_per_part)
    {
        w = threadIdx.x >> 6;
        const int l = threadIdx.x & 63;
        r = l & 15, q = l >> 4;
        part = SPLIT ? (int)blockIdx.x / tiles : 0;
        const int tile = SPLIT ? (int)blockIdx.x % tiles : (int)blockIdx.x;
        t0 = (tile % tiles_t) * BT, n0 = (tile / tiles_t) * BN;
        const int trips = K >> 8, nd = BLK == 64 ? K >> 8 : K / BLK / 4;     // exponent dwords per row
        ta = part * trips_per_part, tb = ta + trips_per_part < trips ? ta + trips_per_part : trips;
        // staging: instruction i of wave w fills LDS rows (NW i + w) * 8 .. +7; lane l = row l >> 3, physical slot l & 7 holds the row's
        // logical slot (l & 7) ^ ((row >> 1) & 7).  Rows past N / T repeat the last row (their results are not stored).
#pragma unroll
        for (int i = 0; i < GW; i++) {
            const int row = (NW * i + w) * 8 + (l >> 3), piece = ((l & 7) ^ ((row >> 1) & 7)) << 4;
            const int na = n0 + row < N ? n0 + row : N - 1;
            offW[i] = (uint32_t)na * (uint32_t)K + piece;
        }
#pragma unroll
        for (int i = 0; i < GX; i++) {
            const int row = (NW * i + w) * 8 + (l >> 3), piece = ((l & 7) ^ ((row >> 1) & 7)) << 4;
            const int tr = t0 + row < T ? t0 + row : T - 1;
            offX[i] = (uint32_t)tr * (uint32_t)K + piece;
        }
        const int wr = w / WN, wcl = w % WN;
        rowW = wr * (16 * TM), rowX = wcl * (16 * TN);               // the wave's first LDS row of each operand
        // exponent rows: weight rows n0 + rowW + 16 i + 4 q + j, token rows t0 + rowX + 16 jt + r
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int n = n0 + rowW + 16 * i + 4 * q + j;
                ewo[i][j] = (uint32_t)(n < N ? n : N - 1) * (uint32_t)nd;
            }
#pragma unroll
        for (int jt = 0; jt < TN; jt++) {
            const int t = t0 + rowX + 16 * jt + r;
            exo[jt] = (uint32_t)(t < T ? t : T - 1) * (uint32_t)nd;
        }
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int jt = 0; jt < TN; jt++) acc[i][jt][0] = acc[i][jt][1] = v2f{0.f, 0.f};
    }

    // LDS-DMA of the 128 bytes of K from k0 into stage buffer buf
    __device__ __forceinline__ void stage(uint8_t* lds, const int8_t* wc, const int8_t* xc, int k0, int buf) const
    {
        uint8_t* const sW = lds + buf * STAGE;
        uint8_t* const sX = sW + BN * BK;
#pragma unroll
        for (int i = 0; i < GW; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wc + offW[i] + k0),
                                             (__attribute__((address_space(3))) void*)(sW + (NW * i + w) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < GX; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xc + offX[i] + k0),
                                             (__attribute__((address_space(3))) void*)(sX + (NW * i + w) * 1024), 16, 0, 0);
    }

    // the lane's operand of block b of a staged row
    __device__ __forceinline__ typename I8Blk<BLK>::op_t read_op(const uint8_t* tile, int row, int b) const
    {
        if constexpr (BLK == 64) return read16(tile, row, b * 4 + q);
        else return read8(tile, row, b * BLK + I8Blk<BLK>::lane(q));
    }

    // block b of the stage in buffer buf: the operands from LDS, one MFMA + rescale per instruction tile.  The block's exponents are
    // the byte at bit sh of the rows' dwords ewd[i][j][e], exd[jt][e]
    template <int ED>
    __device__ __forceinline__ void block(const uint8_t* lds, int buf, int b, const uint32_t (&ewd)[TM][4][ED], const uint32_t (&exd)[TN][ED],
                                          int e, int sh, int xm, int wm)
    {
        using Blk = I8Blk<BLK>;
        const uint8_t* const sW = lds + buf * STAGE;
        const uint8_t* const sX = sW + BN * BK;
        typename Blk::op_t aF[TM], bF[TN];
#pragma unroll
        for (int i = 0; i < TM; i++) {
            aF[i] = read_op(sW, rowW + 16 * i + r, b);
            if (!Blk::a_live(q)) aF[i] = {};
        }
#pragma unroll
        for (int jt = 0; jt < TN; jt++) bF[jt] = read_op(sX, rowX + 16 * jt + r, b);
        v2f sx[TN], nm[TN];
#pragma unroll
        for (int jt = 0; jt < TN; jt++) token_scale(exp_byte(exd[jt][e], sh), xm, sx[jt], nm[jt]);
        const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const v2f sw01 = v2f{pow2_scale(exp_byte(ewd[i][0][e], sh), wm), pow2_scale(exp_byte(ewd[i][1][e], sh), wm)};
            const v2f sw23 = v2f{pow2_scale(exp_byte(ewd[i][2][e], sh), wm), pow2_scale(exp_byte(ewd[i][3][e], sh), wm)};
#pragma unroll
            for (int jt = 0; jt < TN; jt++)
                rescale(Blk::mfma(aF[i], bF[jt], magic), sx[jt], nm[jt], sw01, sw23, acc[i][jt][0], acc[i][jt][1]);
        }
    }

    // epilogue: lane holds features n .. n + 3 of token t.  (The biased store is written out here, not store4 + a bias: with the bias add
    // in or in front of a shared function hipcc (ROCm 7.2) hoists bias + n instead of out + n and the register counts change)
    template <int OUT_DT>
    __device__ __forceinline__ void store(const void* bias, void* out, int T, int N) const
    {
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const int n = n0 + rowW + 16 * i + 4 * q;
            if (n >= N) continue;                                    // (N % 16 == 0: all four or none)
#pragma unroll
            for (int jt = 0; jt < TN; jt++) {
                const int t = t0 + rowX + 16 * jt + r;
                if (t >= T) continue;
                if constexpr (SPLIT) store4<BFPQ_F32>(out, ((size_t)part * T + t) * N + n, acc[i][jt][0], acc[i][jt][1]);
                else {
                    const v2f a01 = acc[i][jt][0], a23 = acc[i][jt][1];
                    using raw_t = typename Traits<OUT_DT>::raw_t;
                    float v[4] = {a01.x, a01.y, a23.x, a23.y};
                    if (bias) {
#pragma unroll
                        for (int j = 0; j < 4; j++) v[j] += raw_to_f32<OUT_DT>((uint32_t)reinterpret_cast<const raw_t*>(bias)[n + j]);
                    }
                    if constexpr (OUT_DT == BFPQ_F32) {
                        *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + (size_t)t * N + n) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
                        const uint32_t lo = f32_to_raw<OUT_DT>(v[0]) | (f32_to_raw<OUT_DT>(v[1]) << 16);
                        const uint32_t hi = f32_to_raw<OUT_DT>(v[2]) | (f32_to_raw<OUT_DT>(v[3]) << 16);
                        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + (size_t)t * N + n) = make_uint2(lo, hi);
                    }
                }
            }
        }
    }
};

// the prefill tile.  The exponent schedule is the block's: block 64 reads one dword (4 blocks) per row and trip, one trip ahead; blocks
// 16 and 32 read the NBS = 128 / BLK blocks of a stage (ED dwords per row), one stage ahead, which keeps their registers down.
template <int BLK, int OUT_DT, int WM, int WN, int TM, int TN, bool SPLIT>
__global__ void __launch_bounds__(64 * WM * WN) k_i8_gemm(const int8_t* __restrict__ xc, const int8_t* __restrict__ xe, const int8_t* __restrict__ wc,
                                                          const int8_t* __restrict__ we, const void* __restrict__ bias, void* __restrict__ out,
                                                          int T, int N, int K, int tiles_t, int tiles, int trips_per_part, int xm, int wm)
{
    using Tile = I8Tile<BLK, WM, WN, TM, TN, SPLIT>;
    constexpr int STAGE = Tile::STAGE;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * STAGE];
    Tile t(T, N, K, tiles_t, tiles, trips_per_part);
    const int ta = t.ta, tb = t.tb;
    const uint32_t* const we32 = reinterpret_cast<const uint32_t*>(we);
    const uint32_t* const xe32 = reinterpret_cast<const uint32_t*>(xe);

    if constexpr (BLK == 64) {
        if (ta < tb) {
            uint32_t ewd[TM][4][1], exd[TN][1];                          // block BB of a trip: byte BB of the trip's dwords
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) ewd[i][j][0] = we32[t.ewo[i][j] + ta];
#pragma unroll
            for (int jt = 0; jt < TN; jt++) exd[jt][0] = xe32[t.exo[jt] + ta];
            t.stage(lds, wc, xc, ta << 8, 0);
            landed();
            for (int tr = ta; tr < tb; tr++) {
                const int trn = tr + 1 < tb ? tr + 1 : tr;               // (last trip: re-reads its own exponents, re-stages its first half)
                uint32_t ewn[TM][4], exn[TN];
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) ewn[i][j] = we32[t.ewo[i][j] + trn];
#pragma unroll
                for (int jt = 0; jt < TN; jt++) exn[jt] = xe32[t.exo[jt] + trn];
                t.stage(lds, wc, xc, (tr << 8) + BK, 1);
                t.block(lds, 0, 0, ewd, exd, 0, 0, xm, wm);
                t.block(lds, 0, 1, ewd, exd, 0, 8, xm, wm);
                landed();
                t.stage(lds, wc, xc, trn << 8, 0);
                t.block(lds, 1, 0, ewd, exd, 0, 16, xm, wm);
                t.block(lds, 1, 1, ewd, exd, 0, 24, xm, wm);
                landed();
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) ewd[i][j][0] = ewn[i][j];
#pragma unroll
                for (int jt = 0; jt < TN; jt++) exd[jt][0] = exn[jt];
            }
        }
    } else {
        constexpr int NBS = BK / BLK, ED = NBS / 4;                  // blocks per stage; exponent dwords per row and stage
        // exponent dwords of stage s (128 bytes of K from s * 128)
        auto exps = [&](int s, uint32_t (&ewd)[TM][4][ED], uint32_t (&exd)[TN][ED]) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int e = 0; e < ED; e++) ewd[i][j][e] = we32[t.ewo[i][j] + s * ED + e];
#pragma unroll
            for (int jt = 0; jt < TN; jt++)
#pragma unroll
                for (int e = 0; e < ED; e++) exd[jt][e] = xe32[t.exo[jt] + s * ED + e];
        };
        // every block of the stage in buffer buf
        auto blocks = [&](int buf, const uint32_t (&ewd)[TM][4][ED], const uint32_t (&exd)[TN][ED]) __attribute__((always_inline)) {
#pragma unroll
            for (int b = 0; b < NBS; b++) t.block(lds, buf, b, ewd, exd, b >> 2, 8 * (b & 3), xm, wm);
        };

        if (ta < tb) {
            uint32_t ewd[TM][4][ED], exd[TN][ED], ewn[TM][4][ED], exn[TN][ED];
            exps(2 * ta, ewd, exd);
            t.stage(lds, wc, xc, ta << 8, 0);
            landed();
            for (int tr = ta; tr < tb; tr++) {
                const int trn = tr + 1 < tb ? tr + 1 : tr;               // (last trip: re-reads its own first stage)
                exps(2 * tr + 1, ewn, exn);
                t.stage(lds, wc, xc, (tr << 8) + BK, 1);
                blocks(0, ewd, exd);
                landed();
                exps(2 * trn, ewd, exd);
                t.stage(lds, wc, xc, trn << 8, 0);
                blocks(1, ewn, exn);
                landed();
            }
        }
    }
    t.template store<OUT_DT>(bias, out, T, N);
}

// few tokens: wave = 16 features x 16 tokens (token group blockIdx.y) x a slice of the blocks; fp32 slab [slice][Tpad][N]; K % BLK == 0
template <int BLK>
__global__ void __launch_bounds__(256) k_i8_decode(const int8_t* __restrict__ wc, const int8_t* __restrict__ we, const int8_t* __restrict__ xc,
                                                   const int8_t* __restrict__ xe, float* __restrict__ slabs, int T, int N, int K,
                                                   int blocks_per_slice, int slices, int wm, int xm)
{
    using B = I8Blk<BLK>;
    using op_t = typename B::op_t;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int row_tiles = N / 16;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int rt = wave % row_tiles, slice = wave / row_tiles;
    if (slice >= slices) return;                                 // grid rounded up to whole workgroups
    const int nb = K / BLK, Tpad = gridDim.y * 16;
    const int b0 = slice * blocks_per_slice;
    const int b1 = b0 + blocks_per_slice < nb ? b0 + blocks_per_slice : nb;
    const int n0 = rt * 16, tok = blockIdx.y * 16 + r;
    const int tx = tok < T ? tok : T - 1;                        // token columns past T repeat the last token (results dropped)
    const int8_t* wrow = wc + (size_t)(n0 + r) * K + B::lane(q);
    const int8_t* xrow = xc + (size_t)tx * K + B::lane(q);
    const int8_t* wer = we + (size_t)(n0 + 4 * q) * nb;
    const int8_t* xer = xe + (size_t)tx * nb;
    const v4i zero = {0, 0, 0, 0};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = b0; b < b1; b++) {
        const op_t av = B::a_live(q) ? *reinterpret_cast<const op_t*>(wrow + (size_t)b * BLK) : op_t{};
        const op_t bv = *reinterpret_cast<const op_t*>(xrow + (size_t)b * BLK);
        const v4i c = B::mfma(av, bv, zero);
        const int xe_b = xer[b];
        const int cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int we_b = wer[(size_t)j * nb + b];
            // -128 marks a NaN block: the pair contributes NaN
            const float sc = (we_b == -128 || xe_b == -128) ? __builtin_nanf("") : ldexpf(1.0f, we_b - wm + xe_b - xm);
            acc[j] += (float)cv[j] * sc;
        }
    }
    *reinterpret_cast<float4*>(slabs + ((size_t)slice * Tpad + blockIdx.y * 16 + r) * N + n0 + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// exponent bytes of two operands -> *flag = 1 when some block's byte is 127 (the saturated top exponent: the only blocks whose 2^e can
// overflow the operand dtype, where a stochastically rounded value may be +-2^m codes).  One thread = 4 bytes of a 4-aligned run;
// the stray bytes of each run's ends are read one by one.  Threads that find nothing store nothing.
__device__ __forceinline__ bool has_top_exp(uint32_t w) { return ((w ^ 0x7f7f7f7fu) - 0x01010101u) & ~(w ^ 0x7f7f7f7fu) & 0x80808080u; }
__global__ void __launch_bounds__(256) k_exp_top_flag(const int8_t* __restrict__ ea, int64_t na, const int8_t* __restrict__ eb, int64_t nb,
                                                      int* __restrict__ flag)
{
    bool hit = false;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    auto run = [&](const int8_t* e, int64_t n) __attribute__((always_inline)) {
        const int64_t mis = (int64_t)((4u - (reinterpret_cast<uintptr_t>(e) & 3u)) & 3u);     // bytes in front of the first aligned word
        const int64_t head = mis < n ? mis : n;
        const int64_t words = (n - head) / 4;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(e + head);
        for (int64_t i = tid; i < words; i += step) hit = hit || has_top_exp(w[i]);
        if (tid < head) hit = hit || e[tid] == 127;
        const int64_t tail0 = head + 4 * words;
        if (tid < n - tail0) hit = hit || e[tail0 + tid] == 127;
    };
    if (ea) run(ea, na);
    if (eb) run(eb, nb);
    if (hit) *flag = 1;
}

// one thread = 8 codes (4 bytes of nibbles -> 8 bytes)
__global__ void __launch_bounds__(256) k_codes4_to_i8(const uint32_t* __restrict__ in, uint2* __restrict__ out, int64_t n_items)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * 256) {
        const uint32_t v = in[i];
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t nib = (v >> (4 * j)) & 15u;
            const uint32_t b = nib >= 8 ? nib + 0xf0u : nib;    // sign-extend the nibble to a byte
            if (j < 4) lo |= b << (8 * j); else hi |= b << (8 * (j - 4));
        }
        out[i] = make_uint2(lo, hi);
    }
}

// tile variants (bfpq_tune key BFPQ_TUNE_I8_VARIANT): 0 = 128 features x 128 tokens, 1 = 128 x 64, 2 = 64 x 64; all 4 waves
constexpr int kI8Variants = 3;
template <int V> struct I8Var;
template <> struct I8Var<0> { static constexpr int WM = 2, WN = 2, TM = 4, TN = 4; };
template <> struct I8Var<1> { static constexpr int WM = 2, WN = 2, TM = 4, TN = 2; };
template <> struct I8Var<2> { static constexpr int WM = 2, WN = 2, TM = 2, TN = 2; };

template <int V> int var_bn() { return 16 * I8Var<V>::WM * I8Var<V>::TM; }
template <int V> int var_bt() { return 16 * I8Var<V>::WN * I8Var<V>::TN; }
int var_tile_n(int v) { return v == 0 ? var_bn<0>() : (v == 1 ? var_bn<1>() : var_bn<2>()); }
int var_tile_t(int v) { return v == 0 ? var_bt<0>() : (v == 1 ? var_bt<1>() : var_bt<2>()); }

template <int BLK, int V, int OUT_DT, bool SPLIT>
void launch_tile(dim3 grid, hipStream_t s, const int8_t* xc, const int8_t* xe, const int8_t* wc, const int8_t* we, const void* bias, void* out,
                 int T, int N, int K, int tiles_t, int tiles, int tpp, int xm, int wm)
{
    using P = I8Var<V>;
    hipLaunchKernelGGL((k_i8_gemm<BLK, OUT_DT, P::WM, P::WN, P::TM, P::TN, SPLIT>), grid, dim3(64 * P::WM * P::WN), 0, s, xc, xe, wc, we, bias,
                       out, T, N, K, tiles_t, tiles, tpp, xm, wm);
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) int bfpq_g_i8_variant = -1;    // -1 = choose; 0..2 force (bfpq_tune, BFPQ_TUNE_I8_VARIANT)
extern "C" __attribute__((visibility("hidden"))) int bfpq_g_i8_parts = 0;       // 0 = choose; >= 1 force (bfpq_tune, BFPQ_TUNE_I8_PARTS)

static bool i8_args_ok(int out_dtype, int w_mant_bits, int x_mant_bits)
{
    return dtype_ok(out_dtype) && i8_mant_ok(w_mant_bits) && i8_mant_ok(x_mant_bits);
}

static bool small_block(int block_size) { return block_size == 16 || block_size == 32; }      // the blocks of the `b` entries

static int64_t i8_tiles(int64_t T, int64_t N, int v)
{
    return ((T + var_tile_t(v) - 1) / var_tile_t(v)) * ((N + var_tile_n(v) - 1) / var_tile_n(v));
}

// The plan.  Block 64: variant 0 past 64 tokens, else 1; K split in parts of at least two trips.  Blocks 16 / 32: a trip holds 4x / 2x
// the matrix and rescale work of block 64 (the tile is VALU-bound on the rescale), so the plan fills the chip first -- the largest tile
// variant with >= 256 tiles, else the smallest, and K split down to one trip per part.
static int i8_variant(int64_t T, int64_t N, int block_size)
{
    if (bfpq_g_i8_variant >= 0 && bfpq_g_i8_variant < kI8Variants) return bfpq_g_i8_variant;
    if (block_size == 64) return T > 64 ? 0 : 1;
    return i8_tiles(T, N, 0) >= 256 ? 0 : (i8_tiles(T, N, 1) >= 256 ? 1 : 2);
}

static int i8_parts(int64_t T, int64_t N, int64_t K, int block_size)
{
    if (!bfpq_hbfp_linear_i8_ok(T, N, K)) return 1;
    const int64_t trips = K / 256;
    if (bfpq_g_i8_parts > 0) return (int)(bfpq_g_i8_parts < trips ? bfpq_g_i8_parts : trips);
    const int64_t min_trips = block_size == 64 ? 2 : 1;           // trips per part
    const int64_t tiles = i8_tiles(T, N, i8_variant(T, N, block_size));
    if (tiles >= 256 || trips < 2 * min_trips) return 1;
    int64_t parts = 512 / tiles;                                  // aim at two workgroups per CU
    if (parts > 8) parts = 8;
    if (parts > trips / min_trips) parts = trips / min_trips;
    return parts < 2 ? 1 : (int)parts;
}

static bool i8_ptrs_ok(const void* xc, const void* xe, const void* wc, const void* we, const void* out, int block_size)
{
    if (!xc || !xe || !wc || !we || !out) return false;
    // LDS-DMA sources: 16-byte aligned codes; vector stores of 4 outputs: 8-byte aligned; exponents read as dwords, two per row and
    // stage at block 16
    const uintptr_t emask = block_size == 16 ? 7u : 3u;
    return aligned16(xc, wc, out) && !((reinterpret_cast<uintptr_t>(xe) | reinterpret_cast<uintptr_t>(we)) & emask);
}

// the tile entries of every block, with (split) or without the K split: checks, the launch and the slab sum
static int i8_tile(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out, bool split,
                   float* slabs, int parts, int64_t T, int64_t N, int64_t K, int block_size, int out_dtype, int wm, int xm, void* stream)
{
    if (!i8_args_ok(out_dtype, wm, xm) || T < 0 || N < 0 || (split && (parts < 1 || parts > 64))) return BFPQ_E_ARG;
    if (T == 0 || N == 0) return 0;
    if (!bfpq_hbfp_linear_i8_ok(T, N, K)) return BFPQ_E_UNSUPPORTED;
    if (!i8_ptrs_ok(xcodes, xexp, wcodes, wexp, out, block_size) || (split && (!slabs || !aligned16(slabs)))) return BFPQ_E_ARG;
    const int v = i8_variant(T, N, block_size), trips = (int)(K / 256);
    if (parts > trips) parts = trips;
    const int tpp = (trips + parts - 1) / parts;
    parts = (trips + tpp - 1) / tpp;                              // (no empty part)
    const int tiles_t = (int)((T + var_tile_t(v) - 1) / var_tile_t(v)), tiles = tiles_t * (int)((N + var_tile_n(v) - 1) / var_tile_n(v));
    const dim3 grid((unsigned)(tiles * (split ? parts : 1)));
    hipStream_t s = (hipStream_t)stream;
    const int8_t *xc = (const int8_t*)xcodes, *wc = (const int8_t*)wcodes;
    with_block(block_size, [&](auto blk) {
        constexpr int BLK = decltype(blk)::value;
        auto go = [&](auto var) {
            if (split) launch_tile<BLK, var, BFPQ_F32, true>(grid, s, xc, xexp, wc, wexp, nullptr, slabs, (int)T, (int)N, (int)K, tiles_t, tiles, tpp, xm, wm);
            else with_dtype(out_dtype, [&](auto dt) {
                launch_tile<BLK, var, dt, false>(grid, s, xc, xexp, wc, wexp, bias, out, (int)T, (int)N, (int)K, tiles_t, tiles, tpp, xm, wm);
            });
        };
        if (v == 0) go(std::integral_constant<int, 0>{});
        else if (v == 1) go(std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, 2>{});
    });
    if (split) launch_slab_reduce(out_dtype, slabs, (size_t)(T * N), bias, out, T * N, N, parts, s);
    return (int)hipGetLastError();
}

static int decode8_slices(int64_t T, int64_t N, int64_t K)
{
    const int64_t nb = K / 64, waves = (N / 16) * ((T + 15) / 16);
    int64_t slices = (4096 + waves - 1) / waves;                  // aim at ~4096 waves on the chip
    if (slices > nb) slices = nb;
    if (slices < 1) slices = 1;
    const int64_t bps = (nb + slices - 1) / slices;
    return (int)((nb + bps - 1) / bps);
}

// the few-token entries of every block.  Every block slices K in whole 64-byte runs (finer slices would multiply the fp32 slab
// traffic, which is what a few-token call pays for).
static int i8_decode(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out, float* slabs,
                     int64_t T, int64_t N, int64_t K, int block_size, int out_dtype, int wm, int xm, void* stream)
{
    if (!i8_args_ok(out_dtype, wm, xm) || T < 1 || N < 1) return BFPQ_E_ARG;
    if (bfpq_hbfp_linear_decode8_ws(T, N, K) < 0) return BFPQ_E_UNSUPPORTED;
    if (!xcodes || !xexp || !wcodes || !wexp || !out || !slabs) return BFPQ_E_ARG;
    if (!aligned16(xcodes, wcodes, slabs)) return BFPQ_E_ARG;
    const int slices = decode8_slices(T, N, K), bps = (int)((K / 64 + slices - 1) / slices) * (64 / block_size);
    const int64_t waves = (N / 16) * slices, groups = (T + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    with_block(block_size, [&](auto blk) {
        hipLaunchKernelGGL(k_i8_decode<blk>, dim3((unsigned)((waves + 3) / 4), (unsigned)groups), dim3(256), 0, s, (const int8_t*)wcodes, wexp,
                           (const int8_t*)xcodes, xexp, slabs, (int)T, (int)N, (int)K, bps, slices, wm, xm);
    });
    // slabs are [slices][Tpad][N]: the first T rows of each slab are the outputs' partial sums
    launch_slab_reduce(out_dtype, slabs, (size_t)(groups * 16 * N), bias, out, T * N, N, slices, s);
    return (int)hipGetLastError();
}

extern "C" {

int bfpq_hbfp_linear_i8_ok(int64_t T, int64_t N, int64_t K)
{
    return T >= 1 && N >= 16 && N % 16 == 0 && K >= 256 && K % 256 == 0 && T * K < ((int64_t)1 << 32) && N * K < ((int64_t)1 << 32) &&
           ((T + 63) / 64) * ((N + 63) / 64) < ((int64_t)1 << 30);
}

int bfpq_hbfp_linear_i8_parts(int64_t T, int64_t N, int64_t K) { return i8_parts(T, N, K, 64); }

int bfpq_hbfp_linear_i8(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out,
                        int64_t T, int64_t N, int64_t K, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream)
{
    return i8_tile(xcodes, xexp, wcodes, wexp, bias, out, false, nullptr, 1, T, N, K, 64, out_dtype, w_mant_bits, x_mant_bits, stream);
}

int bfpq_hbfp_linear_i8_splitk(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out,
                               float* slabs, int parts, int64_t T, int64_t N, int64_t K, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream)
{
    return i8_tile(xcodes, xexp, wcodes, wexp, bias, out, true, slabs, parts, T, N, K, 64, out_dtype, w_mant_bits, x_mant_bits, stream);
}

int64_t bfpq_hbfp_linear_decode8_ws(int64_t T, int64_t N, int64_t K)
{
    if (T < 1 || N < 16 || K < 64 || N % 16 != 0 || K % 64 != 0 || T > 65535 * 16 || N * K >= ((int64_t)1 << 32) || T * K >= ((int64_t)1 << 32))
        return BFPQ_E_UNSUPPORTED;
    return (int64_t)decode8_slices(T, N, K) * ((T + 15) / 16 * 16) * N;
}

int bfpq_hbfp_linear_decode8(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out,
                             float* slabs, int64_t T, int64_t N, int64_t K, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream)
{
    return i8_decode(xcodes, xexp, wcodes, wexp, bias, out, slabs, T, N, K, 64, out_dtype, w_mant_bits, x_mant_bits, stream);
}

// ---- the same entries at blocks 16 and 32 (any other block_size: BFPQ_E_ARG, or 0 from _ok) ---------------------------------------
int bfpq_hbfp_linear_i8b_ok(int64_t T, int64_t N, int64_t K, int block_size)
{
    return small_block(block_size) && bfpq_hbfp_linear_i8_ok(T, N, K);
}

int bfpq_hbfp_linear_i8b_parts(int64_t T, int64_t N, int64_t K, int block_size)
{
    return small_block(block_size) ? i8_parts(T, N, K, block_size) : BFPQ_E_ARG;
}

int bfpq_hbfp_linear_i8b(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out,
                         int64_t T, int64_t N, int64_t K, int block_size, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream)
{
    if (!small_block(block_size)) return BFPQ_E_ARG;
    return i8_tile(xcodes, xexp, wcodes, wexp, bias, out, false, nullptr, 1, T, N, K, block_size, out_dtype, w_mant_bits, x_mant_bits, stream);
}

int bfpq_hbfp_linear_i8b_splitk(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out,
                                float* slabs, int parts, int64_t T, int64_t N, int64_t K, int block_size, int out_dtype, int w_mant_bits,
                                int x_mant_bits, void* stream)
{
    if (!small_block(block_size)) return BFPQ_E_ARG;
    return i8_tile(xcodes, xexp, wcodes, wexp, bias, out, true, slabs, parts, T, N, K, block_size, out_dtype, w_mant_bits, x_mant_bits, stream);
}

int64_t bfpq_hbfp_linear_decode8b_ws(int64_t T, int64_t N, int64_t K, int block_size)
{
    return small_block(block_size) ? bfpq_hbfp_linear_decode8_ws(T, N, K) : BFPQ_E_ARG;
}

int bfpq_hbfp_linear_decode8b(const void* xcodes, const int8_t* xexp, const void* wcodes, const int8_t* wexp, const void* bias, void* out,
                              float* slabs, int64_t T, int64_t N, int64_t K, int block_size, int out_dtype, int w_mant_bits, int x_mant_bits,
                              void* stream)
{
    if (!small_block(block_size)) return BFPQ_E_ARG;
    return i8_decode(xcodes, xexp, wcodes, wexp, bias, out, slabs, T, N, K, block_size, out_dtype, w_mant_bits, x_mant_bits, stream);
}

int bfpq_exp_top_flag(const int8_t* exp_a, int64_t n_a, const int8_t* exp_b, int64_t n_b, int* flag, void* stream)
{
    if (n_a < 0 || n_b < 0 || !flag || (n_a && !exp_a) || (n_b && !exp_b)) return BFPQ_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t h = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (h != hipSuccess) return (int)h;
    const int64_t most = (n_a > n_b ? n_a : n_b) / 4 + 4;
    int64_t g = (most + 255) / 256;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(k_exp_top_flag, dim3((unsigned)g), dim3(256), 0, s, n_a ? exp_a : nullptr, n_a, n_b ? exp_b : nullptr, n_b, flag);
    return (int)hipGetLastError();
}

int bfpq_codes4_to_i8(const void* codes4, void* codes8, int64_t n_codes, void* stream)
{
    if (n_codes < 0 || n_codes % 8 != 0) return BFPQ_E_ARG;
    if (n_codes == 0) return 0;
    if (!codes4 || !codes8 || (reinterpret_cast<uintptr_t>(codes4) & 3u) || (reinterpret_cast<uintptr_t>(codes8) & 7u)) return BFPQ_E_ARG;
    const int64_t items = n_codes / 8;
    int64_t g = (items + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_codes4_to_i8, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)codes4, (uint2*)codes8, items);
    return (int)hipGetLastError();
}

}  // extern "C"
