// bfpq_kvcache.hip -- attention keys and values held as HBFP codes across decode steps (bfp_ops.HBFPKVCache).
//
// The reference's GPT-2 decodes with layer_past (modeling_gpt2.py:345-348, 415-419): every step concatenates the new key and value onto
// the past ones and F_matmul_bfp (bfp_ops.py:240-245 through :187-190, :153) quantizes ALL of K along D and, after a transposed copy, ALL
// of V along S again.  Here the codes are kept: a step quantizes the one new token and multiplies straight from the cache.
//
// Format (per head b < B H): k_codes [cap, ldd] int8 + k_exps [cap, D / block] (blocks along D: a key row is final once appended);
// v_codes [D, cap] int8 + v_exps [D, cap / block] (blocks along the tokens) and v_tail [block, D] of the dtype, the original values of
// the one token block that is still open.  The open block's shared exponent can rise with every token, and rounding codes that were
// already rounded is a double rounding, so that block is quantized again FROM v_tail at every append, absent tokens as zeros -- which
// is the reference's zero pad of a ragged last block (bfp_ops.py:50-53).  A closed block is never touched again.
//
// k_kv_append: one launch for any t >= 1.  Its first workgroups quantize the t key rows (a thread per 16 elements, the block maximum
// over 1, 2 or 4 neighbour lanes); the others own one 64-column slice of V and one token block each: rows below pos come from v_tail,
// rows of the chunk from v_new (and go to v_tail where the block stays open), the rest are zeros; the block x 64 tile goes through
// LDS as in k_codes_t (bfpq_bmm.hip), the scale and the codes are block_scale / quant_elem of bfpq_common.h.  The workgroup of the
// chunk's first block also does its last one, after a barrier: those are the only two that touch v_tail (read, then write).
//
// k_kv_bmm_dec: out[b][t][n] = sum_k x[b][t][k] w[b][n][k] for t < Tq <= 16, x in its float dtype and quantized in the kernel block by
// block as the walk reaches it (a lane holds the 16 or 8 elements of its MFMA operand; the block maximum over the four lanes of a
// token; elements past Kx count as zeros), w a cached operand.  Family qk: w = k_codes, n the S cached keys, k = D.  Family pv:
// w = v_codes, n = D, k the S cached tokens (the last block ragged: zero codes on the cache side, zeros on x's).  The block product,
// the rescale, the NaN marker and the lane map are bfpq_i8mma.h; blocks are added in block order, so on the same codes the result is
// k_bmm_i8's bit for bit.  Rows past Nout repeat the last row (never stored); a lane stores four consecutive n of one token, so the
// output has a pitch ldo (a multiple of 4).  The next 64-byte chunk of w, its exponents and x's elements are loaded before the current
// one is multiplied.  No split of the contraction: pv at batch 1 runs B H D / 64 workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfpq.h"
#include "bfpq_common.h"
#include "bfpq_device.h"
#include "bfpq_i8mma.h"

using namespace bfpq;

namespace {

constexpr int kTD = 64;                                   // columns of V per workgroup
constexpr int kPitch = kTD + 1;                           // words per token row of the value tile

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// one token block tb of one 64-column slice of V
template <int DT>
__device__ __forceinline__ void v_block(const typename Traits<DT>::raw_t* __restrict__ vnew, typename Traits<DT>::raw_t* __restrict__ tail,
                                        int8_t* __restrict__ vcodes, int8_t* __restrict__ vexps, int bh, int tb, int d0, int D, int pos, int t,
                                        int cap, int block, int mant_bits, float eps_dt, const uint8_t* s_win, uint32_t* s_val, uint32_t* s_max)
{
    using Tr = Traits<DT>;
    constexpr int VEC = Tr::VEC, LPR = kTD / VEC, RPP = 256 / LPR;
    const int tid = threadIdx.x;
    const bool open = (tb + 1) * block > pos + t;                         // the block is still open after this call
    for (int p = 0; p < 64 / RPP; p++) {
        const int row = p * RPP + tid / LPR, col = (tid % LPR) * VEC;
        if (row >= block) break;
        const int s = tb * block + row;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (d0 + col < D) {
            const size_t to = ((size_t)bh * block + row) * D + d0 + col;
            if (s < pos) v = *reinterpret_cast<const uint4*>(tail + to);
            else if (s < pos + t) {
                v = *reinterpret_cast<const uint4*>(vnew + ((size_t)bh * t + (s - pos)) * D + d0 + col);
                if (open) *reinterpret_cast<uint4*>(tail + to) = v;
            }
        }
        uint32_t* const dst = s_val + row * kPitch + col;
        if constexpr (VEC == 4) {
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        } else {
            dst[0] = v.x & 0xffffu; dst[1] = v.x >> 16; dst[2] = v.y & 0xffffu; dst[3] = v.y >> 16;
            dst[4] = v.z & 0xffffu; dst[5] = v.z >> 16; dst[6] = v.w & 0xffffu; dst[7] = v.w >> 16;
        }
    }
    __syncthreads();
    const int d = tid & 63, sq = tid >> 6, per = block >> 2;              // this thread's column and its `per` tokens
    uint32_t raw[16], mx = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        raw[i] = i < per ? s_val[(sq * per + i) * kPitch + d] : 0u;
        mx = umax(mx, raw[i] & Tr::ABS);
    }
    s_max[sq * kTD + d] = mx;
    __syncthreads();
    for (int o = 0; o < 4; o++) mx = umax(mx, s_max[o * kTD + d]);
    const BlockScale bs = block_scale<DT>(mx, mant_bits, eps_dt, s_win);
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        float c = 0.f;
        if (i < per) quant_elem<DT>(raw_to_f32<DT>(raw[i]), bs, false, 0.f, &c);
        pk[i >> 2] |= ((uint32_t)(int)c & 0xffu) << (8 * (i & 3));
    }
    if (d0 + d < D) {
        int8_t* const dst = vcodes + ((size_t)bh * D + d0 + d) * cap + tb * block + sq * per;
        if (per == 16) *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        else if (per == 8) *reinterpret_cast<uint2*>(dst) = make_uint2(pk[0], pk[1]);
        else *reinterpret_cast<uint32_t*>(dst) = pk[0];
        if (sq == 0) vexps[((size_t)bh * D + d0 + d) * (cap / block) + tb] = sat_exp(bs);
    }
}

template <int DT>
__global__ void __launch_bounds__(256) k_kv_append(const void* __restrict__ knew, const void* __restrict__ vnew, int8_t* __restrict__ kcodes,
                                                   int8_t* __restrict__ kexps, int8_t* __restrict__ vcodes, int8_t* __restrict__ vexps,
                                                   void* __restrict__ vtail, int BH, int D, int pos, int t, int cap, int ldd, int block,
                                                   int mant_bits, float eps_dt, const uint8_t* __restrict__ exp_win, int nkb, int zc)
{
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    __shared__ uint32_t s_val[64 * kPitch];
    __shared__ uint32_t s_max[4 * kTD];
    const int tid = threadIdx.x;
    for (int i = tid; i < BFPQ_EXP_WIN_ENTRIES; i += 256) s_win[i] = exp_win[i];
    __syncthreads();
    if ((int)blockIdx.x < nkb) {
        // keys: a thread per 16 elements of a row, blocks along D
        const int segs = D >> 4, per = block >> 4;
        const int64_t total = (int64_t)BH * t * segs;
        const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
        const bool valid = idx < total;                                   // (total % per == 0: the lanes of a block are valid together)
        const int64_t it = valid ? idx : total - 1;
        const int seg = (int)(it % segs);
        const int64_t row = it / segs;                                    // bh * t + i
        const int bh = (int)(row / t), i = (int)(row % t);
        const raw_t* const src = reinterpret_cast<const raw_t*>(knew) + (size_t)row * D + seg * 16;
        uint32_t raw[16], mx = 0;
#pragma unroll
        for (int v = 0; v < 16 / Tr::VEC; v++) bfpq_dev::load_raw_vec<DT>(src, v, raw + v * Tr::VEC);
#pragma unroll
        for (int e = 0; e < 16; e++) mx = umax(mx, raw[e] & Tr::ABS);
        if (per >= 2) mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 1, 64));
        if (per >= 4) mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 2, 64));
        const BlockScale bs = block_scale<DT>(mx, mant_bits, eps_dt, s_win);
        uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; e++) {
            float c;
            quant_elem<DT>(raw_to_f32<DT>(raw[e]), bs, false, 0.f, &c);
            pk[e >> 2] |= ((uint32_t)(int)c & 0xffu) << (8 * (e & 3));
        }
        if (valid) {
            const size_t r = (size_t)bh * cap + pos + i;
            *reinterpret_cast<uint4*>(kcodes + r * ldd + seg * 16) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            if (seg % per == 0) kexps[r * (D / block) + seg / per] = sat_exp(bs);
        }
        return;
    }
    // values: workgroup (bh, 64-column slice, z); z = 0 does the chunk's first block and then its last, z >= 1 the block first + z
    const int dtiles = (D + kTD - 1) / kTD;
    const int vb = (int)blockIdx.x - nkb;
    const int z = vb % zc, dt = (vb / zc) % dtiles, bh = vb / (zc * dtiles);
    const int first = pos / block, last = (pos + t - 1) / block;
    const int n = (z == 0 && last != first) ? 2 : 1;
    for (int it = 0; it < n; it++) {
        if (it) __syncthreads();                                          // (the first block's tile and tail rows have been read)
        v_block<DT>(reinterpret_cast<const raw_t*>(vnew), reinterpret_cast<raw_t*>(vtail), vcodes, vexps, bh, it ? last : first + z, dt * kTD, D,
                    pos, t, cap, block, mant_bits, eps_dt, s_win, s_val, s_max);
    }
}

// ---- the decode product -----------------------------------------------------------------------------------------------------------
template <int BLK, int DT, int TM>
__global__ void __launch_bounds__(256) k_kv_bmm_dec(const void* __restrict__ x, const int8_t* __restrict__ wc, const int8_t* __restrict__ we,
                                                    void* __restrict__ out, int B, int Tq, int Kx, int Nout, int ldx, int ldw, int ldwe, int wbs,
                                                    int ldo, int xm, int wm, float eps_dt, const uint8_t* __restrict__ exp_win)
{
    using Blk = I8Blk<BLK>;
    using op_t = typename Blk::op_t;
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    constexpr int NBS = 64 / BLK;                                // blocks per 64-byte chunk
    constexpr int NE = BLK == 64 ? 16 : 8;                       // a lane's bytes of a block
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    for (int i = threadIdx.x; i < BFPQ_EXP_WIN_ENTRIES; i += 256) s_win[i] = exp_win[i];
    __syncthreads();
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 15, q = l >> 4;
    const int n0 = ((int)blockIdx.x * 4 + w) * 16 * TM;
    if (n0 >= Nout) return;                                      // (wave-uniform; no barrier below)
    const int nb = (Kx + BLK - 1) / BLK, nch = (Kx + 63) >> 6;
    const bool tok = r < Tq;

    uint32_t offW[TM], ewo[TM][4];
#pragma unroll
    for (int i = 0; i < TM; i++) {
        const int n = n0 + 16 * i + r;
        offW[i] = (uint32_t)(n < Nout ? n : Nout - 1) * (uint32_t)ldw + Blk::lane(q);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int ne = n0 + 16 * i + 4 * q + j;
            ewo[i][j] = (uint32_t)(ne < Nout ? ne : Nout - 1) * (uint32_t)ldwe;
        }
    }
    const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};

    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int8_t* const wcb = wc + (size_t)b * wbs * ldw;
        const int8_t* const web = we + (size_t)b * wbs * ldwe;
        const raw_t* const xr = reinterpret_cast<const raw_t*>(x) + ((size_t)b * Tq + (tok ? r : 0)) * ldx;

        // chunk c: the lane's w codes, the exponents of its four output rows (byte s of a word = block s of the chunk) and its x elements
        auto load = [&](int c, op_t (&aF)[TM][NBS], uint32_t (&ew)[TM][4], uint32_t (&xv)[NBS][NE]) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; i++) {
#pragma unroll
                for (int s = 0; s < NBS; s++) {
                    aF[i][s] = *reinterpret_cast<const op_t*>(wcb + offW[i] + (c << 6) + s * BLK);
                    if (!Blk::a_live(q)) aF[i][s] = op_t{};
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t v = 0;
#pragma unroll
                    for (int s = 0; s < NBS; s++)
                        if (c * NBS + s < nb) v |= (uint32_t)(uint8_t)web[ewo[i][j] + c * NBS + s] << (8 * s);
                    ew[i][j] = v;
                }
            }
#pragma unroll
            for (int s = 0; s < NBS; s++)
#pragma unroll
                for (int e = 0; e < NE; e++) {
                    const int k = (c << 6) + s * BLK + Blk::lane(q) + e;
                    xv[s][e] = (tok && k < Kx) ? (uint32_t)xr[k] : 0u;
                }
        };

        v2f acc[TM][2];
#pragma unroll
        for (int i = 0; i < TM; i++) acc[i][0] = acc[i][1] = v2f{0.f, 0.f};

        op_t aF[TM][NBS], aN[TM][NBS];
        uint32_t ew[TM][4], ewN[TM][4], xv[NBS][NE], xN[NBS][NE];
        load(0, aF, ew, xv);
#pragma unroll 1
        for (int c = 0; c < nch; c++) {
            if (c + 1 < nch) load(c + 1, aN, ewN, xN);
#pragma unroll
            for (int s = 0; s < NBS; s++) {
                if (c * NBS + s < nb) {                          // (wave-uniform)
                    // x's block: the maximum over the four lanes of the token, the dtype-exact scale, the lane's codes
                    uint32_t mx = 0;
#pragma unroll
                    for (int e = 0; e < NE; e++) mx = umax(mx, xv[s][e] & Tr::ABS);
                    mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 16, 64));
                    mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 32, 64));
                    const BlockScale bs = block_scale<DT>(mx, xm, eps_dt, s_win);
                    uint32_t pk[NE / 4];
#pragma unroll
                    for (int e = 0; e < NE / 4; e++) pk[e] = 0u;
#pragma unroll
                    for (int e = 0; e < NE; e++) {
                        float cd;
                        quant_elem<DT>(raw_to_f32<DT>(xv[s][e]), bs, false, 0.f, &cd);
                        pk[e >> 2] |= ((uint32_t)(int)cd & 0xffu) << (8 * (e & 3));
                    }
                    op_t bF;
                    if constexpr (BLK == 64) bF = v4i{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
                    else bF = (long)(((uint64_t)pk[1] << 32) | pk[0]);
                    v2f sx, nm;
                    token_scale((int)sat_exp(bs), xm, sx, nm);
                    const int sh = 8 * s;
#pragma unroll
                    for (int i = 0; i < TM; i++) {
                        const v2f sw01 = v2f{pow2_scale(exp_byte(ew[i][0], sh), wm), pow2_scale(exp_byte(ew[i][1], sh), wm)};
                        const v2f sw23 = v2f{pow2_scale(exp_byte(ew[i][2], sh), wm), pow2_scale(exp_byte(ew[i][3], sh), wm)};
                        rescale(Blk::mfma(aF[i][s], bF, magic), sx, nm, sw01, sw23, acc[i][0], acc[i][1]);
                    }
                }
            }
            if (c + 1 < nch) {
#pragma unroll
                for (int i = 0; i < TM; i++) {
#pragma unroll
                    for (int s = 0; s < NBS; s++) aF[i][s] = aN[i][s];
#pragma unroll
                    for (int j = 0; j < 4; j++) ew[i][j] = ewN[i][j];
                }
#pragma unroll
                for (int s = 0; s < NBS; s++)
#pragma unroll
                    for (int e = 0; e < NE; e++) xv[s][e] = xN[s][e];
            }
        }

        // the lane holds rows n .. n + 3 of token r (the pitch ldo takes the ones past Nout)
        if (tok) {
#pragma unroll
            for (int i = 0; i < TM; i++) {
                const int n = n0 + 16 * i + 4 * q;
                if (n < Nout) store4<DT>(out, ((size_t)b * Tq + r) * ldo + n, acc[i][0], acc[i][1]);
            }
        }
    }
}

constexpr int64_t kLim = (int64_t)1 << 31;

}  // namespace

extern "C" {

int bfpq_kv_ok(int64_t D, int64_t cap, int block_size)
{
    return i8_block_ok(block_size) && D >= 16 && D % 16 == 0 && D % block_size == 0 && D <= 1024 && cap >= 64 && cap % 64 == 0 &&
           D * cap < kLim;
}

int bfpq_kv_append(const void* k_new, const void* v_new, void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail, int64_t BH,
                   int64_t D, int64_t pos, int64_t t, int64_t cap, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon,
                   const uint8_t* exp_win, void* stream)
{
    if (!dtype_ok(dtype) || !i8_block_ok(block_size) || !i8_mant_ok(mant_bits) || BH < 0 || t < 0 || pos < 0) return BFPQ_E_ARG;
    if (!bfpq_kv_ok(D, cap, block_size) || ldd < D || ldd % 64 != 0 || pos + t > cap || BH >= kLim) return BFPQ_E_UNSUPPORTED;
    if (BH == 0 || t == 0) return 0;
    if (!k_new || !v_new || !k_codes || !k_exps || !v_codes || !v_exps || !v_tail || !exp_win ||
        !aligned16(k_new, v_new, k_codes, v_codes, v_tail))
        return BFPQ_E_ARG;
    const int64_t nkb = (BH * t * (D / 16) + 255) / 256;
    const int64_t nblk = (pos + t - 1) / block_size - pos / block_size + 1, zc = nblk > 1 ? nblk - 1 : 1;
    const int64_t nvb = BH * ((D + kTD - 1) / kTD) * zc;
    if (nkb + nvb >= kLim) return BFPQ_E_UNSUPPORTED;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    with_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_kv_append<decltype(dt)::value>), dim3((unsigned)(nkb + nvb)), dim3(256), 0, (hipStream_t)stream, k_new, v_new,
                           (int8_t*)k_codes, k_exps, (int8_t*)v_codes, v_exps, v_tail, (int)BH, (int)D, (int)pos, (int)t, (int)cap, (int)ldd,
                           block_size, mant_bits, eps_dt, exp_win, (int)nkb, (int)zc);
    });
    return (int)hipGetLastError();
}

int bfpq_kv_bmm_dec(const void* x, const void* wcodes, const int8_t* wexp, void* out, int64_t B, int64_t Tq, int64_t Kx, int64_t Nout,
                    int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo, int family, int dtype, int block_size,
                    int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* stream)
{
    if (!dtype_ok(dtype) || !i8_block_ok(block_size) || !i8_mant_ok(x_mant_bits) || !i8_mant_ok(w_mant_bits) ||
        (family != BFPQ_KV_QK && family != BFPQ_KV_PV) || B < 0 || Tq < 0 || Nout < 0 || Kx < 0)
        return BFPQ_E_ARG;
    if (B == 0 || Tq == 0 || Nout == 0) return 0;
    const int64_t nb = (Kx + block_size - 1) / block_size;
    if (Tq > BFPQ_KV_DEC_MAX_TOKENS || Kx < 1 || (family == BFPQ_KV_QK ? Kx % block_size != 0 : Nout % 16 != 0) || ldx < Kx || ldw % 64 != 0 ||
        ldw < (Kx + 63) / 64 * 64 || ldwe < nb || w_bstride < Nout || ldo % 4 != 0 || ldo < Nout || w_bstride * ldw >= kLim ||
        w_bstride * ldwe >= kLim || Tq * ldx >= kLim || Tq * ldo >= kLim)
        return BFPQ_E_UNSUPPORTED;
    if (!x || !wcodes || !wexp || !out || !exp_win || !aligned16(wcodes, out) || (reinterpret_cast<uintptr_t>(x) & (dtype == BFPQ_F32 ? 3u : 1u)))
        return BFPQ_E_ARG;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    hipStream_t s = (hipStream_t)stream;
    const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
    with_block(block_size, [&](auto blk) {
        with_dtype(dtype, [&](auto dt) {
            auto go = [&](auto tmc) {
                constexpr int TM = decltype(tmc)::value;
                hipLaunchKernelGGL((k_kv_bmm_dec<decltype(blk)::value, decltype(dt)::value, TM>), dim3((unsigned)((Nout + 64 * TM - 1) / (64 * TM)), gy),
                                   dim3(256), 0, s, x, (const int8_t*)wcodes, wexp, out, (int)B, (int)Tq, (int)Kx, (int)Nout, (int)ldx, (int)ldw,
                                   (int)ldwe, (int)w_bstride, (int)ldo, x_mant_bits, w_mant_bits, eps_dt, exp_win);
            };
            // rows per wave: 64 (32 at the small blocks) of the many cached keys, 16 of V's D columns
            if (family == BFPQ_KV_PV) go(std::integral_constant<int, 1>{});
            else if constexpr (decltype(blk)::value == 64) go(std::integral_constant<int, 4>{});
            else go(std::integral_constant<int, 2>{});
        });
    });
    return (int)hipGetLastError();
}

}  // extern "C"
