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
// Every kernel quantizes with the same steps, each written once below: quant_operand (a token's block of x -> its int8 MFMA operand:
// the block maximum over the token's four lanes, block_scale, pack_codes of bfpq_i8mma.h) and, for the softmax, row_stats (a row's
// maximum and sum, in an order that depends on the row alone), form_p (p of a lane's elements, rounded once) and att_scores (what the
// softmax reads of a score).  The bit-for-bit laws of DESIGN 5k-5n are these helpers being the only copy.
//
// k_kv_append: one launch for any t >= 1.  Its first workgroups quantize the t key rows (a thread per 16 elements, the block maximum
// over 1, 2 or 4 neighbour lanes); the others own one 64-column slice of V and one token block each (v_block): rows below pos come from
// v_tail, rows of the chunk from v_new (and go to v_tail where the block stays open), the rest are zeros; the block x 64 tile goes
// through LDS as in k_codes_t (bfpq_bmm.hip).  The workgroup of the chunk's first block also does its last one, after a barrier: those
// are the only two that touch v_tail (read, then write).
//
// k_kv_bmm_dec: out[b][t][n] = sum_k x[b][t][k] w[b][n][k] for t < Tq <= 16, x in its float dtype and quantized block by block as the
// walk reaches it (quant_operand; elements past Kx count as zeros), w a cached operand.  Family qk: w = k_codes, n the S cached keys,
// k = D.  Family pv: w = v_codes, n = D, k the S cached tokens (the last block ragged: zero codes on the cache side, zeros on x's).
// The block product, the rescale, the NaN marker and the lane map are bfpq_i8mma.h; blocks are added in block order, so on the same
// codes the result is k_bmm_i8's bit for bit.  Rows past Nout repeat the last row (never stored); a lane stores four consecutive n of
// one token, so the output has a pitch ldo (a multiple of 4).  The next 64-byte chunk of w, its exponents and x's elements are loaded
// before the current one is multiplied.  No split of the contraction: pv at batch 1 runs B H D / 64 workgroups.
//
// bfpq_kv_attend: scores, scale, softmax and context of one decode step in three launches.  k_kv_bmm_dec<.., kAtt> leaves
// att_scores as fp32 rows in a workspace; k_kv_pv_split<.., true> runs row_stats on the head's rows in every workgroup of the head, then
// form_p and quant_operand on its own slice, in registers; k_kv_pv_combine is the one context() runs.
//
// Grouped-query attention (the reference's LLaMA, modeling_llama.py:385-409): the cache holds B x kv_heads heads and query
// head h reads kv head h / g (repeat_kv, :264-273).  Nothing is repeated: the rows of a kv head are the contiguous view
// [B kv_heads, R = g Tq, .] of q / p / the outputs, row r being query head r / Tq of the group and its token t = r % Tq, and the GRP
// instances of k_kv_bmm_dec and k_kv_pv_split walk them in tiles of 16 consecutive rows that share every load of the K / V codes and
// exponents (a further tile is an iteration of k_kv_bmm_dec's y loop or a workgroup of k_kv_pv_split, and reads them again).  The
// result is, bit for bit, that of a cache of B x heads heads fed repeat_kv(k), repeat_kv(v): repeated heads hold identical codes, and
// nothing the helpers compute for a row depends on which rows share its tile.  Only att_visible needs the token, t = r % Tq.
//
// Prompt attention (modeling_gpt2.py:207-243 / modeling_llama.py:397-409 for the Tq tokens of a prompt or a chunk of one):
// bfpq_kv_attend_rows walks `rows` query tokens from row0 on in two launches.  The rows of a kv head in a panel are its group segments
// of `rows` tokens, panel row pr = query head pr / rows of the group, token row0 + pr % rows; a workgroup owns 64 consecutive panel
// rows, a 16-row tile per wave.  k_kv_qk_rows: quant_operand on its rows of q once, into LDS, then tiles of 64 keys that go through LDS
// once for the four waves, att_scores into the fp32 panel.  k_kv_pv_rows: row_stats, then form_p, quant_operand and the rescale of
// every token block in block order into fp32 accumulators that hold all D columns.  No block sums, no combine pass.
//
// A first visible key per row (left-padded batches, modeling_gpt2.py:228-230 / modeling_llama.py:402-404, and the
// sliding_window of modeling_attn_mask_utils.py): the WIN instances of the four attend kernels, behind bfpq_kv_attend_gqa_win and
// bfpq_kv_attend_rows_win.  A row sees the keys att_first <= n < att_visible.  att_scores, row_stats and form_p leave out what lies below
// the first key -- the bits of the row with -inf there -- and the kernels skip the key tiles, slices and token blocks below every first
// key of a tile, a wave or a workgroup, a skipped block of p leaving the term of a zero block.  The instances without WIN never read
// `starts` and `window` and are the code they were.
//
// A paged cache: the PG instances behind the bfpq_kv_*_paged entries.  The four code and exponent tensors are a pool of
// pages -- a page: P tokens (a multiple of 64) of all kv heads of one sequence, so seen through one kv head a contiguous head of
// capacity P -- and sequence b's token s lies in page page_table[b][s / P].  The kernels get P for `cap` and take the head's base from
// head_at, the one copy of the lookup; tiles, chunks and token blocks never straddle a page, so the entry is fetched once per unit
// (head_tile: as a scalar) and the next unit's ahead of this unit's loads.  v_tail stays per sequence.  An entry outside the pool is
// refused by the append (seq_take_at) and clamped by head_at; it is never dereferenced.  The instances without PG never read the
// descriptor and are the code they were.
//
// 4-bit codes: the C4 instances behind the bfpq_kv_*_cb entries, block 64 of the device-length modes.  For mant_bits <= 3
// the two code tensors hold two codes to a byte (the layout of PackedBFP); the append stores whole bytes, the products load half the
// bytes and widen them to the int8 operand in registers (k_kv_bmm_dec keeps the prefetched chunk packed; the panel kernels widen on
// the way into LDS), and from the MFMA on a C4 instance is its int8 twin's code on the same integers.  The instances without C4 are
// the code they were.
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

// ---- the steps every kernel below shares: each is written here once ----------------------------------------------------------------------
// the exponent window table into LDS, by the 256 threads of a workgroup (no barrier)
__device__ __forceinline__ void load_exp_win(uint8_t* s_win, const uint8_t* __restrict__ exp_win)
{
    for (int i = threadIdx.x; i < BFPQ_EXP_WIN_ENTRIES; i += 256) s_win[i] = exp_win[i];
}

// the tokens a head of `len` contracts over, or the keys it has, where the caller reaches L of them
__device__ __forceinline__ int clamp_len(int len, int L) { return len < L ? (len > 0 ? len : 0) : L; }

// ---- a paged cache: the cache tensors are a pool of pages, a page being `tokens` consecutive tokens of all `heads` kv heads
// of one sequence, and sequence b's token s lies in page table[b][s / tokens].  The PG instances take the head's base from head_at; the
// others never read the descriptor and are the code they were
struct Pages {
    const int32_t* table;                                     // page_table [sequences, width] int32, read at launch; -1: no page
    int width, tokens, count;                                 // entries per sequence, tokens per page (a multiple of 64), pages in the pool
};

// sequence b's table entry e as it stands (e clamped into the row)
__device__ __forceinline__ int page_entry(const Pages& pg, int b, int e)
{
    return pg.table[(size_t)b * pg.width + (e < pg.width ? (e > 0 ? e : 0) : pg.width - 1)];
}
__device__ __forceinline__ bool page_ok(const Pages& pg, int p) { return p >= 0 && p < pg.count; }

// head_at: where token s of head bh (kv head bh % heads of sequence bh / heads) lies -- the head of capacity `tokens` that holds it (a
// page seen through one kv head) and, in sl, its token there.  Without PG: the head itself and s.  The only copy of the lookup: an entry
// outside 0 .. count - 1 is clamped into the pool before use (append refuses such a token and the products walk tokens below the
// length only, so this guards a table the caller corrupted)
template <bool PG> __device__ __forceinline__ int head_at(const Pages& pg, int bh, int heads, int s, int& sl)
{
    if constexpr (!PG) {
        sl = s;
        return bh;
    } else {
        const int b = bh / heads, e = s / pg.tokens;             // (one division each: the remainders by a multiplication)
        const int p = page_entry(pg, b, e);
        sl = s - e * pg.tokens;
        return (p < 0 ? 0 : (p < pg.count ? p : pg.count - 1)) * heads + (bh - b * heads);
    }
}

// head_at for a wave whose lanes ask for one (head, token): a 64-key tile, a slice's chunk, a token block -- none straddles a page.  The
// entry is fetched once, as a scalar
template <bool PG> __device__ __forceinline__ int head_tile(const Pages& pg, int bh, int heads, int s, int& sl)
{
    if constexpr (!PG) return head_at<false>(pg, bh, heads, s, sl);
    else return head_at<true>(pg, __builtin_amdgcn_readfirstlane(bh), heads, __builtin_amdgcn_readfirstlane(s), sl);
}

// the magnitude maximum of a lane's raw elements
template <int DT, int NE> __device__ __forceinline__ uint32_t abs_max(const uint32_t (&xv)[NE])
{
    uint32_t mx = 0;
#pragma unroll
    for (int e = 0; e < NE; e++) mx = umax(mx, xv[e] & Traits<DT>::ABS);
    return mx;
}

// quant_operand: a token's block as the B operand of I8Blk<BLK>::mfma.  xv: the lane's NE elements of the block (I8Blk::lane), mx their
// abs_max.  The block maximum is taken over the token's four lanes (l & 15 alike), the scale is block_scale's, the codes quant_elem's
// (pack_codes).  bs is the block's scale: its sat_exp is the exponent byte, token_scale makes the rescale's factors of it
template <int BLK, int DT, int NE>
__device__ __forceinline__ typename I8Blk<BLK>::op_t quant_operand(const uint32_t (&xv)[NE], uint32_t mx, int xm, float eps_dt, const uint8_t* s_win,
                                                                   BlockScale& bs)
{
    static_assert(NE == (BLK == 64 ? 16 : 8), "a lane's bytes of a block");
    mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 16, 64));
    mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 32, 64));
    bs = block_scale<DT>(mx, xm, eps_dt, s_win);
    uint32_t pk[NE / 4];
    pack_codes<DT>(xv, NE, bs, pk);
    if constexpr (BLK == 64) return v4i{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
    else return (long)(((uint64_t)pk[1] << 32) | pk[0]);
}

// ---- 4-bit codes (the C4 instances): with mant_bits <= 3 a code lies in -7..7 and the two code tensors hold two to a byte --
// element 2 k of a key row (of a V column: token 2 k) in the low nibble of byte k, 2 k + 1 in its high nibble, two's complement: the
// layout of PackedBFP and native.dequantize(.., code_bits=4).  Every offset the kernels form counts codes; a C4 instance halves it where
// it becomes an address (each is even).  A lane's 16 codes of a block are 8 bytes as loaded and become the int8 cache's MFMA operand in
// registers (widen), so from the MFMA on a C4 instance is its int8 twin's code on the same integers.  A byte is written whole by one
// thread (narrow): nothing reads, modifies and writes one.  Block 64 and the device-length modes only; the instances without C4 never
// see any of this and are the code they were
__device__ __forceinline__ v4i widen(uint2 p)
{
    const v2i a = nibbles_to_i8(p.x), b = nibbles_to_i8(p.y);
    return v4i{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ v4i widen(v4i a) { return a; }        // (the int8 cache: the operand as loaded)
__device__ __forceinline__ long widen(long a) { return a; }
// the 16 codes at code offset off of a 4-bit code tensor, widened
__device__ __forceinline__ v4i load_c4(const int8_t* __restrict__ codes, size_t off)
{
    return widen(*reinterpret_cast<const uint2*>(codes + (off >> 1)));
}
// 16 int8 codes, four to a word (pack_codes), as their 8 bytes of nibbles
__device__ __forceinline__ uint2 narrow(const uint32_t (&pk)[4]) { return make_uint2(i8_to_nibbles(pk[0], pk[1]), i8_to_nibbles(pk[2], pk[3])); }

// one token block tb of one 64-column slice of V
template <int DT, bool PG, bool C4>
__device__ __forceinline__ void v_block(const typename Traits<DT>::raw_t* __restrict__ vnew, typename Traits<DT>::raw_t* __restrict__ tail,
                                        int8_t* __restrict__ vcodes, int8_t* __restrict__ vexps, int bh, int tb, int d0, int D, int pos, int t,
                                        int tn, int cap, int block, int mant_bits, float eps_dt, const uint8_t* s_win, uint32_t* s_val, uint32_t* s_max,
                                        const Pages& pg, int heads)
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
                v = *reinterpret_cast<const uint4*>(vnew + ((size_t)bh * tn + (s - pos)) * D + d0 + col);
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
    uint32_t pk[4];
    pack_codes<DT>(raw, per, bs, pk);
    size_t hb = bh;                                                       // the head the block's codes lie in, and the block there
    int tbl = tb;
    if constexpr (PG) {                                                   // (the block's page: cap is the page's tokens)
        int sl;
        hb = head_tile<true>(pg, bh, heads, tb * block, sl);
        tbl = sl / block;
    }
    if (d0 + d < D) {
        int8_t* const dst = vcodes + (C4 ? ((hb * D + d0 + d) * cap + tbl * block + sq * per) >> 1 : (hb * D + d0 + d) * cap + tbl * block + sq * per);
        if constexpr (C4) *reinterpret_cast<uint2*>(dst) = narrow(pk);   // (block 64: per == 16, the thread's 16 tokens are 8 whole bytes)
        else if (per == 16) *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        else if (per == 8) *reinterpret_cast<uint2*>(dst) = make_uint2(pk[0], pk[1]);
        else *reinterpret_cast<uint32_t*>(dst) = pk[0];
        if (sq == 0) vexps[(hb * D + d0 + d) * (cap / block) + tbl] = sat_exp(bs);
    }
}

// what sequence b of a device-length cache takes of a chunk of t rows: its position and count, or count -1 where it is refused (a count
// outside 0..t, a length outside 0..limit, or tokens past limit): such a sequence is left as it is and the overflow flag is raised
__device__ __forceinline__ int seq_take(const int32_t* __restrict__ lens, const int32_t* __restrict__ counts, int b, int t, int limit, int& pos)
{
    pos = lens[b];
    const int n = counts ? counts[b] : t;
    return (n < 0 || n > t || pos < 0 || pos > limit || n > limit - pos) ? -1 : n;
}

// seq_take on a paged cache: a sequence is refused as well where one of the tokens it would take has no page
template <bool PG>
__device__ __forceinline__ int seq_take_at(const Pages& pg, const int32_t* __restrict__ lens, const int32_t* __restrict__ counts, int b, int t,
                                           int limit, int& pos)
{
    int n = seq_take(lens, counts, b, t, limit, pos);
    if constexpr (PG) {
        if (n > 0)
            for (int e = pos / pg.tokens, last = (pos + n - 1) / pg.tokens; e <= last; e++)
                if (!page_ok(pg, page_entry(pg, b, e))) n = -1;
    }
    return n;
}

// DEV: the position and the count of head bh are those of its sequence bh / heads, read from device memory (lens, counts or null); t is
// then the row pitch of k_new / v_new and the most a sequence can take, and the grid is sized for the worst position
// PG (DEV only): cap is a page's tokens and a token's rows lie where head_at says
// C4 (DEV and block 64 only): the code tensors hold nibbles; a thread's 16 codes are stored as 8 bytes
template <int DT, bool DEV, bool PG = false, bool C4 = false>
__global__ void __launch_bounds__(256) k_kv_append(const void* __restrict__ knew, const void* __restrict__ vnew, int8_t* __restrict__ kcodes,
                                                   int8_t* __restrict__ kexps, int8_t* __restrict__ vcodes, int8_t* __restrict__ vexps,
                                                   void* __restrict__ vtail, int BH, int D, int pos, int t, int cap, int ldd, int block,
                                                   int mant_bits, float eps_dt, const uint8_t* __restrict__ exp_win, int nkb, int zc,
                                                   const int32_t* __restrict__ lens, const int32_t* __restrict__ counts,
                                                   int32_t* __restrict__ overflow, int heads, int limit, Pages pg)
{
    static_assert(!PG || DEV, "a paged cache keeps its lengths on the device");
    static_assert(!C4 || DEV, "4-bit codes are the device-length cache's");
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    __shared__ uint32_t s_val[64 * kPitch];
    __shared__ uint32_t s_max[4 * kTD];
    const int tid = threadIdx.x;
    load_exp_win(s_win, exp_win);
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
        bool live = valid;
        if constexpr (DEV) {
            const int n = seq_take_at<PG>(pg, lens, counts, bh / heads, t, limit, pos);
            if (n < 0 && valid && i == 0 && seg == 0) overflow[0] = 1;
            live = valid && i < n;                                        // (one row: the lanes of a block are live together)
        }
        const raw_t* const src = reinterpret_cast<const raw_t*>(knew) + (size_t)row * D + seg * 16;
        uint32_t raw[16];
#pragma unroll
        for (int v = 0; v < 16 / Tr::VEC; v++) bfpq_dev::load_raw_vec<DT>(src, v, raw + v * Tr::VEC);
        uint32_t mx = abs_max<DT>(raw);
        if (per >= 2) mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 1, 64));
        if (per >= 4) mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 2, 64));
        const BlockScale bs = block_scale<DT>(mx, mant_bits, eps_dt, s_win);
        uint32_t pk[4];
        pack_codes<DT>(raw, 16, bs, pk);
        if (live) {
            size_t r = (size_t)bh * cap + pos + i;
            if constexpr (PG) {
                int sl;
                r = (size_t)head_at<true>(pg, bh, heads, pos + i, sl) * cap + sl;
            }
            if constexpr (C4) *reinterpret_cast<uint2*>(kcodes + ((r * ldd + seg * 16) >> 1)) = narrow(pk);
            else *reinterpret_cast<uint4*>(kcodes + r * ldd + seg * 16) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            if (seg % per == 0) kexps[r * (D / block) + seg / per] = sat_exp(bs);
        }
        return;
    }
    // values: workgroup (bh, 64-column slice, z); z = 0 does the chunk's first block and then its last, z >= 1 the block first + z
    const int dtiles = (D + kTD - 1) / kTD;
    const int vb = (int)blockIdx.x - nkb;
    const int z = vb % zc, dt = (vb / zc) % dtiles, bh = vb / (zc * dtiles);
    int cnt = t;
    if constexpr (DEV) {
        cnt = seq_take_at<PG>(pg, lens, counts, bh / heads, t, limit, pos);
        if (cnt <= 0) return;                                             // (the whole workgroup: nothing to take, or refused)
    }
    const int first = pos / block, last = (pos + cnt - 1) / block;
    if (DEV && z > 0 && first + z >= last) return;                        // (a block the worst position has and this one has not)
    const int n = (z == 0 && last != first) ? 2 : 1;
    for (int it = 0; it < n; it++) {
        if (it) __syncthreads();                                          // (the first block's tile and tail rows have been read)
        v_block<DT, PG, C4>(reinterpret_cast<const raw_t*>(vnew), reinterpret_cast<raw_t*>(vtail), vcodes, vexps, bh, it ? last : first + z, dt * kTD, D,
                        pos, cnt, t, cap, block, mant_bits, eps_dt, s_win, s_val, s_max, pg, heads);
    }
}

// ---- the decode product -----------------------------------------------------------------------------------------------------------
// MODE kDev (family qk of a device-length cache): head b has min(lens[b / heads], Nout) keys, the rest of its row up to Nout is -inf.
// MODE kAtt: that, with out an fp32 array: what a softmax over the row takes -- the score rounded to the dtype, widened and multiplied
// by `scale`, -inf from the row's visible length on (att_visible)
constexpr int kHost = 0, kDev = 1, kAtt = 2;

// keys that query row t of Tq sees of a head of `len` tokens, Kx = min(len, max_len) of them in reach: all, or (causal, the rows being
// the last Tq tokens held) those up to its own
__device__ __forceinline__ int att_visible(int len, int Kx, int Tq, int t, int causal)
{
    const int v = causal ? len - Tq + t + 1 : len;
    return v < Kx ? (v > 0 ? v : 0) : Kx;
}

// the first key that row sees (WIN instances): its sequence's `start` (left padding; negative counts as 0) or, with a window,
// the key `window` below the end of what it sees, whichever is later.  The row sees the keys lo <= n < att_visible, none where lo is
// not below that; lo does not decrease with t.  window 0: none
__device__ __forceinline__ int att_first(int len, int Tq, int t, int causal, int start, int window)
{
    const int lo = start > 0 ? start : 0;
    if (window <= 0) return lo;
    const int v = causal ? len - Tq + t + 1 : len;
    const int w = v > window ? v - window : 0;
    return w > lo ? w : lo;
}

// sequence b's start, or 0 without starts
__device__ __forceinline__ int seq_start(const int32_t* __restrict__ starts, int b) { return starts ? starts[b] : 0; }

// the least of a wave's values
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return __builtin_amdgcn_readfirstlane(v);                    // (the same in every lane: a scalar, so a branch on it is uniform)
}

// key k of a row that sees [lo, vis): WIN instances have a first key, the others see a prefix and never read lo
template <bool WIN> __device__ __forceinline__ bool sees(int k, int lo, int vis)
{
    if constexpr (WIN) return k >= lo && k < vis;
    else return k < vis;
}

// att_scores: MODE kAtt's epilogue on a lane's four scores of keys n .. n + 3 of a row that sees the keys lo .. vis - 1
template <int DT, bool WIN = false> __device__ __forceinline__ void att_scores(v2f& a01, v2f& a23, int n, int lo, int vis, float scale)
{
    const float ninf = -__builtin_inff();
    a01.x = sees<WIN>(n + 0, lo, vis) ? rnd<DT>(a01.x) * scale : ninf;
    a01.y = sees<WIN>(n + 1, lo, vis) ? rnd<DT>(a01.y) * scale : ninf;
    a23.x = sees<WIN>(n + 2, lo, vis) ? rnd<DT>(a23.x) * scale : ninf;
    a23.y = sees<WIN>(n + 3, lo, vis) ? rnd<DT>(a23.y) * scale : ninf;
}

// GRP: head b has R = group * Tq rows of x and out (row = query head of the group * Tq + token), walked in tiles of 16: blockIdx.y runs
// over (head, tile).  Without GRP the argument `group` is passed and never read (the compiler drops it: the register figures of those
// instances are the ones they had without it): one tile, the row is the token.
// WIN (kAtt only): rows have a first key (att_first; starts per sequence or null, window or 0 -- both unread without WIN).  A wave whose
// 16 TM keys lie below the first key of all 16 rows of the tile skips the product and stores nothing: the softmax never reads there.
// The WIN instances of block 64 are held to the 2 waves per SIMD of their plain twins (without the bound they take 241-243 VGPRs + 16
// AGPRs and run 1)
// PG (family qk of a paged cache; not with WIN): wbs is a page's tokens; the 16 TM <= 64 keys of a wave lie in one page, whose head
// (head_tile) gives the base of the wave's codes and exponents, its rows counted from the page's first token
// C4 (block 64, not kHost): w holds nibbles.  The chunk in use and the prefetched one stay packed, 2 words per operand instead of 4,
// and are widened right before the MFMA
template <int BLK, int DT, int TM, int MODE, bool GRP = false, bool WIN = false, bool PG = false, bool C4 = false>
__global__ void __launch_bounds__(256, WIN && BLK == 64 ? 2 : 1) k_kv_bmm_dec(const void* __restrict__ x, const int8_t* __restrict__ wc, const int8_t* __restrict__ we,
                                                    void* __restrict__ out, int B, int Tq, int Kx, int Nout, int ldx, int ldw, int ldwe, int wbs,
                                                    int ldo, int xm, int wm, float eps_dt, const uint8_t* __restrict__ exp_win,
                                                    const int32_t* __restrict__ lens, int heads, float scale, int causal, int group,
                                                    const int32_t* __restrict__ starts, int window, Pages pg)
{
    using Blk = I8Blk<BLK>;
    using op_t = typename Blk::op_t;
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    static_assert(!WIN || MODE == kAtt, "a first key is attention's");
    static_assert(!PG || (MODE != kHost && !WIN), "a paged cache keeps its lengths on the device and has no first key");
    static_assert(!C4 || (BLK == 64 && MODE != kHost), "4-bit codes: block 64 of a device-length cache");
    using ld_t = std::conditional_t<C4, uint2, op_t>;            // a lane's codes of a block as loaded
    constexpr bool DEV = MODE != kHost;
    constexpr int ODT = MODE == kAtt ? BFPQ_F32 : DT;            // the output's element type
    constexpr int NBS = 64 / BLK;                                // blocks per 64-byte chunk
    constexpr int NE = BLK == 64 ? 16 : 8;                       // a lane's bytes of a block
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    load_exp_win(s_win, exp_win);
    __syncthreads();
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 15, q = l >> 4;
    const int n0 = ((int)blockIdx.x * 4 + w) * 16 * TM;
    if (n0 >= Nout) return;                                      // (wave-uniform; no barrier below)
    const int nb = (Kx + BLK - 1) / BLK, nch = (Kx + 63) >> 6;
    const int R = GRP ? Tq * group : Tq, ntiles = GRP ? (R + 15) >> 4 : 1;
    const int pt0 = PG ? n0 - n0 % pg.tokens : 0;                // (PG) the first token of the page of the wave's keys

    uint32_t offW[TM], ewo[TM][4];
    auto rows = [&](int No) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const int n = n0 + 16 * i + r;
            offW[i] = (uint32_t)((n < No ? n : No - 1) - pt0) * (uint32_t)ldw + Blk::lane(q);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int ne = n0 + 16 * i + 4 * q + j;
                ewo[i][j] = (uint32_t)((ne < No ? ne : No - 1) - pt0) * (uint32_t)ldwe;
            }
        }
    };
    if constexpr (!DEV) rows(Nout);
    const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};
    const float ninf = -__builtin_inff();

    for (int y = blockIdx.y; y < B * ntiles; y += gridDim.y) {
        const int b = GRP ? y / ntiles : y, row = GRP ? (y % ntiles) * 16 + r : r;   // the head, and the lane's row of it
        const bool tok = row < R;
        size_t hb = b;                                            // the head the wave's codes lie in
        if constexpr (PG) {                                      // (the page of the wave's keys: fetched beside the length)
            int sl;
            hb = head_tile<true>(pg, b, heads, n0, sl);
        }
        int No = Nout, len = 0;
        if constexpr (DEV) {
            len = lens[b / heads];
            No = clamp_len(len, Nout);
            if (n0 >= No) {                                      // (wave-uniform) none of this wave's keys exists
                if (tok) {
#pragma unroll
                    for (int i = 0; i < TM; i++) {
                        const int n = n0 + 16 * i + 4 * q;
                        if (n < Nout) store4<ODT>(out, ((size_t)b * R + row) * ldo + n, v2f{ninf, ninf}, v2f{ninf, ninf});
                    }
                }
                continue;
            }
            rows(No);
        }
        // (WIN) the first key the lane's row sees
        auto first = [&]() __attribute__((always_inline)) { return att_first(len, Tq, GRP ? row % Tq : r, causal, seq_start(starts, b / heads), window); };
        if constexpr (WIN) {
            if (n0 + 16 * TM <= wave_min(tok ? first() : 0x7fffffff)) continue;   // (wave-uniform) no row of the tile sees a key of this wave
        }
        const int8_t* const wcb = wc + (C4 ? (hb * wbs * ldw) >> 1 : hb * wbs * ldw);
        const int8_t* const web = we + hb * wbs * ldwe;
        const raw_t* const xr = reinterpret_cast<const raw_t*>(x) + ((size_t)b * R + (tok ? row : 0)) * ldx;

        // chunk c: the lane's w codes, the exponents of its four output rows (byte s of a word = block s of the chunk) and its x elements
        auto load = [&](int c, ld_t (&aF)[TM][NBS], uint32_t (&ew)[TM][4], uint32_t (&xv)[NBS][NE]) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; i++) {
#pragma unroll
                for (int s = 0; s < NBS; s++) {
                    if constexpr (C4) {
                        aF[i][s] = *reinterpret_cast<const uint2*>(wcb + ((offW[i] + (c << 6)) >> 1));
                    } else {
                        aF[i][s] = *reinterpret_cast<const op_t*>(wcb + offW[i] + (c << 6) + s * BLK);
                        if (!Blk::a_live(q)) aF[i][s] = op_t{};
                    }
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

        ld_t aF[TM][NBS], aN[TM][NBS];
        uint32_t ew[TM][4], ewN[TM][4], xv[NBS][NE], xN[NBS][NE];
        load(0, aF, ew, xv);
#pragma unroll 1
        for (int c = 0; c < nch; c++) {
            if (c + 1 < nch) load(c + 1, aN, ewN, xN);
#pragma unroll
            for (int s = 0; s < NBS; s++) {
                if (c * NBS + s < nb) {                          // (wave-uniform)
                    BlockScale bs;                                // x's block
                    const op_t bF = quant_operand<BLK, DT>(xv[s], abs_max<DT>(xv[s]), xm, eps_dt, s_win, bs);
                    v2f sx, nm;
                    token_scale((int)sat_exp(bs), xm, sx, nm);
                    const int sh = 8 * s;
#pragma unroll
                    for (int i = 0; i < TM; i++) {
                        v2f sw01, sw23;
                        weight_scales(exp_byte(ew[i][0], sh), exp_byte(ew[i][1], sh), exp_byte(ew[i][2], sh), exp_byte(ew[i][3], sh), wm, sw01, sw23);
                        rescale(Blk::mfma(widen(aF[i][s]), bF, magic), sx, nm, sw01, sw23, acc[i][0], acc[i][1]);
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

        // the lane holds rows n .. n + 3 of row `row` (the pitch ldo takes the ones past Nout)
        if (tok) {
            const int lo = WIN ? first() : 0;
#pragma unroll
            for (int i = 0; i < TM; i++) {
                const int n = n0 + 16 * i + 4 * q;
                if constexpr (MODE == kAtt) {
                    att_scores<DT, WIN>(acc[i][0], acc[i][1], n, lo, att_visible(len, No, Tq, GRP ? row % Tq : r, causal), scale);
                } else if constexpr (DEV) {
                    if (n + 0 >= No) acc[i][0].x = ninf;
                    if (n + 1 >= No) acc[i][0].y = ninf;
                    if (n + 2 >= No) acc[i][1].x = ninf;
                    if (n + 3 >= No) acc[i][1].y = ninf;
                }
                if (n < Nout) store4<ODT>(out, ((size_t)b * R + row) * ldo + n, acc[i][0], acc[i][1]);
            }
        }
    }
}

// ---- p v over a device-length cache, the contraction split over workgroups ------------------------------------------------------------
// k_kv_pv_split: workgroup (64-column group of D, slice of kMaxCps or fewer 64-token chunks, head).  Head bh contracts over its first
// Kx = min(lens[bh / heads], L) tokens; a workgroup whose slice starts at or past Kx returns at once.  Wave w first quantizes the chunks
// w, w + 4, ... of the slice (quant_operand; elements at or past Kx are zeros whatever x holds there) into LDS, once for the four
// waves; then every wave multiplies the blocks of
// the slice against its 16 columns of v_codes and writes the raw result of the block product -- the exact integer sum on top of the
// MFMA's C operand MAGIC_I -- to sums [BH, Tq, nbw, D], and the first wave of a head x's block exponents to xexp [BH, Tq, nbw].
// k_kv_pv_combine: a thread per four columns of one token runs rescale() of bfpq_i8mma.h over the blocks j < ceil(Kx / BLK) in block
// order: the fp32 additions are those of k_kv_bmm_dec in the same order, so the result is the same bits whatever the slice size.
//
// ATT (bfpq_kv_attend): x holds no probabilities but the fp32 score rows k_kv_bmm_dec<.., kAtt> left, pitch ldx.  Every workgroup first
// reduces each row of its head over the row's visible columns (att_visible) with row_stats, so all workgroups of a head hold the same
// two numbers per row, whatever the slice size.  The quantization stage then takes form_p's bits exactly as it takes a p it loaded.
// With pout the workgroups of the first column group also store p [BH, Tq, ldp], zeros included (also those past the head's length,
// before they return).
//
// GRP: head bh has R = group * Tq rows (k_kv_bmm_dec), blockIdx.z runs over (head, tile of 16 rows) and a workgroup reduces, quantizes
// and multiplies the rows of its own tile; sums, xexp, the score rows and p are indexed by (head, row).  A row's visible length is that
// of its token, row % Tq.  Without GRP `group` is unused here too.
//
// WIN (ATT only): rows have a first key (att_first).  A slice whose tokens lie below the first key of every row of the tile leaves what
// a zero p block leaves the combine pass -- the bare MAGIC_I, exact for zero codes whatever V holds, and block_scale(0)'s exponent --
// and reads neither score rows nor V codes.  Without WIN starts and window are unread.
constexpr int kMaxCps = 16;                               // chunks per slice (the LDS holds their codes)
constexpr int64_t kSplitGrid = 2048;                      // workgroups the chosen slice size aims to stay within

__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// ---- the softmax row law: one order of operations per row, whatever kernel, slice or panel the row is in ---------------------------------
__device__ __forceinline__ float wave_nan_max(float m)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
    return m;
}
__device__ __forceinline__ float wave_add(float a)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}

// s_red [2][NR rows][4 waves]: the four waves' partial maxima of every row, then their partial sums; combined as (w0, w1), (w2, w3)
__device__ __forceinline__ float row_max(const float* s_red, int row)
{
    const float* const sm = s_red + row * 4;
    return nan_max(nan_max(sm[0], sm[1]), nan_max(sm[2], sm[3]));
}
template <int NR> __device__ __forceinline__ float row_sum(const float* s_red, int row)
{
    const float* const ss = s_red + (NR + row) * 4;
    return (ss[0] + ss[1]) + (ss[2] + ss[3]);
}

// row_stats: rows t < nr of the fp32 score rows sc (pitch ld) reduced over their columns lo(t) .. vis(t) - 1 to s_red, by all 256 threads: the
// maximum (NaN propagates), then the sum of expf(s - max) -- a thread over its columns 4 tid + 1024 i .. + 3 in ascending order, the 64
// lanes of a wave by a butterfly, the waves' partials left for row_max / row_sum.  U rows' loads are in flight at a time; a row's
// operations and their order do not depend on U, nr or the rows beside it.  Both passes end with a barrier; whatever the caller wrote
// to LDS before the call is visible after it.  WIN: a thread keeps the columns it owns and leaves out those below lo(t) -- the bits of the
// row with -inf there, nan_max(m, -inf) == m and a + expf(-inf - m) == a -- starting at its first stride that reaches some row's first
// key; it loads a float4 only where the row sees one of the four.  Without WIN lo is never called
template <int U, int NR, bool WIN, class V, class F>
__device__ __forceinline__ void row_stats(const float* __restrict__ sc, int ld, int nr, V&& vis, F&& lo, float* s_red)
{
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    // f(u, v) over the visible elements this thread owns of rows t0 + u, u < U, each row's in ascending order
    auto walk = [&](int t0, auto&& f) __attribute__((always_inline)) {
        int vt[U], vm = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            vt[u] = t0 + u < nr ? vis(t0 + u) : 0;
            vm = vt[u] > vm ? vt[u] : vm;
        }
        if constexpr (WIN) {
            int lt[U], lm = 0x7fffffff;
#pragma unroll
            for (int u = 0; u < U; u++) {
                lt[u] = t0 + u < nr ? lo(t0 + u) : 0x7fffffff;
                lm = lt[u] < lm ? lt[u] : lm;
            }
            if (lm >= vm) return;                                // no row of these sees a key
            const int own = tid * 4 + 3;                         // the thread's first stride with a column at or past lm
            for (int k = tid * 4 + (lm > own ? (lm - own + 1023) / 1024 * 1024 : 0); k < vm; k += 1024) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (k < vt[u] && k + 3 >= lt[u] && lt[u] < vt[u]) {   // (a row that sees nothing loads nothing)
                        const float4 v = *reinterpret_cast<const float4*>(sc + (size_t)(t0 + u) * ld + k);
                        if (k >= lt[u]) f(u, v.x);
                        if (k + 1 >= lt[u] && k + 1 < vt[u]) f(u, v.y);
                        if (k + 2 >= lt[u] && k + 2 < vt[u]) f(u, v.z);
                        if (k + 3 < vt[u]) f(u, v.w);
                    }
                }
            }
            return;
        }
        for (int k = tid * 4; k < vm; k += 1024) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (k < vt[u]) {
                    const float4 v = *reinterpret_cast<const float4*>(sc + (size_t)(t0 + u) * ld + k);
                    f(u, v.x);
                    if (k + 1 < vt[u]) f(u, v.y);
                    if (k + 2 < vt[u]) f(u, v.z);
                    if (k + 3 < vt[u]) f(u, v.w);
                }
            }
        }
    };
    for (int t0 = 0; t0 < nr; t0 += U) {
        float m[U];
#pragma unroll
        for (int u = 0; u < U; u++) m[u] = -__builtin_inff();
        walk(t0, [&](int u, float v) { m[u] = nan_max(m[u], v); });
#pragma unroll
        for (int u = 0; u < U; u++) {
            m[u] = wave_nan_max(m[u]);
            if (l == 0 && t0 + u < nr) s_red[(t0 + u) * 4 + w] = m[u];
        }
    }
    __syncthreads();
    for (int t0 = 0; t0 < nr; t0 += U) {
        float m[U], a[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            m[u] = row_max(s_red, t0 + u < nr ? t0 + u : 0);
            a[u] = 0.f;
        }
        walk(t0, [&](int u, float v) { a[u] += expf(v - m[u]); });
#pragma unroll
        for (int u = 0; u < U; u++) {
            a[u] = wave_add(a[u]);
            if (l == 0 && t0 + u < nr) s_red[(NR + t0 + u) * 4 + w] = a[u];
        }
    }
    __syncthreads();
}

// form_p: p of the lane's NE elements k0 .. of its fp32 score row, in the dtype's bits: expf(s - rmax) / rsum rounded once, +0 from the
// row's visible length on (WIN: and below its first key lo, with the same guard on the loads).  prow (or null): the lane's row of the p
// the caller returns; the visible elements are stored there
template <int DT, bool WIN, int NE>
__device__ __forceinline__ void form_p(const float* __restrict__ srow, int k0, int lo, int vis, float rmax, float rsum,
                                       typename Traits<DT>::raw_t* prow, uint32_t (&xv)[NE])
{
#pragma unroll
    for (int v = 0; v < NE / 4; v++) {
        float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (WIN) {
            if (k0 + 4 * v < vis && k0 + 4 * v + 3 >= lo) sv = *reinterpret_cast<const float4*>(srow + k0 + 4 * v);
        } else {
            if (k0 + 4 * v < vis) sv = *reinterpret_cast<const float4*>(srow + k0 + 4 * v);
        }
        const float se[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int k = k0 + 4 * v + e;
            xv[4 * v + e] = sees<WIN>(k, lo, vis) ? f32_to_raw<DT>(expf(se[e] - rmax) / rsum) : 0u;
            if (prow && sees<WIN>(k, lo, vis)) prow[k] = (typename Traits<DT>::raw_t)xv[4 * v + e];
        }
    }
}

//
// PG (not with WIN): cap is a page's tokens; a 64-token chunk lies in one page, whose head is fetched once per chunk (head_tile), the
// next chunk's ahead of this chunk's loads.
// C4 (block 64): vc holds nibbles, widened as they are loaded.
template <int BLK, int DT, bool ATT, bool GRP = false, bool WIN = false, bool PG = false, bool C4 = false>
__global__ void __launch_bounds__(256) k_kv_pv_split(const void* __restrict__ x, const int8_t* __restrict__ vc, int32_t* __restrict__ sums,
                                                     int8_t* __restrict__ xexp, const int32_t* __restrict__ lens, int heads, int Tq, int L,
                                                     int D, int ldx, int cap, int nbw, int cps, int xvec, int xm, float eps_dt,
                                                     const uint8_t* __restrict__ exp_win, void* __restrict__ pout, int ldp, int causal,
                                                     int group, const int32_t* __restrict__ starts, int window, Pages pg)
{
    static_assert(!WIN || ATT, "a first key is attention's");
    static_assert(!PG || !WIN, "a paged cache has no first key");
    static_assert(!C4 || BLK == 64, "4-bit codes: block 64");
    using Blk = I8Blk<BLK>;
    using op_t = typename Blk::op_t;
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    constexpr int NBS = 64 / BLK, NE = BLK == 64 ? 16 : 8;
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    __shared__ op_t s_b[kMaxCps][NBS][64];
    __shared__ int8_t s_e[kMaxCps][NBS][16];
    __shared__ float s_red[ATT ? 2 * BFPQ_KV_DEC_MAX_TOKENS * 4 : 1];   // per row and wave: the maximum, then the sum
    const int R = GRP ? Tq * group : Tq, ntiles = GRP ? (R + 15) >> 4 : 1;
    const int bh = GRP ? (int)blockIdx.z / ntiles : (int)blockIdx.z, c0 = (int)blockIdx.y * cps;
    const int r0 = GRP ? ((int)blockIdx.z % ntiles) * 16 : 0, nr = GRP ? (R - r0 < 16 ? R - r0 : 16) : Tq;   // the tile's first row, its rows
    auto token = [&](int i) __attribute__((always_inline)) { return GRP ? (r0 + i) % Tq : i; };               // of the tile's row i
    int hbN = 0, slN = 0;                                        // (PG) the head and the first token of the chunk to come: the slice's first,
    if constexpr (PG) hbN = head_tile<true>(pg, bh, heads, c0 << 6, slN);   // fetched beside the length
    const int len = lens[bh / heads];
    const int Kx = clamp_len(len, L);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 15, q = l >> 4;
    const bool tok = r < nr;
    raw_t* const prow = pout ? reinterpret_cast<raw_t*>(pout) + ((size_t)bh * R + r0) * ldp : nullptr;   // the tile's rows of p
    const int start = WIN ? seq_start(starts, bh / heads) : 0;
    auto first = [&](int i) __attribute__((always_inline)) { return att_first(len, Tq, token(i), causal, start, window); };   // (WIN) of row i
    if constexpr (ATT) {
        if (pout && blockIdx.x == 0) {                           // +0 at what the rows do not see of this slice's columns
            const int k0 = c0 << 6, k1 = k0 + (cps << 6) < L ? k0 + (cps << 6) : L;
            for (int i = threadIdx.x; i < nr * (k1 - k0); i += 256) {
                const int t = i / (k1 - k0), k = k0 + i % (k1 - k0);
                if (!sees<WIN>(k, WIN ? first(t) : 0, att_visible(len, Kx, Tq, token(t), causal))) prow[(size_t)t * ldp + k] = (raw_t)0;
            }
        }
    }
    if ((c0 << 6) >= Kx) return;                                 // (the whole workgroup, before any barrier)
    load_exp_win(s_win, exp_win);
    if constexpr (WIN) {
        const int c1 = c0 + cps < (Kx + 63) >> 6 ? c0 + cps : (Kx + 63) >> 6;
        if ((c1 << 6) <= wave_min(tok ? first(r) : 0x7fffffff)) {  // (the whole workgroup) no row of the tile sees a token of the slice
            __syncthreads();
            const int n0 = ((int)blockIdx.x * 4 + w) * 16, nb = (Kx + BLK - 1) / BLK;
            if (n0 >= D || !tok) return;
            const int8_t e0 = sat_exp(block_scale<DT>(0u, xm, eps_dt, s_win));
            const size_t o0 = ((size_t)bh * R + r0 + r) * nbw;
            for (int j = c0 * NBS; j < c1 * NBS && j < nb; j++) {
                *reinterpret_cast<v4i*>(sums + (o0 + j) * D + n0 + 4 * q) = v4i{MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};
                if (n0 == 0 && q == 0) xexp[o0 + j] = e0;
            }
            return;
        }
    }
    const float* const srow = reinterpret_cast<const float*>(x) + ((size_t)bh * R + r0 + (tok ? r : 0)) * ldx;   // (ATT) the lane's score row
    raw_t* const plane = (prow && blockIdx.x == 0) ? prow + (size_t)r * ldp : nullptr;                            // (ATT) and its row of p
    float rmax = 0.f, rsum = 1.f;
    int vis = 0, lo = 0;
    if constexpr (ATT) {
        row_stats<1, BFPQ_KV_DEC_MAX_TOKENS, WIN>(reinterpret_cast<const float*>(x) + ((size_t)bh * R + r0) * ldx, ldx, nr,
                                                  [&](int t) { return att_visible(len, Kx, Tq, token(t), causal); }, first, s_red);
        if (tok) {
            rmax = row_max(s_red, r);
            rsum = row_sum<BFPQ_KV_DEC_MAX_TOKENS>(s_red, r);
            vis = att_visible(len, Kx, Tq, token(r), causal);
            if constexpr (WIN) lo = first(r);
        }
    } else __syncthreads();
    const int nb = (Kx + BLK - 1) / BLK, nch = (Kx + 63) >> 6, c1 = c0 + cps < nch ? c0 + cps : nch;
    const raw_t* const xr = reinterpret_cast<const raw_t*>(x) + ((size_t)bh * R + r0 + (tok ? r : 0)) * ldx;

    for (int c = c0 + w; c < c1; c += 4) {
#pragma unroll
        for (int s = 0; s < NBS; s++) {
            if (c * NBS + s >= nb) break;                        // (wave-uniform)
            const int k0 = (c << 6) + s * BLK + Blk::lane(q);
            uint32_t xv[NE];
            if constexpr (ATT) {
                form_p<DT, WIN>(srow, k0, lo, vis, rmax, rsum, plane, xv);
            } else if (xvec && k0 + NE <= L) {                   // rows 16-byte aligned: the lane's elements in 16-byte loads
#pragma unroll
                for (int v = 0; v < NE / Tr::VEC; v++) bfpq_dev::load_raw_vec<DT>(xr + k0, v, xv + v * Tr::VEC);
            } else {
#pragma unroll
                for (int e = 0; e < NE; e++) xv[e] = k0 + e < L ? (uint32_t)xr[k0 + e] : 0u;
            }
            if constexpr (!ATT) {
#pragma unroll
                for (int e = 0; e < NE; e++)
                    if (!tok || k0 + e >= Kx) xv[e] = 0u;
            }
            BlockScale bs;
            s_b[c - c0][s][l] = quant_operand<BLK, DT>(xv, abs_max<DT>(xv), xm, eps_dt, s_win, bs);
            if (q == 0) s_e[c - c0][s][r] = sat_exp(bs);
        }
    }
    __syncthreads();

    const int n0 = ((int)blockIdx.x * 4 + w) * 16;
    if (n0 >= D) return;                                         // (wave-uniform; no barrier below.  D % 16 == 0: 16 whole columns)
    const int8_t* const wrow = C4 ? vc + ((((size_t)bh * D + n0 + r) * cap + Blk::lane(q)) >> 1) : vc + ((size_t)bh * D + n0 + r) * cap + Blk::lane(q);
    const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};
    const size_t o0 = ((size_t)bh * R + r0 + (tok ? r : 0)) * nbw;
    for (int c = c0; c < c1; c++) {
        const int8_t* wch = wrow + (C4 ? c << 5 : c << 6);       // the lane's codes of the chunk
        if constexpr (PG) {
            if constexpr (C4) wch = vc + ((((size_t)hbN * D + n0 + r) * cap + slN + Blk::lane(q)) >> 1);
            else wch = vc + ((size_t)hbN * D + n0 + r) * cap + slN + Blk::lane(q);
            if (c + 1 < c1) hbN = head_tile<true>(pg, bh, heads, (c + 1) << 6, slN);
        }
#pragma unroll
        for (int s = 0; s < NBS; s++) {
            const int j = c * NBS + s;
            if (j >= nb) break;                                  // (wave-uniform)
            op_t aF;
            if constexpr (C4) aF = widen(*reinterpret_cast<const uint2*>(wch));
            else aF = *reinterpret_cast<const op_t*>(wch + s * BLK);
            if (!Blk::a_live(q)) aF = op_t{};
            const v4i d = Blk::mfma(aF, s_b[c - c0][s][l], magic);
            if (tok) {
                *reinterpret_cast<v4i*>(sums + (o0 + j) * D + n0 + 4 * q) = d;
                if (n0 == 0 && q == 0) xexp[o0 + j] = s_e[c - c0][s][r];
            }
        }
    }
}

// PG: V's exponents of block j lie in the page of its tokens (head_at: per thread, a thread being a row of a head), ldve a page's blocks
template <int DT, bool PG = false>
__global__ void __launch_bounds__(256) k_kv_pv_combine(const int32_t* __restrict__ sums, const int8_t* __restrict__ xexp,
                                                       const int8_t* __restrict__ ve, void* __restrict__ out, const int32_t* __restrict__ lens,
                                                       int heads, int64_t total, int Tq, int L, int D, int ldve, int nbw, int ldo, int block,
                                                       int xm, int wm, Pages pg)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int d4 = D >> 2, n = (int)(idx % d4) * 4;
    const int64_t row = idx / d4;                                // bh * Tq + t
    const int bh = (int)(row / Tq);
    const int nb = (clamp_len(lens[bh / heads], L) + block - 1) / block;
    const int32_t* const sr = sums + (size_t)row * nbw * D + n;
    const int8_t* const xe = xexp + (size_t)row * nbw;
    const int8_t* const we = ve + ((size_t)bh * D + n) * ldve;
    v2f a01 = v2f{0.f, 0.f}, a23 = v2f{0.f, 0.f};
    // the loads of kCU blocks are written ahead of their use; the additions stay in block order.  (Measured: no gain over the plain loop,
    // 0.4-0.66 us per block and thread either way -- DESIGN 5k; this pass is what bounds context() now.)
    constexpr int kCU = 8;
    for (int j0 = 0; j0 < nb; j0 += kCU) {
        v4i d[kCU];
        int ex[kCU], ew[kCU][4];
#pragma unroll
        for (int u = 0; u < kCU; u++) {
            const int j = j0 + u < nb ? j0 + u : nb - 1;
            d[u] = *reinterpret_cast<const v4i*>(sr + (size_t)j * D);
            ex[u] = (int)xe[j];
            if constexpr (PG) {
                int sl;
                const int hb = head_at<true>(pg, bh, heads, j * block, sl);
                const int8_t* const wej = ve + ((size_t)hb * D + n) * ldve + (sl >> (__ffs(block) - 1));   // (block: a power of two)
#pragma unroll
                for (int i = 0; i < 4; i++) ew[u][i] = (int)wej[i * ldve];
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) ew[u][i] = (int)we[i * ldve + j];
            }
        }
#pragma unroll
        for (int u = 0; u < kCU; u++) {
            if (j0 + u >= nb) break;
            v2f sx, nm;
            token_scale(ex[u], xm, sx, nm);
            v2f sw01, sw23;
            weight_scales(ew[u][0], ew[u][1], ew[u][2], ew[u][3], wm, sw01, sw23);
            rescale(d[u], sx, nm, sw01, sw23, a01, a23);
        }
    }
    store4<DT>(out, (size_t)row * ldo + n, a01, a23);
}

// lens[b] += what sequence b took of the chunk (seq_take: nothing where it was refused); after k_kv_append<.., true> in stream order
// (PG: seq_take_at, so a sequence refused for a missing page stays where it is)
template <bool PG = false>
__global__ void __launch_bounds__(256) k_kv_advance(int32_t* __restrict__ lens, const int32_t* __restrict__ counts, int B, int t, int limit, Pages pg)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int pos;
    const int n = seq_take_at<PG>(pg, lens, counts, b, t, limit, pos);
    if (n > 0) lens[b] = pos + n;
}

// ---- attention over a panel of query rows (bfpq_kv_attend_rows) ------------------------------------------------------------------------
// Shared by the two kernels.  The panel holds PR = group * rows rows per kv head; rows [a, e] of it (e < PR) see at most what their
// latest token sees: the last row's token, or the panel's last token where the range runs over the end of a query head's segment.
constexpr int kRowsWg = 64;                               // panel rows per workgroup: a tile of 16 per wave
constexpr int kMaxDT = 16;                                // 16-column tiles of D a wave of k_kv_pv_rows accumulates: D <= 256

__device__ __forceinline__ int range_visible(int a, int e, int rows, int row0, int len, int Kx, int Tq, int causal)
{
    const int t = a / rows != e / rows ? row0 + rows - 1 : row0 + e % rows;
    return att_visible(len, Kx, Tq, t, causal);
}

// ... and see no key below what their earliest token sees first (att_first does not decrease with the token): the first row's token,
// or the panel's first token where the range runs over the end of a query head's segment
__device__ __forceinline__ int range_first(int a, int e, int rows, int row0, int len, int Tq, int causal, int start, int window)
{
    const int t = a / rows != e / rows ? row0 : row0 + a % rows;
    return att_first(len, Tq, t, causal, start, window);
}

// An operand of block BLK as it lies in LDS: 64 lanes of 16 bytes, of 8 bytes, or (block 16, whose lanes 32..63 carry no k) 32 lanes
template <int BLK> struct LdsOp {
    static constexpr int LN = BLK == 16 ? 32 : 64;
    __device__ __forceinline__ static int slot(int l) { return l & (LN - 1); }
};

// q k^T of panel rows: workgroup (kv head b, 64 panel rows).  Its rows of q are quantized once (quant_operand) and kept as MFMA
// operands s_q [wave][block][lane] with their exponents s_qe; then it loops over the tiles of 64 keys some row of it sees: the tile's codes s_k [16-key tile][block][lane] and exponents s_ke
// [block][key] are loaded once for the four waves, and a wave whose own rows see none of the tile sits it out.  Blocks are added in
// block order, the epilogue is att_scores; only the columns below the wave's visible length are written, which is all the softmax reads.
// WIN: rows have a first key (att_first).  The loop starts at the tile of the workgroup's least first key (range_first) and a wave sits
// out the tiles below its own rows' least; those columns are not written and the softmax does not read them.
// PG (not with WIN): cap is a page's tokens; a tile of 64 keys lies in one page, whose head is fetched once per tile (head_tile), the
// next tile's ahead of this tile's loads.
// C4 (block 64): kc holds nibbles.  They are widened on the way into LDS -- once per workgroup, not once per wave at the fragment read --
// so s_k holds the int8 operands and everything after the tile's load is the int8 instance's code; the LDS bytes stay what they were.
template <int BLK, int DT, bool WIN = false, bool PG = false, bool C4 = false>
__global__ void __launch_bounds__(256) k_kv_qk_rows(const void* __restrict__ x, const int8_t* __restrict__ kc, const int8_t* __restrict__ ke,
                                                    float* __restrict__ ws, int Tq, int D, int Nout, int ldd, int cap, int pitch, int xm, int wm,
                                                    float eps_dt, const uint8_t* __restrict__ exp_win, const int32_t* __restrict__ lens, int heads,
                                                    float scale, int causal, int group, int row0, int rows, const int32_t* __restrict__ starts,
                                                    int window, Pages pg)
{
    static_assert(!PG || !WIN, "a paged cache has no first key");
    static_assert(!C4 || BLK == 64, "4-bit codes: block 64");
    using Blk = I8Blk<BLK>;
    using op_t = typename Blk::op_t;
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    constexpr int NE = BLK == 64 ? 16 : 8, LN = LdsOp<BLK>::LN;
    extern __shared__ uint4 s_dyn[];
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    const int nbd = D / BLK;
    op_t* const s_q = reinterpret_cast<op_t*>(s_dyn);             // [4][nbd][LN]
    op_t* const s_k = s_q + 4 * nbd * LN;                         // [4][nbd][LN]
    int8_t* const s_ke = reinterpret_cast<int8_t*>(s_k + 4 * nbd * LN);   // [nbd][64]
    int8_t* const s_qe = s_ke + nbd * 64;                         // [4][nbd][16]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 15, q = l >> 4;
    const int PR = group * rows, nwg = (PR + kRowsWg - 1) / kRowsWg;
    const int b = (int)blockIdx.x / nwg, pr0 = ((int)blockIdx.x % nwg) * kRowsWg;
    const int len = lens[b / heads];
    const int No = clamp_len(len, Nout);
    const int prl = pr0 + kRowsWg - 1 < PR ? pr0 + kRowsWg - 1 : PR - 1;
    const int vwg = range_visible(pr0, prl, rows, row0, len, No, Tq, causal);
    if (vwg <= 0) return;                                        // (the whole workgroup, before any barrier) no row sees a key
    const int start = WIN ? seq_start(starts, b / heads) : 0;
    const int lwg = WIN ? range_first(pr0, prl, rows, row0, len, Tq, causal, start, window) : 0;   // the workgroup's least first key
    if (WIN && lwg >= vwg) return;                               // (likewise)
    load_exp_win(s_win, exp_win);
    __syncthreads();
    const int pw0 = pr0 + 16 * w, pwl = pw0 + 15 < PR ? pw0 + 15 : PR - 1;
    const int vw = pw0 < PR ? range_visible(pw0, pwl, rows, row0, len, No, Tq, causal) : 0;   // what the wave's rows see at most
    const int lw = WIN && pw0 < PR ? range_first(pw0, pwl, rows, row0, len, Tq, causal, start, window) : 0;   // and where at the earliest
    const int pr = pw0 + r;
    const bool tok = pr < PR;
    const int hq = tok ? pr / rows : 0, t = tok ? row0 + pr % rows : row0;
    {
        const raw_t* const xr = reinterpret_cast<const raw_t*>(x) + ((size_t)b * group * Tq + (size_t)hq * Tq + t) * D;
        for (int j = 0; j < nbd; j++) {
            uint32_t xv[NE];
#pragma unroll
            for (int v = 0; v < NE / Tr::VEC; v++) bfpq_dev::load_raw_vec<DT>(xr + j * BLK + Blk::lane(q), v, xv + v * Tr::VEC);
#pragma unroll
            for (int e = 0; e < NE; e++)
                if (!tok) xv[e] = 0u;
            BlockScale bs;
            const op_t bF = quant_operand<BLK, DT>(xv, abs_max<DT>(xv), xm, eps_dt, s_win, bs);
            if (l < LN) s_q[(w * nbd + j) * LN + l] = bF;
            if (q == 0) s_qe[(w * nbd + j) * 16 + r] = sat_exp(bs);
        }
    }
    const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};
    const int vis = tok ? att_visible(len, No, Tq, t, causal) : 0;
    const int lo = WIN ? att_first(len, Tq, t, causal, start, window) : 0;
    float* const orow = ws + ((size_t)b * PR + (tok ? pr : pr0)) * pitch;
    const int nkt = (vwg + 63) >> 6;
    int hbN = 0, slN = 0;                                        // (PG) the head and the first key of the tile to come
    if constexpr (PG) hbN = head_tile<true>(pg, b, heads, 0, slN);
    for (int kt = WIN ? lwg >> 6 : 0; kt < nkt; kt++) {
        __syncthreads();                                         // (s_q, s_qe written; the tile before this one read)
        const size_t k0 = PG ? (size_t)hbN * cap + slN : (size_t)b * cap + (kt << 6);   // the tile's first row of the codes and exponents
        if constexpr (PG) {
            if (kt + 1 < nkt) hbN = head_tile<true>(pg, b, heads, (kt + 1) << 6, slN);
        }
        const int8_t* const kcb = kc + k0 * ldd;
        const int8_t* const keb = ke + k0 * nbd;
        for (int idx = tid; idx < 4 * nbd * LN; idx += 256) {    // idx = (16-key tile i, block j, lane slot)
            const int ls = idx % LN, j = (idx / LN) % nbd, i = idx / (LN * nbd);
            if constexpr (C4) s_k[idx] = load_c4(kc, (k0 + 16 * i + (ls & 15)) * ldd + j * BLK + Blk::lane(ls >> 4));
            else s_k[idx] = *reinterpret_cast<const op_t*>(kcb + (size_t)(16 * i + (ls & 15)) * ldd + j * BLK + Blk::lane(ls >> 4));
        }
        for (int idx = tid; idx < 64 * nbd; idx += 256) s_ke[(idx % nbd) * 64 + idx / nbd] = keb[idx];
        __syncthreads();
        if ((kt << 6) >= vw) continue;                           // (wave-uniform) none of the wave's rows sees this tile
        if (WIN && ((kt + 1) << 6) <= lw) continue;              // (likewise) it lies below their first keys
        v2f acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i][0] = acc[i][1] = v2f{0.f, 0.f};
        for (int j = 0; j < nbd; j++) {
            const op_t bF = s_q[(w * nbd + j) * LN + LdsOp<BLK>::slot(l)];
            v2f sx, nm;
            token_scale((int)s_qe[(w * nbd + j) * 16 + r], xm, sx, nm);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                op_t aF = s_k[(i * nbd + j) * LN + LdsOp<BLK>::slot(l)];
                if (!Blk::a_live(q)) aF = op_t{};
                v2f sw01, sw23;
                weight_scales(*reinterpret_cast<const uint32_t*>(s_ke + j * 64 + 16 * i + 4 * q), wm, sw01, sw23);
                rescale(Blk::mfma(aF, bF, magic), sx, nm, sw01, sw23, acc[i][0], acc[i][1]);
            }
        }
        if (tok) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int n = (kt << 6) + 16 * i + 4 * q;
                att_scores<DT, WIN>(acc[i][0], acc[i][1], n, lo, vis, scale);
                if (n < Nout) store4<BFPQ_F32>(orow, n, acc[i][0], acc[i][1]);
            }
        }
    }
}

// softmax and p v of panel rows: workgroup (kv head bh, 64 panel rows), wave w the 16-row tile w and all D <= 256 columns.  First every
// row's maximum and sum (row_stats, four rows' loads in flight at a time).  Then the walk over 64-token chunks: the chunk's V codes
// s_v [16-column tile][block][lane] and exponents s_ve [block][column] go through LDS once for the four waves; a wave runs form_p and
// quant_operand on its rows for a block and adds the block's term for every column tile with rescale() -- k_kv_pv_combine's additions
// in its order.  A wave stops forming p after the last block any of its rows sees (jstop); for
// every block j in jstop .. nb - 1 the combine pass would still add the term of an all-zero p block -- its scale from block_scale(0),
// NaN where the dtype's epsilon is zero; the block sum zero; V's scale, NaN for a NaN block -- so the wave adds exactly that term,
// rescale() of the bare MAGIC_I, from V's exponent bytes alone.  With pout, p is zero from a row's visible length on.
// WIN: rows have a first key (att_first).  The blocks below the least first key of the wave's rows (j < jstart) get the same zero-block
// term, in block order before the first block the wave forms p for, and the chunks start at the workgroup's first seen one; p is zero
// below a row's first key too.
// PG (not with WIN): cap is a page's tokens and ldve its blocks; a 64-token chunk lies in one page, whose head is fetched once per chunk
// (head_tile), the next chunk's ahead of this chunk's loads; the zero-block terms look up the page of their block.
// C4 (block 64): vc holds nibbles, widened on the way into LDS as in k_kv_qk_rows.
template <int BLK, int DT, bool WIN = false, bool PG = false, bool C4 = false>
__global__ void __launch_bounds__(256) k_kv_pv_rows(const float* __restrict__ ws, const int8_t* __restrict__ vc, const int8_t* __restrict__ ve,
                                                    void* __restrict__ out, void* __restrict__ pout, const int32_t* __restrict__ lens, int heads,
                                                    int Tq, int L, int D, int pitch, int cap, int ldve, int ldo, int ldp, int xm, int wm,
                                                    float eps_dt, const uint8_t* __restrict__ exp_win, int causal, int group, int row0, int rows,
                                                    const int32_t* __restrict__ starts, int window, Pages pg)
{
    static_assert(!PG || !WIN, "a paged cache has no first key");
    static_assert(!C4 || BLK == 64, "4-bit codes: block 64");
    using Blk = I8Blk<BLK>;
    using op_t = typename Blk::op_t;
    using Tr = Traits<DT>;
    using raw_t = typename Tr::raw_t;
    constexpr int NBS = 64 / BLK, NE = BLK == 64 ? 16 : 8, LN = LdsOp<BLK>::LN;
    extern __shared__ uint4 s_dyn[];
    __shared__ uint8_t s_win[BFPQ_EXP_WIN_ENTRIES];
    __shared__ float s_red[2 * kRowsWg * 4];                     // per row and wave: the maximum, then the sum
    const int ndt = D >> 4;
    op_t* const s_v = reinterpret_cast<op_t*>(s_dyn);             // [ndt][NBS][LN]
    int8_t* const s_ve = reinterpret_cast<int8_t*>(s_v + ndt * NBS * LN);   // [NBS][D]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 15, q = l >> 4;
    const int PR = group * rows, nwg = (PR + kRowsWg - 1) / kRowsWg;
    const int bh = (int)blockIdx.x / nwg, pr0 = ((int)blockIdx.x % nwg) * kRowsWg;
    const int nrw = PR - pr0 < kRowsWg ? PR - pr0 : kRowsWg;      // the workgroup's rows
    int hbN = 0, slN = 0;                                        // (PG) the head and the first token of the chunk to come: the first,
    if constexpr (PG) hbN = head_tile<true>(pg, bh, heads, 0, slN);   // fetched beside the length
    const int len = lens[bh / heads];
    const int Kx = clamp_len(len, L);
    auto row_vis = [&](int i) __attribute__((always_inline)) { return att_visible(len, Kx, Tq, row0 + (pr0 + i) % rows, causal); };
    const int start = WIN ? seq_start(starts, bh / heads) : 0;
    auto row_lo = [&](int i) __attribute__((always_inline)) { return att_first(len, Tq, row0 + (pr0 + i) % rows, causal, start, window); };   // (WIN)
    load_exp_win(s_win, exp_win);
    row_stats<4, kRowsWg, WIN>(ws + ((size_t)bh * PR + pr0) * pitch, pitch, nrw, row_vis, row_lo, s_red);
    const int pw0 = pr0 + 16 * w, pr = pw0 + r;
    const bool tok = pr < PR;
    float rmax = 0.f, rsum = 1.f;
    int vis = 0, lo = 0;
    if (tok) {
        rmax = row_max(s_red, 16 * w + r);
        rsum = row_sum<kRowsWg>(s_red, 16 * w + r);
        vis = row_vis(16 * w + r);
        if constexpr (WIN) lo = row_lo(16 * w + r);
    }
    const int hq = tok ? pr / rows : 0, t = tok ? row0 + pr % rows : row0;
    const size_t grow = (size_t)bh * group * Tq + (size_t)hq * Tq + t;   // the lane's row of q, out and p
    const float* const srow = ws + ((size_t)bh * PR + (tok ? pr : pr0)) * pitch;
    raw_t* const prow = pout ? reinterpret_cast<raw_t*>(pout) + grow * ldp : nullptr;
    const int nb = (Kx + BLK - 1) / BLK;
    const int prl = pr0 + nrw - 1, pwl = pw0 + 15 < PR ? pw0 + 15 : PR - 1;
    const int vwg = range_visible(pr0, prl, rows, row0, len, Kx, Tq, causal);
    const int vw = pw0 < PR ? range_visible(pw0, pwl, rows, row0, len, Kx, Tq, causal) : 0;
    const int jstop = (vw + BLK - 1) / BLK;                       // (<= nb) blocks some row of the wave sees
    const v4i magic = {MAGIC_I, MAGIC_I, MAGIC_I, MAGIC_I};
    v2f acc[kMaxDT][2];
#pragma unroll
    for (int i = 0; i < kMaxDT; i++) acc[i][0] = acc[i][1] = v2f{0.f, 0.f};

    const int nchw = (vwg + 63) >> 6;
    int jstart = 0, cfirst = 0;                                  // (WIN) the first block some row of the wave sees, the workgroup's first chunk
    if constexpr (WIN) {
        const int lwg = range_first(pr0, prl, rows, row0, len, Tq, causal, start, window);
        const int lw = pw0 < PR ? range_first(pw0, pwl, rows, row0, len, Tq, causal, start, window) : 0;
        jstart = lw / BLK < jstop ? lw / BLK : jstop;
        cfirst = lwg >> 6 < nchw ? lwg >> 6 : nchw;
        if (jstart > 0) {                                        // the blocks below every first key of the wave: the term of a zero p block
            const BlockScale bs = block_scale<DT>(0u, xm, eps_dt, s_win);
            v2f sx, nm;
            token_scale((int)sat_exp(bs), xm, sx, nm);
            for (int j = 0; j < jstart; j++) {
#pragma unroll
                for (int i = 0; i < kMaxDT; i++) {
                    if (i < ndt) {
                        const int8_t* const we = ve + ((size_t)bh * D + 16 * i + 4 * q) * ldve + j;
                        v2f sw01, sw23;
                        weight_scales((int)we[0], (int)we[ldve], (int)we[2 * ldve], (int)we[3 * ldve], wm, sw01, sw23);
                        rescale(magic, sx, nm, sw01, sw23, acc[i][0], acc[i][1]);
                    }
                }
            }
        }
    }
    for (int c = WIN ? cfirst : 0; c < nchw; c++) {
        __syncthreads();                                         // (the chunk before this one read)
        if constexpr (PG) {
            const int hb = hbN, t0 = slN;                        // the chunk's head and its first token there
            if (c + 1 < nchw) hbN = head_tile<true>(pg, bh, heads, (c + 1) << 6, slN);
            for (int idx = tid; idx < ndt * NBS * LN; idx += 256) {
                const int ls = idx % LN, s = (idx / LN) % NBS, i = idx / (LN * NBS);
                if constexpr (C4) s_v[idx] = load_c4(vc, ((size_t)hb * D + 16 * i + (ls & 15)) * cap + t0 + s * BLK + Blk::lane(ls >> 4));
                else s_v[idx] = *reinterpret_cast<const op_t*>(vc + ((size_t)hb * D + 16 * i + (ls & 15)) * cap + t0 + s * BLK + Blk::lane(ls >> 4));
            }
            for (int idx = tid; idx < NBS * D; idx += 256)
                s_ve[idx] = c * NBS + idx / D < nb ? ve[((size_t)hb * D + idx % D) * ldve + t0 / BLK + idx / D] : (int8_t)0;
        } else {
            for (int idx = tid; idx < ndt * NBS * LN; idx += 256) {  // idx = (16-column tile i, block s of the chunk, lane slot)
                const int ls = idx % LN, s = (idx / LN) % NBS, i = idx / (LN * NBS);
                if constexpr (C4) s_v[idx] = load_c4(vc, ((size_t)bh * D + 16 * i + (ls & 15)) * cap + (c << 6) + s * BLK + Blk::lane(ls >> 4));
                else s_v[idx] = *reinterpret_cast<const op_t*>(vc + ((size_t)bh * D + 16 * i + (ls & 15)) * cap + (c << 6) + s * BLK + Blk::lane(ls >> 4));
            }
            for (int idx = tid; idx < NBS * D; idx += 256) {
                const int j = c * NBS + idx / D;
                s_ve[idx] = j < nb ? ve[((size_t)bh * D + idx % D) * ldve + j] : (int8_t)0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NBS; s++) {
            const int j = c * NBS + s;
            if (j >= jstop) break;                               // (wave-uniform)
            if (WIN && j < jstart) continue;                     // (likewise)
            const int k0 = (c << 6) + s * BLK + Blk::lane(q);
            uint32_t xv[NE];
            form_p<DT, WIN>(srow, k0, lo, vis, rmax, rsum, prow, xv);
            BlockScale bs;
            const op_t bF = quant_operand<BLK, DT>(xv, abs_max<DT>(xv), xm, eps_dt, s_win, bs);
            v2f sx, nm;
            token_scale((int)sat_exp(bs), xm, sx, nm);
#pragma unroll
            for (int i = 0; i < kMaxDT; i++) {
                if (i < ndt) {                                   // (uniform)
                    op_t aF = s_v[(i * NBS + s) * LN + LdsOp<BLK>::slot(l)];
                    if (!Blk::a_live(q)) aF = op_t{};
                    v2f sw01, sw23;
                    weight_scales(*reinterpret_cast<const uint32_t*>(s_ve + s * D + 16 * i + 4 * q), wm, sw01, sw23);
                    rescale(Blk::mfma(aF, bF, magic), sx, nm, sw01, sw23, acc[i][0], acc[i][1]);
                }
            }
        }
    }
    if (pw0 >= PR) return;                                       // (wave-uniform; no barrier below) a wave without rows
    if (jstop < nb) {                                            // the blocks no row of the wave sees: the term of a zero p block
        const BlockScale bs = block_scale<DT>(0u, xm, eps_dt, s_win);
        v2f sx, nm;
        token_scale((int)sat_exp(bs), xm, sx, nm);
        for (int j = jstop; j < nb; j++) {
            size_t hb = bh;                                      // the head the block's exponents lie in, and the block there
            int jl = j;
            if constexpr (PG) {
                int sl;
                hb = head_tile<true>(pg, bh, heads, j * BLK, sl);
                jl = sl / BLK;
            }
#pragma unroll
            for (int i = 0; i < kMaxDT; i++) {
                if (i < ndt) {
                    const int8_t* const we = ve + (hb * D + 16 * i + 4 * q) * ldve + jl;
                    v2f sw01, sw23;
                    weight_scales((int)we[0], (int)we[ldve], (int)we[2 * ldve], (int)we[3 * ldve], wm, sw01, sw23);
                    rescale(magic, sx, nm, sw01, sw23, acc[i][0], acc[i][1]);
                }
            }
        }
    }
    if (tok) {
#pragma unroll
        for (int i = 0; i < kMaxDT; i++)
            if (i < ndt) store4<DT>(out, grow * ldo + 16 * i + 4 * q, acc[i][0], acc[i][1]);
    }
    if (pout) {                                                  // +0 at what the wave's rows do not see
        for (int i = 0; i < 16 && pw0 + i < PR; i++) {
            const int p = pw0 + i;
            raw_t* const pr_i = reinterpret_cast<raw_t*>(pout) + ((size_t)bh * group * Tq + (size_t)(p / rows) * Tq + row0 + p % rows) * ldp;
            for (int k = row_vis(16 * w + i) + l; k < L; k += 64) pr_i[k] = (raw_t)0;
            if constexpr (WIN) {
                const int e = row_lo(16 * w + i) < L ? row_lo(16 * w + i) : L;
                for (int k = l; k < e; k += 64) pr_i[k] = (raw_t)0;
            }
        }
    }
}

constexpr int64_t kLim = (int64_t)1 << 31;

// f(std::true_type{}) or f(std::false_type{}) for a flag known at run time
template <class F> void with_flag(bool on, F&& f)
{
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

// the tiles of 16 rows a head's group * Tq rows make
inline int64_t row_tiles(int64_t Tq, int64_t group) { return (Tq * group + 15) / 16; }

// the qk product of a device-length cache (arguments checked by the entries): MODE kDev writes the dtype, kAtt the fp32 softmax input.
// x [B, group * Tq, ldx]; group > 1 runs the GRP instances, WIN (kAtt) those with a first key per row (starts or null, window or 0)
// pages (or null; not with WIN): the PG instances, w_bstride then a page's tokens.  c4: the C4 instances (block 64, checked by the entries)
template <int MODE, bool WIN = false>
void qk_dev(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads, int64_t Tq,
            int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo, int dtype, int block_size, int xm, int wm,
            float eps_dt, const uint8_t* exp_win, float scale, int causal, hipStream_t s, const int32_t* starts = nullptr, int window = 0,
            const Pages* pages = nullptr, bool c4 = false)
{
    const int64_t ny = B * row_tiles(Tq, group);
    const unsigned gy = (unsigned)(ny < 65535 ? ny : 65535);
    with_block(block_size, [&](auto blk) {
        with_dtype(dtype, [&](auto dt) {
            auto go = [&](auto grp, auto paged, auto nib) {
                constexpr int TM = decltype(blk)::value == 64 ? 4 : 2;
                constexpr bool PG = decltype(paged)::value, C4 = decltype(nib)::value;
                if constexpr (!C4 || decltype(blk)::value == 64)
                    hipLaunchKernelGGL((k_kv_bmm_dec<decltype(blk)::value, decltype(dt)::value, TM, MODE, decltype(grp)::value, WIN && !PG, PG, C4>),
                                       dim3((unsigned)((Nout + 64 * TM - 1) / (64 * TM)), gy), dim3(256), 0, s, x, (const int8_t*)wcodes, wexp, out, (int)B,
                                       (int)Tq, (int)Kx, (int)Nout, (int)ldx, (int)ldw, (int)ldwe, (int)w_bstride, (int)ldo, xm, wm, eps_dt, exp_win, lens,
                                       (int)heads, scale, causal, (int)group, starts, window, PG ? *pages : Pages{});
            };
            if (c4) with_flag(group > 1, [&](auto grp) { with_flag(pages != nullptr, [&](auto paged) { go(grp, paged, std::true_type{}); }); });
            else if (pages) group > 1 ? go(std::true_type{}, std::true_type{}, std::false_type{}) : go(std::false_type{}, std::true_type{}, std::false_type{});
            else if (group > 1) go(std::true_type{}, std::false_type{}, std::false_type{});
            else go(std::false_type{}, std::false_type{}, std::false_type{});
        });
    });
}

// the split p v product and its combine pass (arguments checked by the entries).  ATT: x holds fp32 score rows (k_kv_pv_split).
// x and out hold R = group * Tq rows per head; the combine pass works per row and takes R for its Tq.  WIN (ATT): as qk_dev
// pages (or null; not with WIN): the PG instances, ldw then a page's tokens and ldwe its blocks
template <bool ATT, bool WIN = false>
int pv_dev(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads, int64_t Tq,
           int64_t group, int64_t Kx, int64_t D, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t ldo, int dtype, int block_size, int xm, int wm, float eps_dt,
           const uint8_t* exp_win, void* ws, int64_t chunks_per_split, void* pout, int64_t ldp, int causal, hipStream_t s,
           const int32_t* starts = nullptr, int window = 0, const Pages* pages = nullptr, bool c4 = false)
{
    const int64_t nb = (Kx + block_size - 1) / block_size, nch = (Kx + 63) / 64, dg = (D + 63) / 64;
    const int64_t R = group * Tq, gz = B * row_tiles(Tq, group);  // a workgroup per (head, row tile) on the grid's z
    int64_t cps = chunks_per_split;
    if (cps == 0)                                                 // the shortest slices that keep the grid within kSplitGrid workgroups
        for (cps = 1; cps < kMaxCps && (nch + cps - 1) / cps * dg * gz > kSplitGrid; cps++) {}
    const int64_t slices = (nch + cps - 1) / cps;
    if (slices > 65535 || gz > 65535) return BFPQ_E_UNSUPPORTED;
    int32_t* const sums = (int32_t*)ws;
    int8_t* const xexp = (int8_t*)ws + B * R * nb * 4 * D;
    const int xvec = !ATT && (reinterpret_cast<uintptr_t>(x) & 15u) == 0 && (ldx * bfpq_dev::dtype_size(dtype)) % 16 == 0;
    with_block(block_size, [&](auto blk) {
        with_dtype(dtype, [&](auto dt) {
            auto go = [&](auto grp, auto paged, auto nib) {
                constexpr bool PG = decltype(paged)::value, C4 = decltype(nib)::value;
                if constexpr (!C4 || decltype(blk)::value == 64)
                    hipLaunchKernelGGL((k_kv_pv_split<decltype(blk)::value, decltype(dt)::value, ATT, decltype(grp)::value, WIN && !PG, PG, C4>),
                                       dim3((unsigned)dg, (unsigned)slices, (unsigned)gz), dim3(256), 0, s, x, (const int8_t*)wcodes, sums, xexp, lens,
                                       (int)heads, (int)Tq, (int)Kx, (int)D, (int)ldx, (int)ldw, (int)nb, (int)cps, xvec, xm, eps_dt, exp_win, pout,
                                       (int)ldp, causal, (int)group, starts, window, PG ? *pages : Pages{});
            };
            if (c4) with_flag(group > 1, [&](auto grp) { with_flag(pages != nullptr, [&](auto paged) { go(grp, paged, std::true_type{}); }); });
            else if (pages) group > 1 ? go(std::true_type{}, std::true_type{}, std::false_type{}) : go(std::false_type{}, std::true_type{}, std::false_type{});
            else if (group > 1) go(std::true_type{}, std::false_type{}, std::false_type{});
            else go(std::false_type{}, std::false_type{}, std::false_type{});
        });
    });
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    const int64_t total = B * R * (D / 4);
    with_dtype(dtype, [&](auto dt) {
        auto go = [&](auto paged) {
            constexpr bool PG = decltype(paged)::value;
            hipLaunchKernelGGL((k_kv_pv_combine<decltype(dt)::value, PG>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sums, xexp, wexp, out,
                               lens, (int)heads, total, (int)R, (int)Kx, (int)D, (int)ldwe, (int)nb, (int)ldo, block_size, xm, wm, PG ? *pages : Pages{});
        };
        if (pages) go(std::true_type{});
        else go(std::false_type{});
    });
    return (int)hipGetLastError();
}

// ---- what the entries check alike.  Each entry runs the three steps in this order -- values (BFPQ_E_ARG), "nothing to do", shapes
// (BFPQ_E_UNSUPPORTED), pointers (BFPQ_E_ARG) -- with its own conditions beside the shared ones of the same step ----------------------------
// bfpq_kv_bmm_dec and bfpq_kv_bmm_dec_gqa; x and out hold R rows per head
inline bool dec_values_ok(int dtype, int block_size, int xm, int wm, int family, int64_t B, int64_t Tq, int64_t Nout, int64_t Kx)
{
    return dtype_ok(dtype) && i8_block_ok(block_size) && i8_mant_ok(xm) && i8_mant_ok(wm) && (family == BFPQ_KV_QK || family == BFPQ_KV_PV) &&
           B >= 0 && Tq >= 0 && Nout >= 0 && Kx >= 0;
}
inline bool dec_shapes_ok(int family, int block_size, int64_t Tq, int64_t R, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe,
                          int64_t w_bstride, int64_t ldo)
{
    const int64_t nb = (Kx + block_size - 1) / block_size;
    return Tq <= BFPQ_KV_DEC_MAX_TOKENS && Kx >= 1 && (family == BFPQ_KV_QK ? Kx % block_size == 0 : Nout % 16 == 0) && ldx >= Kx &&
           ldw % 64 == 0 && ldw >= (Kx + 63) / 64 * 64 && ldwe >= nb && w_bstride >= Nout && ldo % 4 == 0 && ldo >= Nout &&
           w_bstride * ldw < kLim && w_bstride * ldwe < kLim && R * ldx < kLim && R * ldo < kLim;
}
inline bool dec_ptrs_ok(const void* x, const void* wcodes, const void* wexp, const void* out, const void* exp_win, int dtype)
{
    return x && wcodes && wexp && out && exp_win && aligned16(wcodes, out) && !(reinterpret_cast<uintptr_t>(x) & (dtype == BFPQ_F32 ? 3u : 1u));
}

// bfpq_kv_attend_gqa and bfpq_kv_attend_rows
inline bool att_values_ok(int dtype, int block_size, int xm, int wm, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t chunks_per_split,
                          int causal, double scale)
{
    return dtype_ok(dtype) && i8_block_ok(block_size) && i8_mant_ok(xm) && i8_mant_ok(wm) && BH >= 0 && Tq >= 0 && heads >= 1 && BH % heads == 0 &&
           group >= 1 && chunks_per_split >= 0 && (causal == 0 || causal == 1) && scale - scale == 0.0 && (float)scale - (float)scale == 0.f;
}
inline bool att_shapes_ok(int block_size, int64_t group, int64_t D, int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp,
                          const void* p_out, int64_t chunks_per_split)
{
    return bfpq_kv_ok(D, cap, block_size) && group < kLim && max_len >= 1 && max_len <= cap && ldd >= D && ldd % 64 == 0 && ldo % 4 == 0 &&
           ldo >= D && !(p_out && ldp < max_len) && cap * ldd < kLim && chunks_per_split <= kMaxCps;
}
inline bool att_ptrs_ok(const void* q, const void* k_codes, const void* k_exps, const void* v_codes, const void* v_exps, const void* out,
                        const void* p_out, const void* lens, const void* exp_win, const void* score_ws, int dtype)
{
    return q && k_codes && k_exps && v_codes && v_exps && out && lens && exp_win && score_ws && aligned16(k_codes, v_codes, out, score_ws) &&
           !(reinterpret_cast<uintptr_t>(lens) & 3u) && !(reinterpret_cast<uintptr_t>(p_out) & (dtype == BFPQ_F32 ? 3u : 1u));
}

// the _win entries: a window of 0 is none, and so is one no length reaches
inline bool win_values_ok(const int32_t* starts, int64_t window) { return window >= 0 && !(reinterpret_cast<uintptr_t>(starts) & 3u); }
inline int win_arg(int64_t window) { return window < kLim ? (int)window : 0; }

// the _paged entries: cap is the most tokens of a sequence, the table cap / page_tokens entries wide; the cache tensors hold
// `pages` pages of `heads` heads of page_tokens tokens.  The values (BFPQ_E_ARG), the sizes (BFPQ_E_UNSUPPORTED), the table (BFPQ_E_ARG)
inline bool pages_values_ok(int64_t page_tokens, int64_t pages, int64_t cap)
{
    return page_tokens >= 64 && page_tokens % 64 == 0 && pages >= 1 && cap >= page_tokens && cap % page_tokens == 0;
}
inline bool pages_shapes_ok(int64_t page_tokens, int64_t pages, int64_t heads, int64_t D, int64_t ldd, int block_size)
{
    return bfpq_kv_ok(D, page_tokens, block_size) && page_tokens * ldd < kLim && pages * heads < kLim;
}
inline bool pages_ptr_ok(const int32_t* table) { return table && !(reinterpret_cast<uintptr_t>(table) & 3u); }
inline Pages pages_arg(const int32_t* table, int64_t page_tokens, int64_t pages, int64_t cap)
{
    return Pages{table, (int)(cap / page_tokens), (int)page_tokens, (int)pages};
}

// the _cb entries: the code tensors hold int8 codes (8) or, at block 64 and mant_bits <= 3, nibbles (4)
inline bool code_bits_ok(int code_bits, int block_size, int mant_bits)
{
    return code_bits == 8 || (code_bits == 4 && block_size == 64 && mant_bits <= 3);
}

// bfpq_kv_attend_gqa (win false: starts and window are unread), bfpq_kv_attend_gqa_win, _paged and (c4) _cb
int attend_gqa(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out, void* p_out,
               const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len, int64_t cap, int64_t ldd,
               int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
               const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes, void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split,
               bool win, const int32_t* starts, int64_t window, void* stream, const Pages* pages = nullptr, bool c4 = false)
{
    if (!att_values_ok(dtype, block_size, x_mant_bits, w_mant_bits, BH, heads, Tq, group, chunks_per_split, causal, scale) ||
        (win && !win_values_ok(starts, window)) || (pages && !pages_values_ok(pages->tokens, pages->count, cap)))
        return BFPQ_E_ARG;
    if (BH == 0 || Tq == 0) return 0;
    const int64_t pitch = (max_len + 3) / 4 * 4, R = Tq * group;
    const int64_t hcap = pages ? pages->tokens : cap;             // tokens of a head of the cache tensors
    if (!att_shapes_ok(block_size, group, D, max_len, cap, ldd, ldo, ldp, p_out, chunks_per_split) || Tq > BFPQ_KV_DEC_MAX_TOKENS ||
        R * ldo >= kLim || R * pitch >= kLim || (p_out && R * ldp >= kLim) || BH * row_tiles(Tq, group) > 65535 ||
        (pages && !pages_shapes_ok(pages->tokens, pages->count, heads, D, ldd, block_size)))
        return BFPQ_E_UNSUPPORTED;
    const int64_t need_s = bfpq_kv_attend_ws_bytes(BH * group, Tq, max_len), need_p = bfpq_kv_dec_ws_bytes(BH * group, Tq, D, max_len, block_size);
    if (need_s < 0 || need_p < 0 || score_ws_bytes < need_s || sum_ws_bytes < need_p) return BFPQ_E_UNSUPPORTED;
    if (!att_ptrs_ok(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, exp_win, score_ws, dtype) || !sum_ws || !aligned16(sum_ws) ||
        (reinterpret_cast<uintptr_t>(q) & (dtype == BFPQ_F32 ? 3u : 1u)) || (pages && !pages_ptr_ok(pages->table)))
        return BFPQ_E_ARG;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    hipStream_t s = (hipStream_t)stream;
    auto go = [&](auto w) {
        constexpr bool WIN = decltype(w)::value;
        qk_dev<kAtt, WIN>(q, k_codes, k_exps, score_ws, lens, BH, heads, Tq, group, D, max_len, D, ldd, D / block_size, hcap, pitch, dtype, block_size,
                          x_mant_bits, w_mant_bits, eps_dt, exp_win, (float)scale, causal, s, starts, win_arg(window), pages, c4);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
        return pv_dev<true, WIN>(score_ws, v_codes, v_exps, out, lens, BH, heads, Tq, group, max_len, D, pitch, hcap, hcap / block_size, ldo, dtype,
                                 block_size, x_mant_bits, w_mant_bits, eps_dt, exp_win, sum_ws, chunks_per_split, p_out, ldp, causal, s, starts,
                                 win_arg(window), pages, c4);
    };
    return win && (starts || win_arg(window)) ? go(std::true_type{}) : go(std::false_type{});
}

// bfpq_kv_attend_rows and bfpq_kv_attend_rows_win, likewise
int attend_rows(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out, void* p_out,
                const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len, int64_t cap, int64_t ldd,
                int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows, bool win,
                const int32_t* starts, int64_t window, void* stream, const Pages* pages = nullptr, bool c4 = false)
{
    if (!att_values_ok(dtype, block_size, x_mant_bits, w_mant_bits, BH, heads, Tq, group, chunks_per_split, causal, scale) || row0 < 0 || rows < 0 ||
        row0 > Tq || rows > Tq - row0 || (win && !win_values_ok(starts, window)) || (pages && !pages_values_ok(pages->tokens, pages->count, cap)))
        return BFPQ_E_ARG;
    if (BH == 0 || Tq == 0 || rows == 0) return 0;
    const int64_t pitch = (max_len + 3) / 4 * 4, R = Tq * group, PR = rows * group, nwg = (PR + kRowsWg - 1) / kRowsWg;
    if (!att_shapes_ok(block_size, group, D, max_len, cap, ldd, ldo, ldp, p_out, chunks_per_split) || D > 16 * kMaxDT || Tq >= kLim || R >= kLim ||
        BH * nwg >= kLim || (pages && !pages_shapes_ok(pages->tokens, pages->count, heads, D, ldd, block_size)))
        return BFPQ_E_UNSUPPORTED;
    const int64_t need = bfpq_kv_attend_rows_ws_bytes(BH * group, rows, max_len);
    if (need < 0 || score_ws_bytes < need) return BFPQ_E_UNSUPPORTED;
    if (!att_ptrs_ok(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, exp_win, score_ws, dtype) || !aligned16(q) ||
        (pages && !pages_ptr_ok(pages->table)))
        return BFPQ_E_ARG;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nbd = D / block_size, hcap = pages ? pages->tokens : cap;   // (hcap: tokens of a head of the cache tensors)
    const size_t lds_qk = (size_t)(2 * 64 * D + 128 * nbd), lds_pv = (size_t)(64 * D + 64 / block_size * D);   // <= 36 KiB at D = 256
    auto go = [&](auto w, auto paged, auto nib) {
        constexpr bool WIN = decltype(w)::value, PG = decltype(paged)::value, C4 = decltype(nib)::value;
        with_block(block_size, [&](auto blk) {
            with_dtype(dtype, [&](auto dt) {
                if constexpr (!C4 || decltype(blk)::value == 64)
                    hipLaunchKernelGGL((k_kv_qk_rows<decltype(blk)::value, decltype(dt)::value, WIN, PG, C4>), dim3((unsigned)(BH * nwg)), dim3(256), lds_qk,
                                       s, q, (const int8_t*)k_codes, k_exps, (float*)score_ws, (int)Tq, (int)D, (int)max_len, (int)ldd, (int)hcap, (int)pitch,
                                       x_mant_bits, w_mant_bits, eps_dt, exp_win, lens, (int)heads, (float)scale, causal, (int)group, (int)row0, (int)rows,
                                       starts, win_arg(window), PG ? *pages : Pages{});
            });
        });
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
        with_block(block_size, [&](auto blk) {
            with_dtype(dtype, [&](auto dt) {
                if constexpr (!C4 || decltype(blk)::value == 64)
                    hipLaunchKernelGGL((k_kv_pv_rows<decltype(blk)::value, decltype(dt)::value, WIN, PG, C4>), dim3((unsigned)(BH * nwg)), dim3(256), lds_pv,
                                       s, (const float*)score_ws, (const int8_t*)v_codes, v_exps, out, p_out, lens, (int)heads, (int)Tq, (int)max_len, (int)D,
                                       (int)pitch, (int)hcap, (int)(hcap / block_size), (int)ldo, (int)ldp, x_mant_bits, w_mant_bits, eps_dt, exp_win,
                                       causal, (int)group, (int)row0, (int)rows, starts, win_arg(window), PG ? *pages : Pages{});
            });
        });
        return (int)hipGetLastError();
    };
    const bool first_keys = win && (starts || win_arg(window));
    if (c4) {
        if (pages) return go(std::false_type{}, std::true_type{}, std::true_type{});
        return first_keys ? go(std::true_type{}, std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{}, std::true_type{});
    }
    if (pages) return go(std::false_type{}, std::true_type{}, std::false_type{});
    return first_keys ? go(std::true_type{}, std::false_type{}, std::false_type{}) : go(std::false_type{}, std::false_type{}, std::false_type{});
}

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
        hipLaunchKernelGGL((k_kv_append<decltype(dt)::value, false>), dim3((unsigned)(nkb + nvb)), dim3(256), 0, (hipStream_t)stream, k_new, v_new,
                           (int8_t*)k_codes, k_exps, (int8_t*)v_codes, v_exps, v_tail, (int)BH, (int)D, (int)pos, (int)t, (int)cap, (int)ldd,
                           block_size, mant_bits, eps_dt, exp_win, (int)nkb, (int)zc, nullptr, nullptr, nullptr, 1, 0, Pages{});
    });
    return (int)hipGetLastError();
}

int bfpq_kv_bmm_dec(const void* x, const void* wcodes, const int8_t* wexp, void* out, int64_t B, int64_t Tq, int64_t Kx, int64_t Nout,
                    int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo, int family, int dtype, int block_size,
                    int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* stream)
{
    if (!dec_values_ok(dtype, block_size, x_mant_bits, w_mant_bits, family, B, Tq, Nout, Kx)) return BFPQ_E_ARG;
    if (B == 0 || Tq == 0 || Nout == 0) return 0;
    if (!dec_shapes_ok(family, block_size, Tq, Tq, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo)) return BFPQ_E_UNSUPPORTED;
    if (!dec_ptrs_ok(x, wcodes, wexp, out, exp_win, dtype)) return BFPQ_E_ARG;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    hipStream_t s = (hipStream_t)stream;
    const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
    with_block(block_size, [&](auto blk) {
        with_dtype(dtype, [&](auto dt) {
            auto go = [&](auto tmc) {
                constexpr int TM = decltype(tmc)::value;
                hipLaunchKernelGGL((k_kv_bmm_dec<decltype(blk)::value, decltype(dt)::value, TM, kHost>),
                                   dim3((unsigned)((Nout + 64 * TM - 1) / (64 * TM)), gy), dim3(256), 0, s, x, (const int8_t*)wcodes, wexp, out, (int)B,
                                   (int)Tq, (int)Kx, (int)Nout, (int)ldx, (int)ldw, (int)ldwe, (int)w_bstride, (int)ldo, x_mant_bits, w_mant_bits,
                                   eps_dt, exp_win, nullptr, 1, 1.f, 0, 1, nullptr, 0, Pages{});
            };
            // rows per wave: 64 (32 at the small blocks) of the many cached keys, 16 of V's D columns
            if (family == BFPQ_KV_PV) go(std::integral_constant<int, 1>{});
            else if constexpr (decltype(blk)::value == 64) go(std::integral_constant<int, 4>{});
            else go(std::integral_constant<int, 2>{});
        });
    });
    return (int)hipGetLastError();
}

// bfpq_kv_append_dev (pages null), bfpq_kv_append_paged and (c4) bfpq_kv_append_cb
static int append_dev(const void* k_new, const void* v_new, void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail,
                      const int32_t* lens, const int32_t* counts, int32_t* overflow, int64_t BH, int64_t heads, int64_t D, int64_t t,
                      int64_t cap, int64_t limit, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon,
                      const uint8_t* exp_win, void* stream, const Pages* pages, bool c4 = false)
{
    if (!dtype_ok(dtype) || !i8_block_ok(block_size) || !i8_mant_ok(mant_bits) || BH < 0 || t < 0 || heads < 1 || BH % heads != 0 ||
        (pages && !pages_values_ok(pages->tokens, pages->count, cap)))
        return BFPQ_E_ARG;
    if (!bfpq_kv_ok(D, cap, block_size) || ldd < D || ldd % 64 != 0 || limit < 1 || limit > cap || t > cap || BH >= kLim ||
        (pages && !pages_shapes_ok(pages->tokens, pages->count, heads, D, ldd, block_size)))
        return BFPQ_E_UNSUPPORTED;
    if (BH == 0 || t == 0) return 0;
    if (!k_new || !v_new || !k_codes || !k_exps || !v_codes || !v_exps || !v_tail || !lens || !overflow || !exp_win ||
        !aligned16(k_new, v_new, k_codes, v_codes, v_tail) || ((reinterpret_cast<uintptr_t>(lens) | reinterpret_cast<uintptr_t>(counts) |
                                                                 reinterpret_cast<uintptr_t>(overflow)) & 3u) ||
        (pages && !pages_ptr_ok(pages->table)))
        return BFPQ_E_ARG;
    const int64_t nkb = (BH * t * (D / 16) + 255) / 256;
    // the token blocks of V a chunk of t can touch at the worst position (its first token the last of a block)
    const int64_t nblk = (t + block_size - 2) / block_size + 1, zc = nblk > 1 ? nblk - 1 : 1;
    const int64_t nvb = BH * ((D + kTD - 1) / kTD) * zc;
    if (nkb + nvb >= kLim) return BFPQ_E_UNSUPPORTED;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    with_dtype(dtype, [&](auto dt) {
        auto go = [&](auto paged, auto nib) {
            constexpr bool PG = decltype(paged)::value;           // (PG: the kernel's cap is a page's tokens)
            hipLaunchKernelGGL((k_kv_append<decltype(dt)::value, true, PG, decltype(nib)::value>), dim3((unsigned)(nkb + nvb)), dim3(256), 0, (hipStream_t)stream, k_new,
                               v_new, (int8_t*)k_codes, k_exps, (int8_t*)v_codes, v_exps, v_tail, (int)BH, (int)D, 0, (int)t,
                               (int)(PG ? pages->tokens : cap), (int)ldd, block_size, mant_bits, eps_dt, exp_win, (int)nkb, (int)zc, lens, counts,
                               overflow, (int)heads, (int)limit, PG ? *pages : Pages{});
        };
        if (c4) with_flag(pages != nullptr, [&](auto paged) { go(paged, std::true_type{}); });
        else if (pages) go(std::true_type{}, std::false_type{});
        else go(std::false_type{}, std::false_type{});
    });
    return (int)hipGetLastError();
}

int bfpq_kv_append_dev(const void* k_new, const void* v_new, void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail,
                       const int32_t* lens, const int32_t* counts, int32_t* overflow, int64_t BH, int64_t heads, int64_t D, int64_t t,
                       int64_t cap, int64_t limit, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon,
                       const uint8_t* exp_win, void* stream)
{
    return append_dev(k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, lens, counts, overflow, BH, heads, D, t, cap, limit, ldd, dtype,
                      block_size, mant_bits, epsilon, exp_win, stream, nullptr);
}

// bfpq_kv_lens_advance (pages null) and bfpq_kv_lens_advance_paged
static int lens_advance(int32_t* lens, const int32_t* counts, int64_t B, int64_t t, int64_t limit, void* stream, const Pages* pages)
{
    if (B < 0 || t < 0 || limit < 1 || (pages && !pages_values_ok(pages->tokens, pages->count, (int64_t)pages->width * pages->tokens)))
        return BFPQ_E_ARG;
    if (B >= kLim || t >= kLim || limit >= kLim || (pages && limit > (int64_t)pages->width * pages->tokens)) return BFPQ_E_UNSUPPORTED;
    if (B == 0 || t == 0) return 0;
    if (!lens || ((reinterpret_cast<uintptr_t>(lens) | reinterpret_cast<uintptr_t>(counts)) & 3u) || (pages && !pages_ptr_ok(pages->table)))
        return BFPQ_E_ARG;
    if (pages)
        hipLaunchKernelGGL(k_kv_advance<true>, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lens, counts, (int)B, (int)t,
                           (int)limit, *pages);
    else
        hipLaunchKernelGGL(k_kv_advance<false>, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lens, counts, (int)B, (int)t,
                           (int)limit, Pages{});
    return (int)hipGetLastError();
}

int bfpq_kv_lens_advance(int32_t* lens, const int32_t* counts, int64_t B, int64_t t, int64_t limit, void* stream)
{
    return lens_advance(lens, counts, B, t, limit, stream, nullptr);
}

int64_t bfpq_kv_dec_ws_bytes(int64_t B, int64_t Tq, int64_t D, int64_t L, int block_size)
{
    if (!i8_block_ok(block_size) || B < 0 || Tq < 0 || D < 0 || L < 0) return BFPQ_E_ARG;
    if (Tq > BFPQ_KV_DEC_MAX_TOKENS || D % 16 != 0 || D > 1024 || L >= kLim || B >= kLim) return BFPQ_E_UNSUPPORTED;
    const int64_t nbw = (L + block_size - 1) / block_size;
    return (B * Tq * nbw * (4 * D + 1) + 15) / 16 * 16;           // the int32 block sums, then x's block exponents
}

// bfpq_kv_bmm_dec_gqa (pages null) and bfpq_kv_bmm_dec_paged: there the rows of a head are those of one page (ldw, ldwe and w_bstride as
// the entry documents them) and `cap` the most tokens of a sequence
static int bmm_dec_gqa(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads,
                       int64_t Tq, int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride,
                       int64_t ldo, int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                       const uint8_t* exp_win, void* ws, int64_t ws_bytes, int64_t chunks_per_split, void* stream, const Pages* pages, int64_t cap,
                       bool c4 = false)
{
    if (!dec_values_ok(dtype, block_size, x_mant_bits, w_mant_bits, family, B, Tq, Nout, Kx) || heads < 1 || B % heads != 0 || group < 1 ||
        chunks_per_split < 0 || (pages && !pages_values_ok(pages->tokens, pages->count, cap)))
        return BFPQ_E_ARG;
    if (B == 0 || Tq == 0) return 0;
    if (pages) {                                                  // the bounds of a whole sequence, then a page's as the head's
        const int64_t P = pages->tokens;
        if ((family == BFPQ_KV_QK ? Nout : Kx) > cap || pages->count * heads >= kLim ||
            (family == BFPQ_KV_QK ? w_bstride != P || ldw < Kx || ldwe < Kx / block_size
                                  : ldw != P || ldwe != P / block_size || w_bstride != Nout))
            return BFPQ_E_UNSUPPORTED;
        if (Tq > BFPQ_KV_DEC_MAX_TOKENS || group >= kLim || Kx < 1 || Nout < 1 || (family == BFPQ_KV_QK ? Kx % block_size != 0 : Nout % 16 != 0) ||
            ldx < Kx || ldw % 64 != 0 || ldo % 4 != 0 || ldo < Nout || w_bstride * ldw >= kLim || Tq * group * ldx >= kLim ||
            Tq * group * ldo >= kLim || (family == BFPQ_KV_PV && Nout > 1024) || B * row_tiles(Tq, group) >= kLim || chunks_per_split > kMaxCps)
            return BFPQ_E_UNSUPPORTED;
    } else if (Tq > BFPQ_KV_DEC_MAX_TOKENS || group >= kLim ||
               !dec_shapes_ok(family, block_size, Tq, Tq * group, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo) || Nout < 1 ||
               (family == BFPQ_KV_PV && Nout > 1024) || B * row_tiles(Tq, group) >= kLim || chunks_per_split > kMaxCps)
        return BFPQ_E_UNSUPPORTED;
    if (!dec_ptrs_ok(x, wcodes, wexp, out, exp_win, dtype) || !lens || (reinterpret_cast<uintptr_t>(lens) & 3u) ||
        (pages && !pages_ptr_ok(pages->table)))
        return BFPQ_E_ARG;
    const float eps_dt = bfpq_dev::h_round((float)epsilon, dtype);
    hipStream_t s = (hipStream_t)stream;
    if (family == BFPQ_KV_QK) {
        qk_dev<kDev>(x, wcodes, wexp, out, lens, B, heads, Tq, group, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, dtype, block_size, x_mant_bits, w_mant_bits,
                     eps_dt, exp_win, 1.f, 0, s, nullptr, 0, pages, c4);
        return (int)hipGetLastError();
    }
    // p v: w_bstride == Nout == D rows per head (the sums are laid out by D); a workgroup per (head, row tile) on the grid's z
    const int64_t need = bfpq_kv_dec_ws_bytes(B * group, Tq, Nout, Kx, block_size);
    if (w_bstride != Nout || B * row_tiles(Tq, group) > 65535 || need < 0 || ws_bytes < need) return BFPQ_E_UNSUPPORTED;
    if (!ws || !aligned16(ws)) return BFPQ_E_ARG;
    return pv_dev<false>(x, wcodes, wexp, out, lens, B, heads, Tq, group, Kx, Nout, ldx, ldw, ldwe, ldo, dtype, block_size, x_mant_bits, w_mant_bits,
                         eps_dt, exp_win, ws, chunks_per_split, nullptr, 0, 0, s, nullptr, 0, pages, c4);
}

int bfpq_kv_bmm_dec_gqa(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads,
                        int64_t Tq, int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride,
                        int64_t ldo, int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                        const uint8_t* exp_win, void* ws, int64_t ws_bytes, int64_t chunks_per_split, void* stream)
{
    return bmm_dec_gqa(x, wcodes, wexp, out, lens, B, heads, Tq, group, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, family, dtype, block_size,
                       x_mant_bits, w_mant_bits, epsilon, exp_win, ws, ws_bytes, chunks_per_split, stream, nullptr, 0);
}

int bfpq_kv_bmm_dec_dev(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads,
                        int64_t Tq, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo, int family,
                        int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* ws,
                        int64_t ws_bytes, int64_t chunks_per_split, void* stream)
{
    return bfpq_kv_bmm_dec_gqa(x, wcodes, wexp, out, lens, B, heads, Tq, 1, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, family, dtype, block_size,
                               x_mant_bits, w_mant_bits, epsilon, exp_win, ws, ws_bytes, chunks_per_split, stream);
}

int64_t bfpq_kv_attend_ws_bytes(int64_t B, int64_t Tq, int64_t L)
{
    if (B < 0 || Tq < 0 || L < 0) return BFPQ_E_ARG;
    if (Tq > BFPQ_KV_DEC_MAX_TOKENS || L >= kLim || B >= kLim) return BFPQ_E_UNSUPPORTED;
    return (B * Tq * ((L + 3) / 4 * 4) * 4 + 15) / 16 * 16;       // the fp32 score rows, pitch L rounded up to 4
}

int bfpq_kv_attend_gqa(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out, void* p_out,
                       const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len, int64_t cap,
                       int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits,
                       int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes, void* sum_ws,
                       int64_t sum_ws_bytes, int64_t chunks_per_split, void* stream)
{
    return attend_gqa(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype,
                      block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split,
                      false, nullptr, 0, stream);
}

int bfpq_kv_attend_gqa_win(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out,
                           void* p_out, const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len,
                           int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                           int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes,
                           void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split, const int32_t* starts, int64_t window, void* stream)
{
    return attend_gqa(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype,
                      block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split,
                      true, starts, window, stream);
}

int bfpq_kv_attend(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out, void* p_out,
                   const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t D, int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo,
                   int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                   const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes, void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split,
                   void* stream)
{
    return bfpq_kv_attend_gqa(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, 1, D, max_len, cap, ldd, ldo, ldp, scale, causal,
                              dtype, block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes,
                              chunks_per_split, stream);
}

int64_t bfpq_kv_attend_rows_ws_bytes(int64_t BH, int64_t P, int64_t max_len)
{
    if (BH < 0 || P < 0 || max_len < 0) return BFPQ_E_ARG;
    if (max_len >= kLim || BH >= kLim || P >= kLim) return BFPQ_E_UNSUPPORTED;
    const int64_t n = BH * P * ((max_len + 3) / 4 * 4);           // the fp32 score rows of a panel, pitch max_len rounded up to 4
    if (n >= kLim / 4 - 4) return BFPQ_E_UNSUPPORTED;
    return (n * 4 + 15) / 16 * 16;
}

int bfpq_kv_attend_rows(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out, void* p_out,
                        const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len, int64_t cap,
                        int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits,
                        int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes, void* sum_ws,
                        int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows, void* stream)
{
    (void)sum_ws; (void)sum_ws_bytes;                             // no block sums on this route
    return attend_rows(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal,
                       dtype, block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, chunks_per_split, row0, rows, false,
                       nullptr, 0, stream);
}

int bfpq_kv_attend_rows_win(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out,
                            void* p_out, const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len,
                            int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                            int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes,
                            void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows, const int32_t* starts,
                            int64_t window, void* stream)
{
    (void)sum_ws; (void)sum_ws_bytes;
    return attend_rows(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal,
                       dtype, block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, chunks_per_split, row0, rows, true,
                       starts, window, stream);
}

// ---- the paged entries: the entry each extends with page_table, page_tokens and pages in front of the stream ------------------
#define BFPQ_PAGES_OR_RETURN(cap)                                                                          \
    if (!pages_values_ok(page_tokens, pages, cap)) return BFPQ_E_ARG;                                      \
    if (page_tokens >= kLim || pages >= kLim || (cap) >= kLim) return BFPQ_E_UNSUPPORTED;                  \
    const Pages pg = pages_arg(page_table, page_tokens, pages, cap)

int bfpq_kv_append_paged(const void* k_new, const void* v_new, void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail,
                         const int32_t* lens, const int32_t* counts, int32_t* overflow, int64_t BH, int64_t heads, int64_t D, int64_t t,
                         int64_t cap, int64_t limit, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon,
                         const uint8_t* exp_win, const int32_t* page_table, int64_t page_tokens, int64_t pages, void* stream)
{
    BFPQ_PAGES_OR_RETURN(cap);
    return append_dev(k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, lens, counts, overflow, BH, heads, D, t, cap, limit, ldd, dtype,
                      block_size, mant_bits, epsilon, exp_win, stream, &pg);
}

int bfpq_kv_lens_advance_paged(int32_t* lens, const int32_t* counts, int64_t B, int64_t t, int64_t limit, int64_t cap,
                               const int32_t* page_table, int64_t page_tokens, int64_t pages, void* stream)
{
    BFPQ_PAGES_OR_RETURN(cap);
    return lens_advance(lens, counts, B, t, limit, stream, &pg);
}

int bfpq_kv_bmm_dec_paged(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads,
                          int64_t Tq, int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride,
                          int64_t ldo, int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                          const uint8_t* exp_win, void* ws, int64_t ws_bytes, int64_t chunks_per_split, int64_t cap,
                          const int32_t* page_table, int64_t page_tokens, int64_t pages, void* stream)
{
    BFPQ_PAGES_OR_RETURN(cap);
    return bmm_dec_gqa(x, wcodes, wexp, out, lens, B, heads, Tq, group, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, family, dtype, block_size,
                       x_mant_bits, w_mant_bits, epsilon, exp_win, ws, ws_bytes, chunks_per_split, stream, &pg, cap);
}

int bfpq_kv_attend_paged(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out,
                         void* p_out, const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len,
                         int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                         int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes,
                         void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split, const int32_t* page_table, int64_t page_tokens,
                         int64_t pages, void* stream)
{
    BFPQ_PAGES_OR_RETURN(cap);
    return attend_gqa(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype,
                      block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split,
                      false, nullptr, 0, stream, &pg);
}

int bfpq_kv_attend_rows_paged(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out,
                              void* p_out, const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len,
                              int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                              int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes,
                              void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows,
                              const int32_t* page_table, int64_t page_tokens, int64_t pages, void* stream)
{
    (void)sum_ws; (void)sum_ws_bytes;
    BFPQ_PAGES_OR_RETURN(cap);
    return attend_rows(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal,
                       dtype, block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, chunks_per_split, row0, rows, false,
                       nullptr, 0, stream, &pg);
}
#undef BFPQ_PAGES_OR_RETURN

// ---- the _cb entries: the entry each extends with the window and the paged arguments it lacks and code_bits in front of the
// stream.  A null page_table with page_tokens == 0 and pages == 0 is the contiguous cache; with code_bits == 8 the launch is the one of
// the entry it extends
#define BFPQ_CB_OR_RETURN(cap, mant)                                                                       \
    if (!code_bits_ok(code_bits, block_size, mant)) return BFPQ_E_ARG;                                     \
    const bool paged = page_table || page_tokens != 0 || pages != 0;                                       \
    if (paged && !pages_values_ok(page_tokens, pages, cap)) return BFPQ_E_ARG;                             \
    if (paged && (page_tokens >= kLim || pages >= kLim || (cap) >= kLim)) return BFPQ_E_UNSUPPORTED;       \
    const Pages pg = paged ? pages_arg(page_table, page_tokens, pages, cap) : Pages{};                     \
    const Pages* const pgp = paged ? &pg : nullptr

int bfpq_kv_append_cb(const void* k_new, const void* v_new, void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail,
                      const int32_t* lens, const int32_t* counts, int32_t* overflow, int64_t BH, int64_t heads, int64_t D, int64_t t, int64_t cap,
                      int64_t limit, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon, const uint8_t* exp_win,
                      const int32_t* page_table, int64_t page_tokens, int64_t pages, int code_bits, void* stream)
{
    BFPQ_CB_OR_RETURN(cap, mant_bits);
    return append_dev(k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, lens, counts, overflow, BH, heads, D, t, cap, limit, ldd, dtype,
                      block_size, mant_bits, epsilon, exp_win, stream, pgp, code_bits == 4);
}

int bfpq_kv_bmm_dec_cb(const void* x, const void* wcodes, const int8_t* wexp, void* out, const int32_t* lens, int64_t B, int64_t heads, int64_t Tq,
                       int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo, int family,
                       int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* ws,
                       int64_t ws_bytes, int64_t chunks_per_split, int64_t cap, const int32_t* page_table, int64_t page_tokens, int64_t pages,
                       int code_bits, void* stream)
{
    BFPQ_CB_OR_RETURN(cap, w_mant_bits);
    return bmm_dec_gqa(x, wcodes, wexp, out, lens, B, heads, Tq, group, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, family, dtype, block_size,
                       x_mant_bits, w_mant_bits, epsilon, exp_win, ws, ws_bytes, chunks_per_split, stream, pgp, paged ? cap : 0, code_bits == 4);
}

int bfpq_kv_attend_cb(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out, void* p_out,
                      const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len, int64_t cap,
                      int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits,
                      int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes, void* sum_ws,
                      int64_t sum_ws_bytes, int64_t chunks_per_split, const int32_t* starts, int64_t window, const int32_t* page_table,
                      int64_t page_tokens, int64_t pages, int code_bits, void* stream)
{
    BFPQ_CB_OR_RETURN(cap, w_mant_bits);
    if (!win_values_ok(starts, window)) return BFPQ_E_ARG;
    if (paged && (starts || window != 0)) return BFPQ_E_UNSUPPORTED;   // (a paged cache has no first key)
    return attend_gqa(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype,
                      block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split,
                      true, starts, window, stream, pgp, code_bits == 4);
}

int bfpq_kv_attend_rows_cb(const void* q, const void* k_codes, const int8_t* k_exps, const void* v_codes, const int8_t* v_exps, void* out,
                           void* p_out, const int32_t* lens, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D, int64_t max_len,
                           int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                           int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win, void* score_ws, int64_t score_ws_bytes,
                           void* sum_ws, int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows, const int32_t* starts,
                           int64_t window, const int32_t* page_table, int64_t page_tokens, int64_t pages, int code_bits, void* stream)
{
    (void)sum_ws; (void)sum_ws_bytes;
    BFPQ_CB_OR_RETURN(cap, w_mant_bits);
    if (!win_values_ok(starts, window)) return BFPQ_E_ARG;
    if (paged && (starts || window != 0)) return BFPQ_E_UNSUPPORTED;
    return attend_rows(q, k_codes, k_exps, v_codes, v_exps, out, p_out, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal,
                       dtype, block_size, x_mant_bits, w_mant_bits, epsilon, exp_win, score_ws, score_ws_bytes, chunks_per_split, row0, rows, true,
                       starts, window, stream, pgp, code_bits == 4);
}
#undef BFPQ_CB_OR_RETURN

}  // extern "C"
