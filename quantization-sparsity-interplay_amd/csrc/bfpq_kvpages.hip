// bfpq_kvpages.hip -- the device side of page sharing on a paged HBFP KV cache (bfp_ops.HBFPKVCache.reorder / fork).
//
// A full page of a paged cache is immutable -- key rows are final once appended, token blocks of V once closed, and with
// page_tokens % 64 == 0 every page below a sequence's last one holds closed blocks only -- so any number of table rows may name it and a
// reorder of the sequences (the reference's _reorder_cache, modeling_gpt2.py:1370-1379: index_select(0, beam_idx) of every layer's past)
// is an edit of the table on the host plus, per new row that is not its own source: a copy of at most one page, the open one, into a
// fresh page, and a move of what is private to a sequence, its v_tail rows and its length.  This file is that copy and that move; no
// kernel of bfpq_kvcache.hip changes, they read the table at launch.
//
// A job is five int32: src_row, dst_row, src_page, dst_page, tokens (pages of -1: no page copy).  Two launches, because a reorder may be
// a cycle (rows 0 and 1 each the other's source): k_kv_rows_stage copies the pages and reads every source row into the staging buffer,
// k_kv_rows_place writes the destination rows from there.  The length travels only where lens[src_row] == tokens, the count the host
// planned the pages with; otherwise the destination row is left empty and the sticky overflow word set, so a wrong count never gives a
// row that attends over pages it was not given.  A row or page outside its range makes the job a no-op (and sets overflow): a bad list
// cannot fault.  Copies are 16-byte vector loads and stores, coalesced, no LDS; every piece is a multiple of 16 bytes by 5q's conditions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfpq.h"
#include "bfpq_common.h"

using namespace bfpq;

namespace {

constexpr int64_t kLim = (int64_t)1 << 31;
constexpr int kJobWords = 5;                                  // src_row, dst_row, src_page, dst_page, tokens
constexpr int kPieces = 5;                                    // K codes, K exponents, V codes, V exponents of a page; the row (v_tail, length)
constexpr int kSplitMax = 16;                                 // workgroups a piece is split over at the most
constexpr int64_t kVecPerGroup = 1024;                        // 16-byte vectors a workgroup of 256 moves before another one is worth its launch

struct Job {
    int src_row, dst_row, src_page, dst_page, tokens;
};

struct MoveShape {
    int64_t piece[4];                                         // bytes of a page of k_codes, k_exps, v_codes, v_exps (all kv heads)
    int64_t tail;                                             // bytes of a sequence's v_tail rows
    int B, pages;
};

__device__ __forceinline__ Job job_at(const int32_t* __restrict__ jobs, int j)
{
    const int32_t* w = jobs + (size_t)j * kJobWords;
    return Job{w[0], w[1], w[2], w[3], w[4]};
}

// a job whose rows lie in 0 .. B - 1 and whose pages are both -1 or both in 0 .. pages - 1; any other is a no-op in both launches
__device__ __forceinline__ bool job_ok(const Job& jb, const MoveShape& sh)
{
    const bool rows = jb.src_row >= 0 && jb.src_row < sh.B && jb.dst_row >= 0 && jb.dst_row < sh.B;
    const bool none = jb.src_page == -1 && jb.dst_page == -1;
    const bool both = jb.src_page >= 0 && jb.src_page < sh.pages && jb.dst_page >= 0 && jb.dst_page < sh.pages;
    return rows && (none || both);
}
__device__ __forceinline__ bool job_copies(const Job& jb) { return jb.src_page >= 0; }

// bytes [0, n) from src to dst, n % 16 == 0 and both 16-byte aligned, by the workgroups z < nz of 256 threads: four vectors in flight a thread
// (no __restrict__: a bad list may name one page twice, which must stay harmless)
__device__ __forceinline__ void copy16(const void* src, void* dst, int64_t n, int z, int nz)
{
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    const int64_t nv = n >> 4, step = (int64_t)nz * 256;
    int64_t i = (int64_t)z * 256 + threadIdx.x;
    for (; i + 3 * step < nv; i += 4 * step) {
        const uint4 a = s[i], b = s[i + step], c = s[i + 2 * step], e = s[i + 3 * step];
        d[i] = a; d[i + step] = b; d[i + 2 * step] = c; d[i + 3 * step] = e;
    }
    for (; i < nv; i += step) d[i] = s[i];
}

// the tails, then the lengths
__device__ __forceinline__ int64_t stage_lens_at(int64_t n_jobs, int64_t tail) { return n_jobs * tail; }

// launch A.  grid (jobs, pieces, split): pieces 0 .. 3 copy the job's page, piece 4 stages the source row
__global__ void __launch_bounds__(256) k_kv_rows_stage(int8_t* k_codes, int8_t* k_exps, int8_t* v_codes, int8_t* v_exps, const void* v_tail,
                                                        const int32_t* lens, int32_t* overflow, const int32_t* __restrict__ jobs, int n_jobs,
                                                        void* stage, MoveShape sh)
{
    const int j = blockIdx.x, piece = blockIdx.y, z = blockIdx.z, nz = gridDim.z;
    const Job jb = job_at(jobs, j);
    if (!job_ok(jb, sh)) {
        if (piece == kPieces - 1 && z == 0 && threadIdx.x == 0) overflow[0] = 1;
        return;
    }
    if (piece < kPieces - 1) {
        if (!job_copies(jb)) return;
        int8_t* pool = piece == 0 ? k_codes : piece == 1 ? k_exps : piece == 2 ? v_codes : v_exps;
        const int64_t n = sh.piece[piece];
        copy16(pool + (size_t)jb.src_page * n, pool + (size_t)jb.dst_page * n, n, z, nz);
        return;
    }
    copy16((const char*)v_tail + (size_t)jb.src_row * sh.tail, (char*)stage + (size_t)j * sh.tail, sh.tail, z, nz);
    if (z == 0 && threadIdx.x == 0) {
        const int len = lens[jb.src_row];
        const bool agree = jb.tokens >= 0 && len == jb.tokens;    // the count the host planned the pages with
        reinterpret_cast<int32_t*>((char*)stage + stage_lens_at(n_jobs, sh.tail))[j] = agree ? len : 0;
        if (!agree) overflow[0] = 1;
    }
}

// launch B.  grid (jobs, split): the staged row becomes the destination row
__global__ void __launch_bounds__(256) k_kv_rows_place(void* v_tail, int32_t* lens, const int32_t* __restrict__ jobs, int n_jobs,
                                                        const void* stage, MoveShape sh)
{
    const int j = blockIdx.x, z = blockIdx.y, nz = gridDim.y;
    const Job jb = job_at(jobs, j);
    if (!job_ok(jb, sh)) return;
    copy16((const char*)stage + (size_t)j * sh.tail, (char*)v_tail + (size_t)jb.dst_row * sh.tail, sh.tail, z, nz);
    if (z == 0 && threadIdx.x == 0) lens[jb.dst_row] = reinterpret_cast<const int32_t*>((const char*)stage + stage_lens_at(n_jobs, sh.tail))[j];
}

inline int64_t elem_bytes(int dtype) { return dtype == BFPQ_F32 ? 4 : 2; }
inline bool block_ok(int block_size) { return block_size == 16 || block_size == 32 || block_size == 64; }
inline int64_t tail_bytes(int64_t kv_heads, int64_t D, int block_size, int dtype) { return kv_heads * block_size * D * elem_bytes(dtype); }
inline int split_of(int64_t bytes)
{
    const int64_t n = ((bytes >> 4) + kVecPerGroup - 1) / kVecPerGroup;
    return (int)(n < 1 ? 1 : (n > kSplitMax ? kSplitMax : n));
}

}  // namespace

extern "C" {

int64_t bfpq_kv_rows_move_ws_bytes(int64_t n_jobs, int64_t kv_heads, int64_t D, int block_size, int dtype)
{
    if (!dtype_ok(dtype) || !block_ok(block_size) || n_jobs < 0 || kv_heads < 1 || D < 0) return BFPQ_E_ARG;
    if (D % 16 != 0 || D > 1024 || n_jobs >= kLim || kv_heads >= kLim) return BFPQ_E_UNSUPPORTED;
    return n_jobs * tail_bytes(kv_heads, D, block_size, dtype) + (n_jobs * 4 + 15) / 16 * 16;   // the v_tail rows, then the lengths
}

// bfpq_kv_rows_move (code_bits 8) and bfpq_kv_rows_move_cb: with 4-bit codes a page of k_codes and of v_codes is half the bytes
static int rows_move(void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail, int32_t* lens, int32_t* overflow,
                     const int32_t* jobs_dev, int64_t n_jobs, void* stage_dev, int64_t stage_bytes, int64_t B, int64_t kv_heads, int64_t D,
                     int block_size, int dtype, int64_t page_tokens, int64_t pages, int code_bits, void* stream)
{
    if (code_bits != 8 && !(code_bits == 4 && block_size == 64)) return BFPQ_E_ARG;
    if (!dtype_ok(dtype) || !block_ok(block_size) || n_jobs < 0 || B < 1 || kv_heads < 1 || page_tokens < 64 || page_tokens % 64 != 0 ||
        pages < 1)
        return BFPQ_E_ARG;
    const int64_t ldd = (D + 63) / 64 * 64;
    if (!bfpq_kv_ok(D, page_tokens, block_size) || n_jobs >= kLim || B >= kLim || pages >= kLim || kv_heads >= kLim ||
        page_tokens * ldd >= kLim || pages * kv_heads >= kLim)
        return BFPQ_E_UNSUPPORTED;
    if (n_jobs == 0) return 0;
    if (!k_codes || !k_exps || !v_codes || !v_exps || !v_tail || !lens || !overflow || !jobs_dev || !stage_dev ||
        !aligned16(k_codes, k_exps, v_codes, v_exps, v_tail, stage_dev) ||
        ((reinterpret_cast<uintptr_t>(lens) | reinterpret_cast<uintptr_t>(overflow) | reinterpret_cast<uintptr_t>(jobs_dev)) & 3u))
        return BFPQ_E_ARG;
    const int64_t need = bfpq_kv_rows_move_ws_bytes(n_jobs, kv_heads, D, block_size, dtype);
    if (need < 0 || stage_bytes < need) return BFPQ_E_ARG;
    MoveShape sh;
    sh.piece[0] = kv_heads * page_tokens * ldd * code_bits / 8;   // (page_tokens % 64 == ldd % 64 == 0: halves are multiples of 16 too)
    sh.piece[1] = kv_heads * page_tokens * (D / block_size);
    sh.piece[2] = kv_heads * D * page_tokens * code_bits / 8;
    sh.piece[3] = kv_heads * D * (page_tokens / block_size);
    sh.tail = tail_bytes(kv_heads, D, block_size, dtype);
    sh.B = (int)B;
    sh.pages = (int)pages;
    int64_t most = sh.tail;
    for (int i = 0; i < 4; i++) most = sh.piece[i] > most ? sh.piece[i] : most;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_kv_rows_stage, dim3((unsigned)n_jobs, kPieces, (unsigned)split_of(most)), dim3(256), 0, s, (int8_t*)k_codes, k_exps,
                       (int8_t*)v_codes, v_exps, (const void*)v_tail, (const int32_t*)lens, overflow, jobs_dev, (int)n_jobs, stage_dev, sh);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_kv_rows_place, dim3((unsigned)n_jobs, (unsigned)split_of(sh.tail)), dim3(256), 0, s, v_tail, lens, jobs_dev, (int)n_jobs,
                       (const void*)stage_dev, sh);
    return (int)hipGetLastError();
}

int bfpq_kv_rows_move(void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail, int32_t* lens, int32_t* overflow,
                      const int32_t* jobs_dev, int64_t n_jobs, void* stage_dev, int64_t stage_bytes, int64_t B, int64_t kv_heads, int64_t D,
                      int block_size, int dtype, int64_t page_tokens, int64_t pages, void* stream)
{
    return rows_move(k_codes, k_exps, v_codes, v_exps, v_tail, lens, overflow, jobs_dev, n_jobs, stage_dev, stage_bytes, B, kv_heads, D, block_size,
                     dtype, page_tokens, pages, 8, stream);
}

int bfpq_kv_rows_move_cb(void* k_codes, int8_t* k_exps, void* v_codes, int8_t* v_exps, void* v_tail, int32_t* lens, int32_t* overflow,
                         const int32_t* jobs_dev, int64_t n_jobs, void* stage_dev, int64_t stage_bytes, int64_t B, int64_t kv_heads, int64_t D,
                         int block_size, int dtype, int64_t page_tokens, int64_t pages, int code_bits, void* stream)
{
    return rows_move(k_codes, k_exps, v_codes, v_exps, v_tail, lens, overflow, jobs_dev, n_jobs, stage_dev, stage_bytes, B, kv_heads, D, block_size,
                     dtype, page_tokens, pages, code_bits, stream);
}

}  // extern "C"
