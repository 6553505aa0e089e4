/*
 * bfpq.h -- C ABI of libbfpq.so, the MI355X (gfx950) BFP quantize + sparsify engine.
 *
 * This is the drop-in boundary for the reference's hot path
 *     src/transformers/bfp/bfp_ops.py:16-149   (get_exponent, _convert_blocked_float_to_bfp,
 *     _no_sparsity_float_to_bfp, _structured_N_M_sparsity, _unstructured_sparsity, _sparsify,
 *     _quantize, float_to_bfp_blocked)
 * The reference has no native code on this path (it is ~25 ATen passes per call); these entry
 * points are what a ctypes / pybind binding placed in that file would call instead.
 *
 * Conventions
 *   - every pointer named *_dev is a DEVICE pointer owned by the caller; *_host is host memory
 *   - tensors are dense row-major [rows, cols]; blocks and N:M groups run along cols only and
 *     never cross a row (bfp_ops.py:50-59, :79-91); leading dims are flattened into rows
 *   - dtype: BFPQ_F32 / BFPQ_F16 / BFPQ_BF16 (input and dequantised output share the dtype)
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*); nothing here
 *     synchronises, allocates or frees device memory, so every call is hipGraph-capturable
 *   - return value: 0 on success, a negative BFPQ_E_* for argument errors, a positive
 *     hipError_t if a launch failed
 *   - rounding is round-half-to-even ('determ', bfp_ops.py:24-25) unless a stochastic seed is given
 */
#ifndef BFPQ_H
#define BFPQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFPQ_VERSION 4

enum { BFPQ_F32 = 0, BFPQ_F16 = 1, BFPQ_BF16 = 2 };

enum {
    BFPQ_E_ARG = -1,        /* bad shape / pointer / enum                                        */
    BFPQ_E_UNSUPPORTED = -2,/* valid in the reference but not handled by this entry point        */
    BFPQ_E_ALIGN = -3       /* a fast-path entry point was given a misaligned pointer            */
};

/* sizes of the small constant tables the kernels read (built on the host, uploaded by the caller
 * once per device; keeping them caller-owned keeps the library stateless -- but for the pointer pairs of bfpq_nm4_lut_bind) */
#define BFPQ_EXP_WIN_ENTRIES 320   /* uint8 per unbiased exponent k in [-160, 160)              */
#define BFPQ_NM4_LUT_ENTRIES 729   /* uint8 keep-mask per 3^6 pairwise-comparison signature     */
#define BFPQ_NM8_LUT_ENTRIES (1 << 24) /* uint8 prune-mask per (number of smaller keys)^8 vector, 3 bits each */

int bfpq_version(void);
/* process-wide tuning knobs (measurement aid; defaults are the measured optimum on MI355X) */
#define BFPQ_TUNE_MAX_GRID 0       /* cap on workgroups of the streaming kernels (default 1024) */
#define BFPQ_TUNE_GEMM_ROW_TILES 1 /* 16-row tiles per wave in bfpq_hbfp_linear_decode_tiled: 0 = choose (default), 1, 2, 4 */
#define BFPQ_TUNE_LIST_OWN_MB 3    /* list calls: tensors from this many MB on get launches of their own (default 24; 0 = all, a huge value = none) */
#define BFPQ_TUNE_MX8_VARIANT 2    /* tile shape of bfpq_hbfp_linear_mx8: -1 = choose (default), 0..6 force (A/B measurements) */
#define BFPQ_TUNE_I8_VARIANT 4     /* tile shape of bfpq_hbfp_linear_i8 / _splitk: -1 = choose (default), 0..2 force */
#define BFPQ_TUNE_I8_PARTS 5       /* K parts bfpq_hbfp_linear_i8_parts returns: 0 = choose (default), 1..64 force (capped at K / 256) */
int bfpq_tune(int key, int value);
const char* bfpq_error_string(int code);

/* ---- host-side table builders ---------------------------------------------------------------
 * bfpq_exp_window_host: replaces the dtype-dependent rounding inside get_exponent
 * (bfp_ops.py:29-33): for s = 2^k (1+f) the reference's ceil(log2(s)) evaluated in `dtype` is k
 * when the dtype mantissa field of s is <= table[k + 160], else k + 1.
 * bfpq_nm4_lut_host: keep-mask (bit i set = element i kept) of one group of 4 for "keep N of 4",
 * indexed by sum_{p} c_p 3^p over pairs p = (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) with
 * c = 0/1/2 for |a_i| <,==,> |a_j|; reproduces ATen CPU topk's std::nth_element tie order
 * used by _structured_N_M_sparsity (bfp_ops.py:85). */
int bfpq_exp_window_host(int dtype, uint8_t* table_host /* [BFPQ_EXP_WIN_ENTRIES] */);
int bfpq_nm4_lut_host(int N, uint8_t* lut_host /* [BFPQ_NM4_LUT_ENTRIES] */);
/* bfpq_nm4_masks_host: the same table expanded for the 16-bit dtypes -- per signature the two AND masks (elements 0,1 | 2,3 as
 * 0xffff halves) of a group of 4, padded with keep-everything entries to BFPQ_NM4_MASK_BYTES.  Optional: a caller that uploads it
 * (16-byte aligned) and names it with bfpq_nm4_lut_bind(lut_dev, masks_dev) spares the packed-output kernels the expansion of the byte
 * table in every workgroup; a LUT pointer that was never bound works as before.  Both device buffers stay the caller's and must
 * outlive the binding (masks_dev == NULL removes it); at most BFPQ_NM4_BIND_MAX bindings, BFPQ_E_ARG beyond. */
#define BFPQ_NM4_MASK_BYTES 5888   /* 736 x 2 x uint32 */
#define BFPQ_NM4_BIND_MAX 64
int bfpq_nm4_masks_host(int N, uint32_t* masks_host /* [BFPQ_NM4_MASK_BYTES / 4] */);
int bfpq_nm4_lut_bind(const uint8_t* nm4_lut_dev, const void* masks_dev);
/* bfpq_nm8_lut_host: PRUNE mask (bit i set = element i zeroed) of one group of 8 for "keep N of 8", indexed by
 * sum_i less_i << (3 i) with less_i = number of keys strictly smaller than key i (this vector identifies the weak
 * ordering of the group, which is all std::nth_element's behaviour depends on).  16 MiB, optional: pass it as nm4_lut_dev
 * when M == 8; with NULL the kernel replays nth_element for the groups whose ties straddle the cut (slower, same result). */
int bfpq_nm8_lut_host(int N, uint8_t* lut_host /* [BFPQ_NM8_LUT_ENTRIES] */);
/* host restatement of the N:M selection for one group (any 1 <= N <= M <= 64); keys are
 * non-negative magnitudes compared as unsigned integers. Returns the 64-bit PRUNE mask. Used by the
 * host-logic tests and to build the LUT above. */
uint64_t bfpq_nm_prune_mask_host(const uint32_t* keys, int N, int M);

/* ---- fused quantize (+ N:M) -----------------------------------------------------------------
 * Replaces float_to_bfp_blocked (bfp_ops.py:124-149) for sparsity_mode 'structured' or no
 * sparsity, sparsity_num_format 'bfp' or 'fp32':
 *     sparsify_first != 0:  out = Q(S(in))   (first == 's')
 *     sparsify_first == 0:  out = S(Q(in))
 * with Q = _no_sparsity_float_to_bfp (block_size, mant_bits; block_size == 0 -> identity, the
 * 'fp32' format) and S = _structured_N_M_sparsity (N, M; M == 0 -> identity).
 * Outputs (each nullable, at least one required):
 *   out_deq_dev   [rows, cols] dtype          the reference's fake-quantised tensor (drop-in mode)
 *   out_codes_dev sign-magnitude mantissas as two's-complement integers, code_bits wide
 *                 (4: two per byte, low nibble first, [rows, ceil(cols/2)] bytes; 8: int8; 16: int16;
 *                 32: not codes but the fp32 image of the dequantised tensor, [rows, cols] float -- what the
 *                 reference returns for 'stoc' rounding of a half tensor; single-pass kernel only)
 *   out_exp_dev   int8 [rows, ceil(cols/block)] shared exponent e (value = code * 2^(e-mant_bits));
 *                 saturated to [-127, 127]; -128 marks a block the reference turns into NaN
 * Any shape, block size and 1 <= N <= M <= 64 is accepted; the single-pass fused kernel is used
 * when cols % block == 0, block is 16 bytes x a power of two <= 64 lanes, and M in {0, 2, 4} (or 8 on a
 * 16-bit dtype) divides the block; otherwise the work is split into a sparsify and a quantize launch through
 * scratch_dev (rows*cols elements of dtype, may be NULL when the fused kernel applies).
 * stoch_seed == 0 -> round-half-even; otherwise stochastic rounding (uniform dither in
 * [-0.5, 0.5) from a counter-based generator keyed by (seed, element index), bfp_ops.py:21-23). */
int bfpq_quantize_nm(const void* in_dev, void* out_deq_dev, void* out_codes_dev, int8_t* out_exp_dev,
                     int64_t rows, int64_t cols, int dtype,
                     int block_size, int mant_bits, double epsilon,
                     int N, int M, int sparsify_first,
                     int code_bits, uint64_t stoch_seed,
                     const uint8_t* exp_win_dev, const uint8_t* nm4_lut_dev,
                     void* scratch_dev, void* stream);

/* The drop-in call with its constants bound once (what a module's forward issues per tensor): the same work as
 * bfpq_quantize_nm(in, out, NULL, NULL, rows, cols, plan->...) in round-half-even mode, six arguments instead of nineteen.
 * Shapes that need the two-launch general path work in place through out_dev (no scratch). */
typedef struct bfpq_plan {
    int dtype, block_size, mant_bits, N, M, sparsify_first;
    double epsilon;
    const uint8_t* exp_win_dev;   /* BFPQ_EXP_WIN_ENTRIES, for dtype (NULL when block_size == 0) */
    const uint8_t* nm_lut_dev;    /* bfpq_nm4_lut_host(N) for M == 4, bfpq_nm8_lut_host(N) or NULL for M == 8, else NULL */
} bfpq_plan;
int bfpq_fake_quantize(const bfpq_plan* plan_host, const void* in_dev, void* out_dev, int64_t rows, int64_t cols, void* stream);

/* A LIST of tensors in as few launches as possible (up to 64 tensors per launch, their descriptors travel as kernel
 * arguments: no device memory, graph-capturable).  All tensors share the plan (dtype, block, mantissa width, N:M); apply_nm
 * says per tensor whether the plan's N:M pruning applies (a Linear's weight) or not (its activation).  What a model pass
 * issues for "all Linear weights", and what one BFPLinear forward issues for its activation + weight.  Tensors whose
 * shape the single-pass kernel does not take (ragged rows, M = 8, ...) are handled one by one inside the call. */
typedef struct bfpq_tensor_desc { const void* in_dev; void* out_dev; int64_t rows, cols; int apply_nm; int reserved; } bfpq_tensor_desc;
int bfpq_fake_quantize_batched(const bfpq_plan* plan_host, const bfpq_tensor_desc* descs_host, int n, void* stream);
/* The same list over several LANES (ABI 4): the caller's stream and up to 7 aux streams.  Inside either call a tensor of 24 MB or more
 * gets a launch of its own (the list kernel only pays where a launch of its own would be mostly ramp and tail); with aux streams those
 * launches are spread over the lanes -- each to the lane that has been given the fewest bytes so far -- so that the tail of one
 * tensor's launch runs beside the ramp of another's (64 x [4096,11008] bf16 2:4 -> HBFP4, us per tensor: one aux stream 29.5-30.2,
 * none 31.9-33.4, the list kernel 35.7-37.0; LLaMA-7B's 224 weights 4.07 ms against 5.31; more than one aux stream buys nothing here).
 * The aux lanes wait for what `stream` held at the call and `stream` waits for them before the call returns (one fork, one join, no
 * event between the lanes: hipGraph-capturable from `stream`).  A list with fewer than two such tensors stays on `stream` (a Linear's
 * weight next to its activation: the fork and join would cost more than they gain).  The tensors of one list must not overlap one
 * another (they are processed side by side).  bfpq_fake_quantize_batched(...) is bfpq_fake_quantize_list(..., stream, NULL, 0). */
int bfpq_fake_quantize_list(const bfpq_plan* plan_host, const bfpq_tensor_desc* descs_host, int n, void* stream,
                            void* const* aux_streams_host, int n_aux);

/* returns 1 if bfpq_quantize_nm would take the single-pass fused kernel for this problem */
int bfpq_is_fused(int64_t rows, int64_t cols, int dtype, int block_size, int N, int M);

/* ---- N:M only (replaces _structured_N_M_sparsity, bfp_ops.py:73-91) --------------------------- */
int bfpq_nm_sparsify(const void* in_dev, void* out_dev, int64_t rows, int64_t cols, int dtype,
                     int N, int M, const uint8_t* nm4_lut_dev, void* stream);

/* ---- unstructured magnitude pruning (replaces _unstructured_sparsity, bfp_ops.py:61-71) -------
 * Exact global k-th smallest |v| by radix select on the magnitude bit pattern, then "zero everything below the
 * threshold tau and the first `need` (flat index order, lower ranks first) of the elements equal to it".
 *
 * Single device, TWO launches for a 16-bit dtype:
 *   1. bfpq_select(...)            one launch: per-segment histograms, and the LAST workgroup to finish (an atomic ticket, no
 *                                  workgroup ever waits for another) resolves threshold + tie bookkeeping into ws_dev.
 *                                  fp32: two such launches (the high 15 bits of the key, then the low 16 bits of the keys that
 *                                  share them): the tensor is read three times in all, the launch-pair form reads it four times.
 *   2. bfpq_threshold_apply(...) or bfpq_quantize_threshold(...)   prune (and quantize) in one pass
 * ws_dev must be ZERO before its first use; every call leaves it ready for the next one.
 *
 * Multi-GPU (row slabs, one global threshold): for pass p in [0, bfpq_select_passes(dtype)):
 *     bfpq_select_hist(...)      histogram of the current digit of this device's elements into a caller-owned hist_dev
 *                                (BFPQ_SELECT_HIST_COPIES x BFPQ_SELECT_HIST_ENTRIES uint32, zero on entry); on the last pass also
 *                                per-segment windows of it -> ws_dev
 *     ALL-GATHER the per-rank buffers into hist_all_dev [n_ranks][BFPQ_SELECT_HIST_COPIES][BFPQ_SELECT_HIST_ENTRIES] -- the one
 *                                exchange of the path: the per-rank counts of the threshold bin also tell every rank how many
 *                                ties lower ranks hold
 *     bfpq_select_resolve(...)   picks the digit (pass 0 starts the selection with k); on the last pass leaves tau, need, ties
 *                                and the tie bookkeeping of this device's slab in ws_dev; clears the local histogram for its
 *                                next use (zero_hist_dev = hist_dev)
 *   then the apply launch as above.  (hist_dev = NULL / hist_all_dev = NULL run the same launches on histogram buffers inside
 *   ws_dev; fp32 takes three pairs, 11 + 11 + 9 bits.)
 * ws_dev: BFPQ_SELECT_WS_BYTES bytes, zeroed once, 16-byte aligned; it begins with a bfpq_select_state.
 * k is the GLOBAL prune count int(numel_global * frac) (bfp_ops.py:66); numel_global < 2^32.
 * in_dev and out_dev of the apply launch must not alias (the tie ranks are counted from the input while other tiles are written).
 * Tie positions: the reference's are those of a sequential introselect over the whole tensor and
 * are not reproduced; threshold, count and every element outside the tie class are.
 * How ties are ranked without a rank per tile: csrc/bfpq_device.h, block comment at "Unstructured pruning". */
#define BFPQ_SELECT_STATE_BYTES 80
#define BFPQ_SELECT_MAX_SEGMENTS 256
#define BFPQ_SELECT_WINDOW_BINS 2048
#define BFPQ_SELECT_HIST_ENTRIES (32768 + 256)   /* fine bins, then (16-bit dtypes) 256 coarse bins of 128 */
#define BFPQ_SELECT_HIST_COPIES 8                /* a device accumulates into 8 copies (cuts the contention of the flush) */
#define BFPQ_SELECT_WS_BYTES (BFPQ_SELECT_STATE_BYTES + 4 * (12 + BFPQ_SELECT_HIST_COPIES * 512 + 3 * BFPQ_SELECT_HIST_COPIES * BFPQ_SELECT_HIST_ENTRIES + \
                              3 * BFPQ_SELECT_MAX_SEGMENTS + 2 * BFPQ_SELECT_MAX_SEGMENTS * BFPQ_SELECT_WINDOW_BINS))

int bfpq_select_passes(int dtype);
int64_t bfpq_select_ws_bytes(void);
/* single device: every launch of the selection (16-bit dtypes: ONE, fp32: TWO) */
int bfpq_select(const void* in_dev, int64_t numel, int dtype, int64_t k, void* ws_dev, void* stream);
int bfpq_select_hist(const void* in_dev, int64_t numel, int dtype, int pass, int64_t k, int64_t numel_global,
                     void* ws_dev, uint32_t* hist_dev, void* stream);
int bfpq_select_resolve(const void* in_dev, int64_t numel, int dtype, int pass, int64_t k,
                        const uint32_t* hist_all_dev /* [n_ranks][COPIES][ENTRIES] */, int n_ranks, int rank,
                        void* ws_dev, uint32_t* zero_hist_dev, void* stream);
/* The same resolve launch over a gathered block of another shape (ABI 4): per rank `copies` histograms (1 ... BFPQ_SELECT_HIST_COPIES) of
 * BFPQ_SELECT_HIST_ENTRIES words, rank r's set at hist_all_dev + r * rank_stride_words.  What a LIST of row-sharded tensors uses to get by with ONE
 * exchange per radix pass for the whole list instead of one per tensor: every tensor's local histogram is launched first, the copies of each are
 * summed (a tensor then sends 132 KB instead of 1 MB), the [tensors, ENTRIES] block is all-gathered in one collective, and tensor i resolves
 * from hist_all_dev = gathered + i * ENTRIES with copies = 1, rank_stride_words = tensors * ENTRIES.  zero_hist_dev as above: the tensor's
 * local 8-copy buffer, cleared for its next use.  bfpq_select_resolve(...) is the call with copies = 8, rank_stride_words = 8 * ENTRIES. */
int bfpq_select_resolve_ex(const void* in_dev, int64_t numel, int dtype, int pass, int64_t k,
                           const uint32_t* hist_all_dev, int n_ranks, int rank, int copies, int64_t rank_stride_words,
                           void* ws_dev, uint32_t* zero_hist_dev, void* stream);
int bfpq_select_reset(void* ws_dev, void* stream);
int bfpq_threshold_apply(const void* in_dev, void* out_dev, int64_t numel, int dtype, void* ws_dev, void* stream);
/* step 3 fused with the quantizer: out = Q(S_threshold(in)) in one pass over the tensor (first == 's',
 * bfp_ops.py:141-144 with sparsity_mode 'unstructured'); same outputs / tables / fallbacks as
 * bfpq_quantize_nm (scratch_dev only when the shape needs the two-launch path and out_deq_dev is NULL).  Not in place: in_dev == out_deq_dev
 * or in_dev == out_codes_dev returns BFPQ_E_ARG before any launch (the workgroups of the cut re-read in_dev to rank the ties while
 * other workgroups write their pruned tiles), as bfpq_threshold_apply and bfpq_prune_quantize refuse in == out. */
int bfpq_quantize_threshold(const void* in_dev, void* out_deq_dev, void* out_codes_dev, int8_t* out_exp_dev,
                            int64_t rows, int64_t cols, int dtype, int block_size, int mant_bits, double epsilon,
                            int code_bits, uint64_t stoch_seed, const uint8_t* exp_win_dev,
                            void* ws_dev, void* scratch_dev, void* stream);

/* The whole s-first unstructured drop-in op, out = Q(S_unstructured(in)) with k = int(numel * frac) elements pruned
 * (float_to_bfp_blocked with sparsity_mode 'unstructured', first 's': bfp_ops.py:61-71, :141-144), single device, round-half-even:
 * bfpq_select + bfpq_quantize_threshold behind one call (two launches for a 16-bit dtype; the tensor is read by both). */
int bfpq_prune_quantize(const void* in_dev, void* out_dev, int64_t rows, int64_t cols, int dtype, int block_size, int mant_bits,
                        double epsilon, int64_t k, const uint8_t* exp_win_dev, void* ws_dev, void* stream);
/* The same op for a LIST of tensors -- every Linear weight of a model (BASELINE config 4) -- over independent LANES (ABI 4): the
 * caller's stream and up to 7 aux streams, a workspace per lane (ws_devs: n_ws distinct caller-owned workspaces, BFPQ_SELECT_WS_BYTES
 * each, zeroed once; lanes used = min(1 + n_aux, n_ws)).  A tensor's two launches go back to back to the lane that has been given the
 * fewest bytes so far; nothing orders the lanes against one another, so a lane's serial tail (publishing, the ticket, the resolve
 * step, the kernel boundary: ~13 us in which that lane moves no data) is covered by the other lanes' streaming.  LLaMA-13B, all 280
 * weights, bf16: one lane 16.8 ms, two 14.2, three 12.7, four 12.5.  The aux lanes wait for what `stream` held at the call and
 * `stream` waits for them before the call returns (one fork, one join: hipGraph-capturable from `stream`).  The tensors of one list
 * must not overlap one another.  Creates and destroys a handful of hipEvents per call; launches only, no synchronisation.
 * bfpq_prune_quantize_batched (ABI 3) is the same call with at most one aux stream. */
typedef struct bfpq_prune_desc { const void* in_dev; void* out_dev; int64_t rows, cols; int64_t k; } bfpq_prune_desc;
int bfpq_prune_quantize_list(const bfpq_prune_desc* descs_host, int n, int dtype, int block_size, int mant_bits, double epsilon,
                             const uint8_t* exp_win_dev, void* const* ws_devs_host, int n_ws, void* stream,
                             void* const* aux_streams_host, int n_aux);
int bfpq_prune_quantize_batched(const bfpq_prune_desc* descs_host, int n, int dtype, int block_size, int mant_bits, double epsilon,
                                const uint8_t* exp_win_dev, void* const* ws_devs_host, int n_ws, void* stream, void* aux_stream);

/* ---- 'int' per-channel format (replaces _quantize's 'int' branch, bfp_ops.py:111-120, i.e.
 * int_ops.Quantizer.configure/find_params/quantize with the defaults perchannel=True, sym=True) -------
 * The tensor is viewed as [outer, C, inner] with the channel in the middle (int_ops.py:38-50):
 * weight: outer = 1, C = shape[0], inner = rest; 2-D/3-D activation: outer = rows, C = last dim,
 * inner = 1; 4-D activation: outer = N, C = shape[1], inner = H*W.  maxq = 2^bits - 1.
 * out_dev is fp32 for every input dtype (as in the reference).  ws_dev: bfpq_int_workspace_elems(C)
 * uint32, needed (any content) unless outer == 1. */
int64_t bfpq_int_workspace_elems(int64_t C);
int bfpq_int_quantize(const void* in_dev, float* out_dev, int64_t outer, int64_t C, int64_t inner, int dtype, int bits,
                      uint32_t* ws_dev, void* stream);

/* ---- packed HBFP -> tensor (no counterpart in the reference, which never stores quantized tensors;
 * SURVEY §8f next #3): out = code * 2^(exp - mant_bits) in dtype, from the codes / exponents that
 * bfpq_quantize_nm / bfpq_quantize_threshold write.  Equals their out_deq except that a negative zero
 * comes back as +0 (a two's-complement code has no -0) and saturated exponents (|e| > 127) are lost. */
int bfpq_dequantize(const void* codes_dev, const int8_t* exp_dev, void* out_dev, int64_t rows, int64_t cols, int dtype,
                    int block_size, int mant_bits, int code_bits, void* stream);

/* ---- 'stoc' rounding of an fp16 tensor, fp16 result -> the reference's fp32 result (n elements): a plain widening,
 * except that +-inf becomes +-65536 -- the one fp32 result of a finite fp16 input that fp16 cannot hold (a block whose
 * 2^e overflows).  in_dev 8-byte aligned, out_dev 16-byte aligned. */
int bfpq_stoc_widen_f16(const void* in_dev, void* out_dev, int64_t n, void* stream);

/* ---- 2:4 compaction of 4-bit codes (optional part of the packed format) --------------------
 * codes_dev: n_bytes bytes of 4-bit codes as bfpq_quantize_nm writes them (n_bytes % 4 == 0; 8 elements per 4 bytes),
 * every aligned group of 4 codes holding at most 2 non-zeros (N=2, M=4 in either order guarantees it).
 * vals_dev: n_bytes / 2 bytes (per group one byte: the two kept codes, lower position in the low nibble);
 * idx_dev: n_bytes / 4 bytes (per group 4 bits: the two positions).  0.375 B per element instead of 0.5.
 * status_dev[0] (int32, zeroed by the caller) is set to 1 if some group had more than 2 non-zero codes.
 * bfpq_expand24 is the exact inverse. */
int bfpq_compact24(const void* codes_dev, void* vals_dev, void* idx_dev, int64_t n_bytes, int32_t* status_dev, void* stream);
int bfpq_expand24(const void* vals_dev, const void* idx_dev, void* codes_dev, int64_t n_bytes, void* stream);

/* ---- packed-format consumer for decode (no reference counterpart: it runs F.linear on fake-quantised tensors,
 * bfp_ops.py:187-190): out[t][n] = sum_k x[t][k] W[n][k], T <= 16 tokens, W packed HBFP
 * (4-bit codes, mant_bits <= 3) and x packed HBFP (int8 codes, mant_bits <= 7), both block 64, exact integer
 * block sums on the int8 matrix cores, fp32 across blocks.  N % 16 == 0, K % 256 == 0.
 * NaN blocks propagate: a block whose exponent byte is -128 (the NaN block marker bfpq_quantize_nm writes), in x or in W,
 * makes every output it contributes to NaN, as the reference's product of the fake-quantised tensors does.
 *   xcodes_dev [16, K] int8 and xexp_dev [16, K/64] (rows >= T: any content, their results are discarded),
 *   slabs_dev [bfpq_hbfp_linear_slices(N, K), 16, N] fp32 scratch, out_dev [T, N] of out_dtype. */
int bfpq_hbfp_linear_slices(int64_t N, int64_t K);
int bfpq_hbfp_linear_decode(const void* wcodes_dev, const int8_t* wexp_dev, const int8_t* xcodes_dev, const int8_t* xexp_dev,
                            void* out_dev, float* slabs_dev, int64_t T, int64_t N, int64_t K,
                            int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);

/* the same product from the MFMA-tiled weight layout (a one-time repack of the packed weight; K % 128 == 0, K >= 256):
 *   wtiles_dev [N/16][K/128][64][16] bytes: lane l = r + 16 q of the pair p holds the 16 codes k = 16q..16q+15 of row
 *               16*rt + r for block 2p (bytes 0-7) and block 2p+1 (bytes 8-15)
 *   wexpt_dev  [N/16][K/128][16][2] int8: exponents of the pair's two blocks per row
 * Up to 64 tokens per call here (groups of 16 tokens walk the weight one after the other inside the one launch; xcodes_dev /
 * xexp_dev then hold T rows).
 * One launch, no workspace: each workgroup owns one or two 16-row tiles, its waves split K and are summed in slice order
 * through LDS, so the result is reproducible.  NaN blocks propagate as in bfpq_hbfp_linear_decode. */
int bfpq_hbfp_linear_tiled_ok(int64_t N, int64_t K);   /* 1 when the tiled layout applies to [N, K] */
int bfpq_hbfp_linear_decode_tiled(const void* wtiles_dev, const void* wexpt_dev, const int8_t* xcodes_dev, const int8_t* xexp_dev,
                                  void* out_dev, int64_t T, int64_t N, int64_t K,
                                  int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);

/* ---- packed-format consumer for prefill (replaces F.linear on the two fake-quantised operands,
 * bfp_ops.py:187-190): out[T, N] = x[T, K] W[N, K]^T (+ bias[N]) for any T, both operands HBFP with block 64 and mantissas that
 * fit e4m3 exactly (mant_bits <= 4), on CDNA4's block-scaled matrix instruction (one v_mfma_scale_f32_32x32x64_f8f6f4 = the
 * exact integer dot product of one HBFP block times the two power-of-two block scales, fp32 across blocks).
 * Operand images ("mx8"): e4m3 bytes [rows, K] + E8M0 scale bytes [rows, K/64], made by bfpq_mx8_from_hbfp from the codes
 * (code_bits 4: two's-complement nibbles, or 8: int8) and int8 exponents that bfpq_quantize_nm writes (exponent -128, the NaN
 * block marker, becomes the E8M0 NaN).  K % 256 == 0; x8 / w8 16-byte aligned, the scale arrays 4-byte aligned;
 * bias (nullable) and out of out_dtype. */
int bfpq_mx8_from_hbfp(const void* codes_dev, const int8_t* exp_dev, void* out8_dev, void* out_scale_dev, int64_t rows, int64_t cols,
                       int code_bits, int mant_bits, void* stream);
/* a tensor straight to its mx8 image (dense HBFP quantize, block 64, round-half-even: the activation operand of a
 * prefill; one pass, sizeof(dtype) B read + 1.016 B written per element).  cols % 64 != 0 / unaligned pointers: BFPQ_E_UNSUPPORTED
 * (take bfpq_quantize_nm with int8 codes + bfpq_mx8_from_hbfp). */
int bfpq_quantize_mx8(const void* in_dev, void* out8_dev, void* out_scale_dev, int64_t rows, int64_t cols, int dtype, int mant_bits,
                      double epsilon, const uint8_t* exp_win_dev, void* stream);
/* the same image of a PRUNED activation (float_to_bfp_blocked with in_sparsity, identifier 'in': bfp_ops.py:129-149): N:M along the
 * rows in either order (sparsify_first != 0: Q(S(in)), bfp_ops.py:141-144; else S(Q(in)), :146-149; S = _structured_N_M_sparsity,
 * bfp_ops.py:73-91, ties as bfpq_quantize_nm), HBFP(mant_bits + 1) block 64, one pass.  M in {2, 4, 8} (nm_lut: bfpq_nm4_lut_host(N)
 * for M == 4, required; bfpq_nm8_lut_host(N) or NULL for M == 8; ignored otherwise); N == M is the dense image.  Other M, cols % 64 != 0,
 * unaligned pointers: BFPQ_E_UNSUPPORTED (take bfpq_quantize_nm with int8 codes + bfpq_mx8_from_hbfp). */
int bfpq_quantize_mx8_nm(const void* in_dev, void* out8_dev, void* out_scale_dev, int64_t rows, int64_t cols, int dtype, int mant_bits,
                         double epsilon, int N, int M, int sparsify_first, const uint8_t* exp_win_dev, const uint8_t* nm_lut_dev, void* stream);
/* the image of an unstructured-pruned activation, prune first (bfp_ops.py:61-71, :141-144): the apply step of the unstructured path
 * with the threshold that bfpq_select left in ws_dev, writing the image instead of the tensor (so the whole op is two launches:
 * bfpq_select, then this).  Same threshold and tie rule as bfpq_quantize_threshold.  Neither output may overlap the input (the
 * cut-segment workgroups re-read it): BFPQ_E_ARG.  cols % 64 != 0, unaligned pointers, more than 2^30 elements of a 16-bit dtype:
 * BFPQ_E_UNSUPPORTED (take bfpq_quantize_threshold with int8 codes + bfpq_mx8_from_hbfp). */
int bfpq_quantize_threshold_mx8(const void* in_dev, void* out8_dev, void* out_scale_dev, int64_t rows, int64_t cols, int dtype, int mant_bits,
                                double epsilon, const uint8_t* exp_win_dev, void* ws_dev, void* stream);
int bfpq_hbfp_linear_mx8_ok(int64_t T, int64_t N, int64_t K);   /* 1 when the kernel applies */
int bfpq_hbfp_linear_mx8(const void* x8_dev, const void* xscale_dev, const void* w8_dev, const void* wscale_dev, const void* bias_dev,
                         void* out_dev, int64_t T, int64_t N, int64_t K, int out_dtype, void* stream);

/* short token counts (<= 256) leave too few output tiles for the chip (128 tokens x [4096 x 11008]: 32 tiles): K is then split over
 * `parts` workgroups per tile, each writing an fp32 slab, added in part order (deterministic) by a second small launch.
 * bfpq_hbfp_linear_mx8_parts: the number of parts the plan wants for this shape (1: use bfpq_hbfp_linear_mx8);
 * slabs_dev: parts * T * N floats, 16-byte aligned. */
int bfpq_hbfp_linear_mx8_parts(int64_t T, int64_t N, int64_t K);
int bfpq_hbfp_linear_mx8_splitk(const void* x8_dev, const void* xscale_dev, const void* w8_dev, const void* wscale_dev, const void* bias_dev,
                                void* out_dev, float* slabs_dev, int parts, int64_t T, int64_t N, int64_t K, int out_dtype, void* stream);

/* The same product (replaces F.linear on the two fake-quantised operands, bfp_ops.py:187-190) with the PACKED TENSOR ITSELF as the
 * weight operand: wcodes4_dev = the 4-bit codes as bfpq_quantize_nm writes them with code_bits 4 (two's-complement nibbles, low nibble
 * first, row-major [N, K/2] bytes, 16-byte aligned), wexp_dev = their int8 exponents [N, K/64] (4-byte aligned; -128 = NaN block).  The
 * kernel turns nibbles into e4m3 bytes and exponents into E8M0 scales (the rule of bfpq_mx8_from_hbfp) on the way to the matrix
 * instruction, so no weight image exists; the activation operand is its mx8 image as above.  Same tile plans, same walk over K and the
 * same bits as bfpq_hbfp_linear_mx8 on the image of the same weight.  Takes what bfpq_hbfp_linear_mx8_ok takes, with w_mant_bits 1..3
 * (else BFPQ_E_ARG).  BFPQ_TUNE_MX8_VARIANT forces the tile shape here too (0, 1: the 128 x 128 ring; 2: the 256 x 256 ring). */
int bfpq_hbfp_linear_mx4w_ok(int64_t T, int64_t N, int64_t K);
int bfpq_hbfp_linear_mx4w(const void* x8_dev, const void* xscale_dev, const void* wcodes4_dev, const int8_t* wexp_dev, const void* bias_dev,
                          void* out_dev, int64_t T, int64_t N, int64_t K, int out_dtype, int w_mant_bits, void* stream);
/* its split of K for short token counts (replaces the same lines, bfp_ops.py:187-190): the plan and the slabs of
 * bfpq_hbfp_linear_mx8_parts / _splitk, slabs added in part order */
int bfpq_hbfp_linear_mx4w_parts(int64_t T, int64_t N, int64_t K);
int bfpq_hbfp_linear_mx4w_splitk(const void* x8_dev, const void* xscale_dev, const void* wcodes4_dev, const int8_t* wexp_dev, const void* bias_dev,
                                 void* out_dev, float* slabs_dev, int parts, int64_t T, int64_t N, int64_t K, int out_dtype, int w_mant_bits,
                                 void* stream);
/* host: the e4m3 byte (OCP e4m3: sign, 4 exponent bits with bias 7, 3 mantissa bits) that the kernel makes of each 4-bit code 0..15,
 * computed by the kernel's own conversion routine compiled for the host */
int bfpq_e4m3_of_code4_host(uint8_t table[16]);

/* ---- packed-format consumer for HBFP5-HBFP8 (replaces F.linear on the two fake-quantised operands, bfp_ops.py:187-190):
 * out[T, N] = x[T, K] W[N, K]^T (+ bias[N]), both operands int8 codes + int8 block exponents, block 64, mantissa widths
 * x_mant_bits, w_mant_bits in 1..7 (value = code * 2^(exp - mant_bits)), as bfpq_quantize_nm writes them with code_bits 8.
 * Each block's dot product is an exact integer sum on the int8 matrix unit (|sum| < 2^20), scaled once by its two power-of-two
 * block scales and added in block order in fp32.  An exponent byte of -128 (the NaN block marker) on either side makes the block
 * contribute NaN.  The result does not depend on the tile variant or the K split beyond fp32 summation order, and the same inputs
 * give the same bits on every call.
 *   xcodes_dev [T, K] int8, xexp_dev [T, K/64] int8, wcodes_dev [N, K] int8, wexp_dev [N, K/64] int8, bias_dev [N] of out_dtype
 *   (nullable), out_dev [T, N] of out_dtype.
 * bfpq_hbfp_linear_i8 / _splitk (the LDS-tiled prefill kernel): 1 == bfpq_hbfp_linear_i8_ok(T, N, K), i.e. N % 16 == 0 and
 * K % 256 == 0 (other shapes: bfpq_hbfp_linear_decode8); codes and out 16-byte aligned, exponents 4-byte aligned.
 * _splitk: K split over `parts` workgroups per output tile, each writing an fp32 slab, added in part order by a second small launch;
 * slabs_dev: parts * T * N floats, 16-byte aligned.  bfpq_hbfp_linear_i8_parts: the parts the plan wants (1: call bfpq_hbfp_linear_i8). */
int bfpq_hbfp_linear_i8_ok(int64_t T, int64_t N, int64_t K);   /* 1 when the tile kernel applies */
int bfpq_hbfp_linear_i8_parts(int64_t T, int64_t N, int64_t K);
int bfpq_hbfp_linear_i8(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, const void* bias_dev,
                        void* out_dev, int64_t T, int64_t N, int64_t K, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);
int bfpq_hbfp_linear_i8_splitk(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, const void* bias_dev,
                               void* out_dev, float* slabs_dev, int parts, int64_t T, int64_t N, int64_t K, int out_dtype,
                               int w_mant_bits, int x_mant_bits, void* stream);
/* the same product for few tokens (the decode shape; any T >= 1, N % 16 == 0, K % 64 == 0): a wave owns 16 output features x 16 tokens
 * x a slice of K, the slices' fp32 slabs are added in slice order.  bfpq_hbfp_linear_decode8_ws: floats of slabs_dev (16-byte aligned)
 * for this shape, or BFPQ_E_UNSUPPORTED.  Codes 16-byte aligned. */
int64_t bfpq_hbfp_linear_decode8_ws(int64_t T, int64_t N, int64_t K);
int bfpq_hbfp_linear_decode8(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, const void* bias_dev,
                             void* out_dev, float* slabs_dev, int64_t T, int64_t N, int64_t K, int out_dtype,
                             int w_mant_bits, int x_mant_bits, void* stream);
/* The same product with blocks of 16 or 32 (block_size; any other value: BFPQ_E_ARG, before anything touches the device).  Each block's
 * dot product is one v_mfma_i32_16x16x32_i8 (block 16: the second half of K zero in the weight operand), |sum| <= 32 * 127^2 < 2^19,
 * exact; the rescale, the NaN block marker, the block-order fp32 sum and the reproducibility are those of the block-64 entries above.
 *   xexp_dev [T, K/block_size] int8, wexp_dev [N, K/block_size] int8; the rest as above.
 * bfpq_hbfp_linear_i8b / _splitk (the LDS-tiled kernel, 256 of K = 8 or 16 blocks per trip): 1 == bfpq_hbfp_linear_i8b_ok(T, N, K,
 * block_size) (0 for other blocks); codes and out 16-byte aligned, exponents 4-byte (block 32) or 8-byte (block 16) aligned.
 * bfpq_hbfp_linear_i8b_parts: as bfpq_hbfp_linear_i8_parts.  bfpq_hbfp_linear_decode8b / _ws: the few-token kernel (any T >= 1,
 * N % 16 == 0, K % 64 == 0), slabs as for bfpq_hbfp_linear_decode8. */
int bfpq_hbfp_linear_i8b_ok(int64_t T, int64_t N, int64_t K, int block_size);
int bfpq_hbfp_linear_i8b_parts(int64_t T, int64_t N, int64_t K, int block_size);
int bfpq_hbfp_linear_i8b(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, const void* bias_dev,
                         void* out_dev, int64_t T, int64_t N, int64_t K, int block_size, int out_dtype, int w_mant_bits, int x_mant_bits,
                         void* stream);
int bfpq_hbfp_linear_i8b_splitk(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev,
                                const void* bias_dev, void* out_dev, float* slabs_dev, int parts, int64_t T, int64_t N, int64_t K, int block_size,
                                int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);
int64_t bfpq_hbfp_linear_decode8b_ws(int64_t T, int64_t N, int64_t K, int block_size);
int bfpq_hbfp_linear_decode8b(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, const void* bias_dev,
                              void* out_dev, float* slabs_dev, int64_t T, int64_t N, int64_t K, int block_size, int out_dtype,
                              int w_mant_bits, int x_mant_bits, void* stream);
/* 4-bit codes (two's-complement nibbles, low nibble first, as bfpq_quantize_nm writes them) -> int8 codes, so that HBFP4 weights
 * run on the entry points above; n_codes % 8 == 0, codes4_dev 4-byte and codes8_dev 8-byte aligned. */
int bfpq_codes4_to_i8(const void* codes4_dev, void* codes8_dev, int64_t n_codes, void* stream);
/* ---- the batched product of two HBFP activations on the int8 matrix unit (csrc/bfpq_bmm.hip) ----------------------------------------
 * out[b][t][n] = sum_k x[b][t][k] w[b][n][k] for b < B: torch.matmul on the two fake-quantised operands of F_matmul_bfp (reference
 * bfp_ops.py:240-245, the op of :187-190 with the second operand quantized along its contraction dimension, :153), the attention
 * matmuls of the reference's GPT-2 (modeling_gpt2.py:207, 243, 297).  Arithmetic as bfpq_hbfp_linear_i8 / _i8b: one int8 matrix
 * instruction per block of 64, 32 or 16 (an exact integer sum), one rescale by the two block scales, fp32 across blocks in block order,
 * one rounding to out_dtype; an exponent of -128 on either side makes the block contribute NaN.  No bias.
 *   xcodes_dev [B, T, ldk] int8, xexp_dev [B, T, K/block_size] int8, wcodes_dev [B, N, ldk] int8, wexp_dev [B, N, K/block_size] int8,
 *   out_dev [B, T, N] of out_dtype, all dense in b.  ldk: the pitch of a code row, a multiple of 64 and >= K, the codes past K zero.
 * Any T >= 1, N % 16 == 0, K % block_size == 0 (1 == bfpq_hbfp_bmm_i8_ok; else BFPQ_E_UNSUPPORTED).  A block_size other than 16, 32
 * or 64, an unknown out_dtype or a mantissa width outside 1..7: BFPQ_E_ARG.  B, T or N of 0: returns 0, nothing is launched.  Codes
 * and out 16-byte aligned (else, or NULL: BFPQ_E_ARG); exponents any alignment.  Every check returns before anything is launched. */
int bfpq_hbfp_bmm_i8_ok(int64_t B, int64_t T, int64_t N, int64_t K, int64_t ldk, int block_size);
int bfpq_hbfp_bmm_i8(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev, int64_t B,
                     int64_t T, int64_t N, int64_t K, int64_t ldk, int block_size, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);
/* The same product with the second operand read in place from a larger array (the codes of a KV cache): w's code rows have the pitch
 * w_ld (a multiple of 64, >= K rounded up to 64), its exponent rows the pitch w_exp_ld (>= K / block_size), batch b starts w_bstride
 * rows after batch b - 1, and only the first w_rows <= N rows of a batch exist: the rows from w_rows to N are computed from row
 * w_rows - 1 (never read past it) and are the caller's to drop.  x and out as above.  bfpq_hbfp_bmm_i8 is this entry with
 * w_ld = ldk, w_exp_ld = K / block_size, w_bstride = w_rows = N.  A pitch or stride that does not fit: BFPQ_E_UNSUPPORTED. */
int bfpq_hbfp_bmm_i8_strided(const void* xcodes_dev, const int8_t* xexp_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev,
                             int64_t B, int64_t T, int64_t N, int64_t K, int64_t ldk, int64_t w_ld, int64_t w_exp_ld, int64_t w_bstride,
                             int64_t w_rows, int block_size, int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);
/* The second operand of that product when its blocks run along its second-to-last dimension (V of P V): in_dev [B, S, D] of dtype,
 * dense -> int8 codes [B, D, ldk] + int8 exponents [B, D, S/block_size] of float_to_bfp_blocked(in.transpose(-1, -2), identifier 'w')
 * (reference bfp_ops.py:153 with :29-59: the transposed copy, the quantizer and the transpose back), round-half-even, no pruning; one
 * read of in_dev, a tile transpose through LDS.  code * 2^(exp - mant_bits) is that operand bit for bit (up to the sign of zero); the
 * codes from S to ldk are written as zeros.  block_size 16, 32 or 64 and mant_bits 1..7 (else BFPQ_E_ARG); S % block_size == 0,
 * D % 16 == 0, ldk % 64 == 0, ldk >= S (else BFPQ_E_UNSUPPORTED); B, S or D of 0 returns 0.  in_dev and codes_dev 16-byte aligned;
 * exp_win_dev: bfpq_exp_window_host(dtype) on the device. */
int bfpq_hbfp_codes_t(const void* in_dev, void* codes_dev, int8_t* exps_dev, int64_t B, int64_t S, int64_t D, int64_t ldk, int dtype,
                      int block_size, int mant_bits, double epsilon, const uint8_t* exp_win_dev, void* stream);
/* ---- attention keys and values held as HBFP codes across decode steps (csrc/bfpq_kvcache.hip) ----------------------------------------
 * Replaces, for decoding with layer_past (reference modeling_gpt2.py:345-348, 415-419), the torch.cat of the past keys / values and the
 * quantization of all of K along D and of all of V^T along S at every step (bfp_ops.py:240-245 through :187-190 and :153).  Per head
 * b < BH, capacity cap tokens (bfpq_kv_ok: block_size 16, 32 or 64, D % block_size == 0, D % 16 == 0, D <= 1024, cap % 64 == 0):
 *   k_codes [BH, cap, ldd] int8 (ldd % 64 == 0, >= D), k_exps [BH, cap, D / block_size] int8: blocks along D;
 *   v_codes [BH, D, cap] int8 (zeroed by the caller once), v_exps [BH, D, cap / block_size] int8: blocks along the tokens;
 *   v_tail  [BH, block_size, D] of dtype: the original values of the token block that is still open.
 * bfpq_kv_append: k_new, v_new [BH, t, D] of dtype become tokens pos .. pos + t - 1 (pos = tokens held so far, pos + t <= cap, any
 * t >= 1 in one call).  Key rows are quantized once.  Every token block of V the chunk touches is quantized from original values --
 * v_tail for the tokens before pos, v_new for the chunk, zeros for the tokens not yet there (the reference's zero pad of a ragged last
 * block, bfp_ops.py:50-53) -- so after every call code * 2^(exp - mant_bits) equals float_to_bfp_blocked(K_all, identifier 'w') and
 * float_to_bfp_blocked(V_all^T, identifier 'w') bit for bit (up to the sign of zero), and the codes from pos + t to the end of the
 * open block are zero.  Unknown dtype / block_size, mant_bits outside 1..7, a negative size, a NULL or (float arrays, codes) not
 * 16-byte aligned pointer: BFPQ_E_ARG; a shape bfpq_kv_ok refuses, a bad ldd or pos + t > cap: BFPQ_E_UNSUPPORTED; BH or t of 0
 * returns 0.  Every check returns before anything is launched.  exp_win_dev: bfpq_exp_window_host(dtype) on the device. */
int bfpq_kv_ok(int64_t D, int64_t cap, int block_size);
int bfpq_kv_append(const void* k_new_dev, const void* v_new_dev, void* k_codes_dev, int8_t* k_exps_dev, void* v_codes_dev, int8_t* v_exps_dev,
                   void* v_tail_dev, int64_t BH, int64_t D, int64_t pos, int64_t t, int64_t cap, int64_t ldd, int dtype, int block_size,
                   int mant_bits, double epsilon, const uint8_t* exp_win_dev, void* stream);
/* The decode product against one cached operand, the few-token operand quantized inside the kernel (reference bfp_ops.py:187-190 on
 * (q, K_all^T) or (p, V_all) of modeling_gpt2.py:207, 243): out[b][t][n] = sum_k Q(x)[b][t][k] w[b][n][k] for t < Tq <=
 * BFPQ_KV_DEC_MAX_TOKENS, x [B, Tq, ldx] of dtype (Kx elements per row, dense, unpruned), out [B, Tq, ldo] of dtype (Nout per row,
 * ldo % 4 == 0: the entries from Nout to ldo may be written), w the codes (row pitch ldw, a multiple of 64), exponents (row pitch ldwe)
 * and batch stride in rows (w_bstride) of
 *   BFPQ_KV_QK: k_codes -- n the Nout = S cached keys, k the Kx = D elements of a key (Kx % block_size == 0);
 *   BFPQ_KV_PV: v_codes -- n the Nout = D columns (Nout % 16 == 0), k the Kx = S cached tokens, any S >= 1: x's last block is quantized
 *               with zeros past S, which is the reference's zero pad; the cache holds zero codes there.
 * Arithmetic as bfpq_hbfp_bmm_i8 (an exact integer sum per block, one rescale, fp32 across blocks in block order, -128 = NaN block):
 * on the same operands the same bits.  Rows of w at or past Nout are never read.  Errors as above; Tq > BFPQ_KV_DEC_MAX_TOKENS or a
 * pitch that does not fit: BFPQ_E_UNSUPPORTED; B, Tq or Nout of 0 returns 0.  w's codes and out 16-byte aligned. */
#define BFPQ_KV_QK 0
#define BFPQ_KV_PV 1
#define BFPQ_KV_DEC_MAX_TOKENS 16
int bfpq_kv_bmm_dec(const void* x_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev, int64_t B, int64_t Tq, int64_t Kx,
                    int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo, int family, int dtype,
                    int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* stream);
/* The same cache with the lengths in device memory, one per sequence: a ragged batch, and a decode step that a captured graph can
 * replay (the reference's layer_past grows by torch.cat on the host, modeling_gpt2.py:345-348, 415-419; bfp_ops.py:240-245, :187-190,
 * :153 as above).  Head b < BH belongs to sequence b / heads (heads >= 1, BH % heads == 0; else BFPQ_E_ARG); lens_dev [BH / heads]
 * int32 holds the tokens of each sequence.  No entry reads anything back or synchronises.
 * bfpq_kv_append_dev: bfpq_kv_append with pos = lens_dev[b / heads] and, of the t rows of k_new / v_new [BH, t, D], only the first
 * counts_dev[b / heads] taken (counts_dev NULL: all t).  t is the row pitch and bounds the grid, which is sized for the worst position
 * ((t + block_size - 2) / block_size + 1 token blocks of V); workgroups whose block a sequence does not have exit.  A sequence with a
 * count outside 0..t, a length outside 0..limit or lens + count > limit (limit: the tokens a sequence may hold, 1..cap) is left
 * untouched -- no codes, no v_tail -- and overflow_dev[0] (int32) is set to 1 by the kernel; nothing ever clears it but the caller.
 * lens_dev is only read: bfpq_kv_lens_advance, a launch of its own after it in stream order (so no workgroup of the append can see a
 * moved length), adds to lens_dev[b] what sequence b took by the same rule.  Errors as bfpq_kv_append; limit outside 1..cap or t > cap:
 * BFPQ_E_UNSUPPORTED; the int32 arrays NULL (counts_dev may be) or not 4-byte aligned: BFPQ_E_ARG. */
int bfpq_kv_append_dev(const void* k_new_dev, const void* v_new_dev, void* k_codes_dev, int8_t* k_exps_dev, void* v_codes_dev, int8_t* v_exps_dev,
                       void* v_tail_dev, const int32_t* lens_dev, const int32_t* counts_dev, int32_t* overflow_dev, int64_t BH, int64_t heads,
                       int64_t D, int64_t t, int64_t cap, int64_t limit, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon,
                       const uint8_t* exp_win_dev, void* stream);
int bfpq_kv_lens_advance(int32_t* lens_dev, const int32_t* counts_dev, int64_t B, int64_t t, int64_t limit, void* stream);
/* bfpq_kv_bmm_dec with the cached length of head b read from lens_dev[b / heads] and a host bound that sizes the grid and the arrays:
 *   BFPQ_KV_QK: Nout = max_len, 1 <= max_len <= w_bstride.  Column n < min(lens, max_len) of out [B, Tq, ldo] is the product, every
 *               column from there to max_len is -inf (a softmax over the row ignores it).
 *   BFPQ_KV_PV: Kx = L, the elements of a row of x, 1 <= L <= ldw; Nout = w_bstride = D <= 1024, B <= 65535.  Head b contracts over its
 *               first min(lens, L) tokens; what x holds at or past that counts as zero, NaN and Inf included (the reference's zero pad,
 *               bfp_ops.py:50-53); a sequence of length 0 gives zeros.  The contraction is split over workgroups: slices of
 *               chunks_per_split 64-token chunks (1..16; 0: the library chooses) write each block's exact integer sum and x's block
 *               exponents to ws_dev (16-byte aligned, ws_bytes >= bfpq_kv_dec_ws_bytes(B, Tq, D, L, block_size)), and a second launch
 *               rescales and adds the blocks in block order: the fp32 additions of bfpq_kv_bmm_dec in its order, the same bits for
 *               every chunks_per_split.
 * Errors as bfpq_kv_bmm_dec; Nout or Kx of 0, a workspace too small or chunks_per_split > 16: BFPQ_E_UNSUPPORTED; lens_dev or (PV)
 * ws_dev NULL or misaligned, a bad heads or a negative chunks_per_split: BFPQ_E_ARG; B or Tq of 0 returns 0.
 * bfpq_kv_dec_ws_bytes: a negative error code for arguments the product refuses. */
int64_t bfpq_kv_dec_ws_bytes(int64_t B, int64_t Tq, int64_t D, int64_t L, int block_size);
int bfpq_kv_bmm_dec_dev(const void* x_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev, const int32_t* lens_dev, int64_t B,
                        int64_t heads, int64_t Tq, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe, int64_t w_bstride, int64_t ldo,
                        int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev,
                        void* ws_dev, int64_t ws_bytes, int64_t chunks_per_split, void* stream);
/* One attention call on the device-length cache: scores, scale, softmax and context of a decode step (reference modeling_gpt2.py:207-243:
 * the matmul of q and K^T, the scale, the causal mask, the softmax and the matmul with V) in three launches, no array of the dtype with
 * a row per cached token in between.  q [BH, Tq, D] of dtype (dense), out [BH, Tq, ldo] of dtype (D per row, ldo % 4 == 0); the cache
 * arrays, lens_dev and heads as above, max_len (1..cap) as bfpq_kv_bmm_dec_dev's BFPQ_KV_QK bound.  The result is that of
 *   s = bfpq_kv_bmm_dec_dev(BFPQ_KV_QK, q), widened to fp32 and multiplied by (float)scale (scale finite; else BFPQ_E_ARG);
 *   row t of head b sees the keys n < min(lens, max_len), with causal = 1 only n <= lens - Tq + t (the rows are the last Tq tokens held);
 *   p = softmax over the keys the row sees, in fp32 -- the maximum (NaN propagates), expf(s - max), the sum in an order that depends on
 *       the row alone, a division -- rounded once to dtype, +0 at every other key;
 *   out = bfpq_kv_bmm_dec_dev(BFPQ_KV_PV, p) bit for bit, for every chunks_per_split.
 * An empty sequence gives zeros; a row that sees no key of a sequence that holds some (causal with Tq > lens) has a p of zeros and
 * gives what BFPQ_KV_PV gives for it.  p_dev, if not NULL: [BH, Tq, ldp] of dtype
 * (ldp >= max_len) receives p, columns 0 .. max_len - 1 of every row.  score_ws_dev: the fp32 score rows, 16-byte aligned,
 * score_ws_bytes >= bfpq_kv_attend_ws_bytes(BH, Tq, max_len) = 4 BH Tq (max_len rounded up to 4), rounded up to 16 (no device needed;
 * a negative size: BFPQ_E_ARG, Tq > BFPQ_KV_DEC_MAX_TOKENS or a size of 2^31 or more: BFPQ_E_UNSUPPORTED); sum_ws_dev: the workspace of
 * bfpq_kv_bmm_dec_dev's BFPQ_KV_PV family, sum_ws_bytes >= bfpq_kv_dec_ws_bytes(BH, Tq, D, max_len, block_size).  Errors as
 * bfpq_kv_bmm_dec_dev; causal not 0 or 1: BFPQ_E_ARG; max_len outside 1..cap, BH > 65535, ldp < max_len or a workspace too small:
 * BFPQ_E_UNSUPPORTED; BH or Tq of 0 returns 0.  Nothing is read back. */
int64_t bfpq_kv_attend_ws_bytes(int64_t BH, int64_t Tq, int64_t max_len);
int bfpq_kv_attend(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                   void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t D, int64_t max_len,
                   int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size, int x_mant_bits,
                   int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev, int64_t score_ws_bytes, void* sum_ws_dev,
                   int64_t sum_ws_bytes, int64_t chunks_per_split, void* stream);
/* Grouped-query attention on the device-length cache (reference modeling_llama.py:397-409: repeat_kv of the key and value states --
 * :264-273, kv head h serving the query heads h g .. h g + g - 1 -- and the two matmuls, the mask and the softmax between them).  The
 * cache arrays hold B (resp. BH) kv heads, `heads` of them per sequence; every kv head serves `group` >= 1 query heads, and x / q, out
 * and p are [B, group * Tq, .]: row r of kv head b is query head r / Tq of its group, token r % Tq (the contiguous view of
 * [sequences, heads * group, Tq, .]).  Nothing is repeated: the rows are walked in tiles of 16, a tile's rows sharing every load of
 * the codes (which are read again per tile).  The result is
 * bit for bit that of the entry without _gqa on B * group heads whose cache arrays repeat every kv head group times: per row nothing
 * depends on the other rows of its tile.  Tq <= BFPQ_KV_DEC_MAX_TOKENS stays a limit per query head; the workspaces are those of
 * B * group heads: ws_bytes >= bfpq_kv_dec_ws_bytes(B * group, Tq, D, L, block_size), score_ws_bytes >=
 * bfpq_kv_attend_ws_bytes(BH * group, Tq, max_len).  causal and max_len as bfpq_kv_attend, per token.  Errors as the entries without
 * _gqa, which are these with group = 1; group < 1: BFPQ_E_ARG; more than 65535 (kv head, row tile) pairs where bfpq_kv_bmm_dec_dev
 * refuses B > 65535, or group * Tq rows whose pitch does not fit: BFPQ_E_UNSUPPORTED. */
int bfpq_kv_bmm_dec_gqa(const void* x_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev, const int32_t* lens_dev, int64_t B,
                        int64_t heads, int64_t Tq, int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe,
                        int64_t w_bstride, int64_t ldo, int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                        const uint8_t* exp_win_dev, void* ws_dev, int64_t ws_bytes, int64_t chunks_per_split, void* stream);
int bfpq_kv_attend_gqa(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                       void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                       int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                       int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev, int64_t score_ws_bytes,
                       void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split, void* stream);
/* Prompt attention on the device-length cache: bfpq_kv_attend_gqa for any number of query tokens, walked in panels (the same reference
 * lines -- modeling_gpt2.py:207-243, the matmul of q and K^T, the scale, the causal mask, the softmax and the matmul with V, and
 * modeling_llama.py:397-409 with repeat_kv, :264-273 -- for the Tq tokens of a prompt or of one chunk of it, where the reference makes
 * the [.., Tq, S] scores and probabilities in the dtype).  Every argument as bfpq_kv_attend_gqa, except: Tq is any count >= 0 and one
 * call covers the query tokens row0 .. row0 + rows - 1 of every query head (0 <= row0, row0 + rows <= Tq), reading those rows of q
 * [BH, group * Tq, D] and writing those rows of out and p; causal sight goes by the token's index in the whole Tq, row t seeing the keys
 * n <= lens - Tq + t.  Two launches per call: q k^T of the panel into score_ws_dev (16-byte aligned, score_ws_bytes >=
 * bfpq_kv_attend_rows_ws_bytes(BH * group, rows, max_len) = 4 BH group rows (max_len rounded up to 4), rounded up to 16; no device
 * needed; a size of 2^31 or more: BFPQ_E_UNSUPPORTED), then softmax and p v with the fp32 accumulators in registers.  There are no
 * block sums: sum_ws_dev, sum_ws_bytes and chunks_per_split (0..16) are taken and not used, sum_ws_dev may be NULL.  Row for row the
 * result is bit for bit bfpq_kv_attend_gqa's for that row -- nothing a row computes depends on Tq, on the panel or on the rows beside
 * it -- with the row's visible length that of its token.  D <= 256 and q 16-byte aligned here; else errors as bfpq_kv_attend_gqa; row0
 * or rows negative or past Tq: BFPQ_E_ARG; rows of 0 returns 0.  Nothing is read back. */
int64_t bfpq_kv_attend_rows_ws_bytes(int64_t BH, int64_t P, int64_t max_len);
int bfpq_kv_attend_rows(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                        void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                        int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                        int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev, int64_t score_ws_bytes,
                        void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows, void* stream);
/* A first visible key per query row: left-padded batches and sliding-window attention on the device-length cache (the reference's
 * transformers tree: batched generate() pads on the left and the additive attention_mask hides the pad tokens, modeling_gpt2.py:228-230,
 * modeling_llama.py:402-404; the sliding_window of modeling_attn_mask_utils.py, row i seeing the keys i - W + 1 .. i).  The two entries
 * are bfpq_kv_attend_gqa and bfpq_kv_attend_rows with two more arguments in front of the stream: starts_dev, int32 [sequences] on the
 * device or NULL, read at launch and never on the host (a negative start counts as 0), and window (0: none).  With len = lens,
 * v = causal ? len - Tq + t + 1 : len and hi = clamp(v, 0, min(len, max_len)) as before, row t sees the keys lo <= n < hi,
 * lo = max(0, starts[sequence], v - window); where lo >= hi it sees none and is the row that sees no key of the entries above.  Keys
 * below lo are +0 in p.  Everything a row computes is, bit for bit, what the entry without _win computes for it with -inf scores
 * below lo; tiles, slices and blocks below every row's lo are skipped (the combine pass still walks every block).  The same
 * workspaces.  Pad tokens are cached tokens like any other: nothing is evicted.  Errors as the entry each extends; window < 0 or
 * starts_dev not 4-byte aligned: BFPQ_E_ARG.  starts_dev NULL and window 0 launch the kernels of the entry without _win. */
int bfpq_kv_attend_gqa_win(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                           void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                           int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype,
                           int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev,
                           int64_t score_ws_bytes, void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split, const int32_t* starts_dev,
                           int64_t window, void* stream);
int bfpq_kv_attend_rows_win(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                            void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                            int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype,
                            int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev,
                            int64_t score_ws_bytes, void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows,
                            const int32_t* starts_dev, int64_t window, void* stream);
/* A paged device-length cache: sequences draw pages of page_tokens tokens from one pool instead of reserving cap tokens each.  The five
 * entries are bfpq_kv_append_dev, bfpq_kv_lens_advance, bfpq_kv_bmm_dec_gqa, bfpq_kv_attend_gqa and bfpq_kv_attend_rows with, in front of
 * the stream, page_table_dev -- int32 [sequences, cap / page_tokens] on the device, read at launch and never on the host, entry
 * [b][s / page_tokens] the page of sequence b's token s, -1 for none -- then page_tokens (a multiple of 64, so a page holds whole token
 * blocks at every block size and whole 64-key tiles) and pages, the number of pages in the pool.  cap becomes the most tokens one sequence
 * may hold (cap % page_tokens == 0; bfpq_kv_lens_advance_paged and bfpq_kv_bmm_dec_paged take it as one more argument in front of the
 * table), and the cache arrays hold pages, a page being page_tokens tokens of all `heads` heads of one sequence:
 *   k_codes [pages, heads, page_tokens, ldd]   k_exps [pages, heads, page_tokens, D / block_size]
 *   v_codes [pages, heads, D, page_tokens]     v_exps [pages, heads, D, page_tokens / block_size]
 * so a page seen through one head is a contiguous head of capacity page_tokens; v_tail stays [BH, block_size, D], per sequence.  On the
 * same appended tokens every result is, bit for bit, that of the entry each extends on a contiguous cache: only where the bytes lie
 * changes.  bfpq_kv_append_paged refuses a sequence, as bfpq_kv_append_dev refuses one that would pass `limit`, where a token it would
 * take has an entry outside 0 .. pages - 1: it is left untouched and overflow_dev[0] set to 1; bfpq_kv_lens_advance_paged leaves its
 * length by the same rule.  Nothing allocates: the table is the caller's.  The products read the pages of tokens below lens_dev only,
 * which an append has checked; an entry outside 0 .. pages - 1 met there all the same is clamped into the pool, never dereferenced as
 * it is.  bfpq_kv_bmm_dec_paged: BFPQ_KV_QK takes w_bstride = page_tokens and Nout = max_len <= cap, BFPQ_KV_PV ldw = page_tokens, ldwe
 * = page_tokens / block_size and L <= cap.  No first visible key per row here (no starts, no window).  Errors as the entry each
 * extends; page_tokens not a multiple of 64, cap not a multiple of page_tokens or pages < 1: BFPQ_E_ARG; page_table_dev NULL or not
 * 4-byte aligned: BFPQ_E_ARG; pages * heads or page_tokens * ldd of 2^31 or more: BFPQ_E_UNSUPPORTED. */
int bfpq_kv_append_paged(const void* k_new_dev, const void* v_new_dev, void* k_codes_dev, int8_t* k_exps_dev, void* v_codes_dev,
                         int8_t* v_exps_dev, void* v_tail_dev, const int32_t* lens_dev, const int32_t* counts_dev, int32_t* overflow_dev,
                         int64_t BH, int64_t heads, int64_t D, int64_t t, int64_t cap, int64_t limit, int64_t ldd, int dtype, int block_size,
                         int mant_bits, double epsilon, const uint8_t* exp_win_dev, const int32_t* page_table_dev, int64_t page_tokens,
                         int64_t pages, void* stream);
int bfpq_kv_lens_advance_paged(int32_t* lens_dev, const int32_t* counts_dev, int64_t B, int64_t t, int64_t limit, int64_t cap,
                               const int32_t* page_table_dev, int64_t page_tokens, int64_t pages, void* stream);
int bfpq_kv_bmm_dec_paged(const void* x_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev, const int32_t* lens_dev, int64_t B,
                          int64_t heads, int64_t Tq, int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe,
                          int64_t w_bstride, int64_t ldo, int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits,
                          double epsilon, const uint8_t* exp_win_dev, void* ws_dev, int64_t ws_bytes, int64_t chunks_per_split, int64_t cap,
                          const int32_t* page_table_dev, int64_t page_tokens, int64_t pages, void* stream);
int bfpq_kv_attend_paged(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                         void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                         int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype,
                         int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev,
                         int64_t score_ws_bytes, void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split,
                         const int32_t* page_table_dev, int64_t page_tokens, int64_t pages, void* stream);
int bfpq_kv_attend_rows_paged(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev,
                              const int8_t* v_exps_dev, void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads,
                              int64_t Tq, int64_t group, int64_t D, int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp,
                              double scale, int causal, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                              const uint8_t* exp_win_dev, void* score_ws_dev, int64_t score_ws_bytes, void* sum_ws_dev, int64_t sum_ws_bytes,
                              int64_t chunks_per_split, int64_t row0, int64_t rows, const int32_t* page_table_dev, int64_t page_tokens,
                              int64_t pages, void* stream);
/* Pages shared between the sequences of a paged cache (csrc/bfpq_kvpages.hip).  Replaces the reference's _reorder_cache
 * (modeling_gpt2.py:1370-1379, and the same in LLaMA and OPT): past_state.index_select(0, beam_idx) of every layer's keys and values at
 * every step of a beam search.  A full page is immutable (key rows are final once appended, token blocks of V once closed, and pages hold
 * whole blocks), so the caller reorders by editing page_table rows, which may then name one page more than once; what is left for the
 * device is one job per new row that does not simply stay what it was, jobs_dev int32 [n_jobs, 5] on the device:
 *   src_row, dst_row   sequences in 0 .. B - 1: dst_row becomes what src_row is
 *   src_page, dst_page pages in 0 .. pages - 1: the open page of src_row copied into a page no job reads (all kv_heads heads of the
 *                      four pool arrays; their layout as above, ldd = D rounded up to 64), or both -1: no page to copy
 *   tokens             the length of src_row the caller planned the pages with
 * Two launches, so that rows may be each other's source (a cycle).  The first copies the pages (16-byte vector loads and stores; every
 * piece is a multiple of 16 bytes) and stages v_tail[src_row] and lens_dev[src_row] of every job in stage_dev; it stages the length only
 * where it equals `tokens`, else 0, setting overflow_dev[0] to 1 (left so, as by a refused append): a wrong count gives an empty row,
 * never one that reads pages it was not given.  The second writes v_tail[dst_row] and lens_dev[dst_row] from stage_dev.  A job with a row
 * or a page outside its range (or one page of -1 only) does nothing in either launch and sets overflow_dev[0]: a bad list cannot fault.
 * Two jobs with one dst_row, or a dst_page that another job reads, are the caller's error and leave either's bytes.  Nothing is read
 * back.  stage_dev: bfpq_kv_rows_move_ws_bytes(n_jobs, ...) bytes -- n_jobs * kv_heads * block_size * D elements of dtype, then n_jobs
 * int32 rounded up to 16 bytes -- 16-byte aligned; that function returns a negative BFPQ_E_* for arguments it does not take.
 * Unknown dtype / block_size, n_jobs < 0, B or kv_heads < 1, page_tokens not a multiple of 64 or pages < 1: BFPQ_E_ARG; a shape
 * bfpq_kv_ok(D, page_tokens, block_size) refuses or a size of 2^31 or more: BFPQ_E_UNSUPPORTED; n_jobs of 0 returns 0; a NULL or
 * misaligned pointer (the pool arrays, v_tail and stage_dev 16 bytes, the int32 arrays 4) or stage_bytes too small: BFPQ_E_ARG.  Every
 * check returns before anything is launched. */
int64_t bfpq_kv_rows_move_ws_bytes(int64_t n_jobs, int64_t kv_heads, int64_t D, int block_size, int dtype);
int bfpq_kv_rows_move(void* k_codes_dev, int8_t* k_exps_dev, void* v_codes_dev, int8_t* v_exps_dev, void* v_tail_dev, int32_t* lens_dev,
                      int32_t* overflow_dev, const int32_t* jobs_dev, int64_t n_jobs, void* stage_dev, int64_t stage_bytes, int64_t B,
                      int64_t kv_heads, int64_t D, int block_size, int dtype, int64_t page_tokens, int64_t pages, void* stream);
/* A device-length cache that holds 4-bit codes (csrc/bfpq_kvcache.hip, the C4 instances).  What the reference keeps as layer_past
 * (modeling_gpt2.py:345-348, 415-419; modeling_llama.py:385-409 for grouped queries) and quantizes again at every step is, for
 * mant_bits <= 3, a tensor of codes in -7..7: the two code arrays then hold two codes to a byte and half the bytes,
 *   k_codes [BH, cap, ldd / 2]   v_codes [BH, D, cap / 2]     (paged: [pages, heads, page_tokens, ldd / 2], [pages, heads, D, page_tokens / 2])
 * element 2 k of a key row -- of a column of V: token 2 k -- in the low nibble of byte k and element 2 k + 1 in its high nibble, two's
 * complement: the layout of bfpq_codes4_to_i8 and of bfpq_dequantize with code_bits 4.  The exponent arrays, v_tail, lens, overflow,
 * starts, the page table, the workspaces and every size and pitch argument (ldd, cap, ldw, w_bstride: still counted in codes) are
 * unchanged, and the NaN block marker is the exponent byte -128 as before.  The five entries are bfpq_kv_append_dev, bfpq_kv_bmm_dec_gqa,
 * bfpq_kv_attend_gqa, bfpq_kv_attend_rows and bfpq_kv_rows_move with, in front of the stream: starts_dev and window where the _win entry
 * has them (the two attends); cap (bfpq_kv_bmm_dec_cb, as bfpq_kv_bmm_dec_paged) and page_table_dev, page_tokens, pages as the _paged
 * entry has them (all but bfpq_kv_rows_move_cb, which has them already) -- a NULL table with page_tokens == 0 and pages == 0 is the
 * contiguous cache, and cap is then not read by bfpq_kv_bmm_dec_cb --; and code_bits, 8 or 4.  With code_bits 8 an entry is, argument
 * for argument and launch for launch, the entry it extends (or its _win / _paged form).  With code_bits 4 the cached operand is loaded
 * as half the bytes and widened to the same int8 matrix-unit operand in registers, and an append stores whole bytes only: every result
 * -- the codes read back through bfpq_dequantize, the exponents, lens, overflow, the products, p and the context -- is bit for bit that
 * of code_bits 8 on the same calls.  bfpq_kv_rows_move_cb copies kv_heads page_tokens ldd / 2 and kv_heads D page_tokens / 2 bytes of a
 * page's codes (multiples of 16 still); bfpq_kv_rows_move_ws_bytes, bfpq_kv_lens_advance[_paged], bfpq_kv_ok and the workspace sizes
 * serve both widths.  Errors as the entry each extends, after these, which return before anything is launched: code_bits not 4 or 8, or
 * 4 with block_size != 64 or (where the entry has one) the cache's mant_bits / w_mant_bits > 3: BFPQ_E_ARG; a table, page_tokens or
 * pages that are not all absent and not what the _paged entry takes: as there; starts_dev misaligned or window < 0: BFPQ_E_ARG; a
 * paged cache with starts_dev or window != 0: BFPQ_E_UNSUPPORTED. */
int bfpq_kv_append_cb(const void* k_new_dev, const void* v_new_dev, void* k_codes_dev, int8_t* k_exps_dev, void* v_codes_dev, int8_t* v_exps_dev,
                      void* v_tail_dev, const int32_t* lens_dev, const int32_t* counts_dev, int32_t* overflow_dev, int64_t BH, int64_t heads,
                      int64_t D, int64_t t, int64_t cap, int64_t limit, int64_t ldd, int dtype, int block_size, int mant_bits, double epsilon,
                      const uint8_t* exp_win_dev, const int32_t* page_table_dev, int64_t page_tokens, int64_t pages, int code_bits,
                      void* stream);
int bfpq_kv_bmm_dec_cb(const void* x_dev, const void* wcodes_dev, const int8_t* wexp_dev, void* out_dev, const int32_t* lens_dev, int64_t B,
                       int64_t heads, int64_t Tq, int64_t group, int64_t Kx, int64_t Nout, int64_t ldx, int64_t ldw, int64_t ldwe,
                       int64_t w_bstride, int64_t ldo, int family, int dtype, int block_size, int x_mant_bits, int w_mant_bits, double epsilon,
                       const uint8_t* exp_win_dev, void* ws_dev, int64_t ws_bytes, int64_t chunks_per_split, int64_t cap,
                       const int32_t* page_table_dev, int64_t page_tokens, int64_t pages, int code_bits, void* stream);
int bfpq_kv_attend_cb(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                      void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                      int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype, int block_size,
                      int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev, int64_t score_ws_bytes,
                      void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split, const int32_t* starts_dev, int64_t window,
                      const int32_t* page_table_dev, int64_t page_tokens, int64_t pages, int code_bits, void* stream);
int bfpq_kv_attend_rows_cb(const void* q_dev, const void* k_codes_dev, const int8_t* k_exps_dev, const void* v_codes_dev, const int8_t* v_exps_dev,
                           void* out_dev, void* p_dev, const int32_t* lens_dev, int64_t BH, int64_t heads, int64_t Tq, int64_t group, int64_t D,
                           int64_t max_len, int64_t cap, int64_t ldd, int64_t ldo, int64_t ldp, double scale, int causal, int dtype,
                           int block_size, int x_mant_bits, int w_mant_bits, double epsilon, const uint8_t* exp_win_dev, void* score_ws_dev,
                           int64_t score_ws_bytes, void* sum_ws_dev, int64_t sum_ws_bytes, int64_t chunks_per_split, int64_t row0, int64_t rows,
                           const int32_t* starts_dev, int64_t window, const int32_t* page_table_dev, int64_t page_tokens, int64_t pages,
                           int code_bits, void* stream);
int bfpq_kv_rows_move_cb(void* k_codes_dev, int8_t* k_exps_dev, void* v_codes_dev, int8_t* v_exps_dev, void* v_tail_dev, int32_t* lens_dev,
                         int32_t* overflow_dev, const int32_t* jobs_dev, int64_t n_jobs, void* stage_dev, int64_t stage_bytes, int64_t B,
                         int64_t kv_heads, int64_t D, int block_size, int dtype, int64_t page_tokens, int64_t pages, int code_bits,
                         void* stream);
/* ---- 2:4-compressed packed weights (format sp24) and their few-token product on v_smfmac_i32_16x16x64_i8 -------------------------
 * A weight pruned N:M with M = 4, N <= 2 along K (_structured_N_M_sparsity, reference bfp_ops.py:73-91) and quantized to HBFP block 64
 * holds at most 2 non-zero codes per group of 4.  sp24 keeps those two codes and their 2-bit positions, tiled for the decode kernel
 * (16 rows per tile; per lane and block of 64 K: 8 values + 16 position bits; layout in csrc/bfpq_sp24.hip), and the [N, K/64] int8
 * exponents of the dense packed weight unchanged (-128 = NaN block).  N % 16 == 0, K % 64 == 0, code_bits 4 or 8:
 *   vals_dev: N * K / 4 bytes (4-bit codes) or N * K / 2 bytes (8-bit codes); idx_dev: N * K / 8 bytes -- 0.391 / 0.641 B per weight
 *   with the exponents.  All sp24 arrays 16-byte aligned.
 * bfpq_sp24_pack: dense codes (as bfpq_quantize_nm writes them with code_bits 4 or 8, [N, K] elements) -> sp24.  status_dev[0]
 * (int32, zeroed by the caller) is set to 1 if some group had more than 2 non-zero codes; a group with fewer keeps the lowest free
 * positions, with zero values.  bfpq_sp24_unpack: the exact inverse, into codes of the same width (codes_dev) and / or int8 codes
 * (codes8_dev, [N, K]); either may be NULL, not both. */
int bfpq_sp24_pack(const void* codes_dev, void* vals_dev, void* idx_dev, int64_t N, int64_t K, int code_bits, int32_t* status_dev, void* stream);
int bfpq_sp24_unpack(const void* vals_dev, const void* idx_dev, void* codes_dev, void* codes8_dev, int64_t N, int64_t K, int code_bits,
                     void* stream);
/* out[T, N] = x[T, K] W[N, K]^T (+ bias[N]) for 1 <= T <= BFPQ_SP24_MAX_TOKENS, W in sp24 form (w_mant_bits 1..3 for 4-bit codes, 1..7
 * for 8-bit codes), x as int8 codes [T, K] + int8 exponents [T, K/64] (x_mant_bits 1..7), the product of the two fake-quantised operands
 * of the reference (bfp_ops.py:187-190).  One sparse instruction per block: an exact integer sum, scaled once by the two block scales,
 * added in block order in fp32; the K slices' fp32 slabs are added in slice order (with the bias) by a second launch.  An exponent of
 * -128 on either side makes the block contribute NaN.  slabs_dev: bfpq_hbfp_linear_sp24_ws(T, N, K) floats (BFPQ_E_UNSUPPORTED for
 * shapes this entry does not take).  xcodes_dev 16-byte aligned.  Checks return before anything is launched. */
#define BFPQ_SP24_MAX_TOKENS 64
int64_t bfpq_hbfp_linear_sp24_ws(int64_t T, int64_t N, int64_t K);
int bfpq_hbfp_linear_sp24(const void* xcodes_dev, const int8_t* xexp_dev, const void* wvals_dev, const void* widx_dev, const int8_t* wexp_dev,
                          const void* bias_dev, void* out_dev, float* slabs_dev, int64_t T, int64_t N, int64_t K, int code_bits,
                          int out_dtype, int w_mant_bits, int x_mant_bits, void* stream);
/* *flag_dev = 1 if some byte of the exponent arrays exp_a [n_a] / exp_b [n_b] (either may be empty) is 127, else 0: the blocks whose
 * 2^e can overflow the operand dtype.  A stochastically rounded block there may hold +-2^m codes (the reference's clamp bound is
 * infinite), which no int8 or e4m3 operand carries, so the caller redoes such a call on the fake-quantize route. */
int bfpq_exp_top_flag(const int8_t* exp_a, int64_t n_a, const int8_t* exp_b, int64_t n_b, int* flag_dev, void* stream);

/* ---- fused BFPAdam step (replaces BFPAdam.step's per-parameter body, bfp_optim_lstm.py:62-87, and its snap
 * float_to_bfp_blocked(p, sgd_update=True) = _no_sparsity_float_to_bfp, bfp_ops.py:46-59) ------------------------------------
 * For every fp32 tensor of the list, in place, element by element:
 *     g' = weight_decay != 0 ? g + weight_decay * p : g              (grad is only read)
 *     m = m * beta1 + (1 - beta1) g';   v = v * beta2 + (1 - beta2) g'^2;   amsgrad: vmax = max(vmax, v) (NaN propagates)
 *     p = p - step_size * m / (sqrt(amsgrad ? vmax : v) + eps)
 *     block_size > 0: p = Q(p), blocks of block_size along the last dim (per-row zero pad), mant_bits, epsilon, round-half-even
 *                     (stoch == 0) or stochastic with the tensor's own seed
 * bit for bit what the loop of torch ops and the engine's quantizer compute on the same GPU: the scalars are the fp32 values of
 * the doubles given here, (1 - beta) is formed in double as in Python, step_size is the tensor's own double (lr * sqrt(bc2) / bc1
 * at its own step) and the stochastic dither is keyed by (seed, element index) as bfpq_quantize_nm keys it for that shape.
 * One launch per 64 tensors (descriptors in the kernel arguments: no device memory, no synchronisation); tensors with no elements
 * are skipped.  block_size: 0 (no snap) or a power of two 4..256 with 1 <= mant_bits <= 23 (bfpq_adam_step_list_ok); exp_win_dev:
 * bfpq_exp_window_host(BFPQ_F32) on the device.  A NULL pointer, a missing max_exp_avg_sq with amsgrad, or two arrays of one
 * tensor that overlap (p aliasing grad, exp_avg, ...) return BFPQ_E_ARG before anything is launched. */
typedef struct bfpq_adam_hparams {
    double beta1, beta2, eps, weight_decay;
    int amsgrad;
    int block_size;                 /* 0: no snap */
    int mant_bits;                  /* weight_mant_bits */
    int stoch;                      /* 0: round-half-even, else stochastic rounding with each tensor's seed */
    double epsilon;                 /* the quantizer's epsilon */
    const uint8_t* exp_win_dev;     /* BFPQ_EXP_WIN_ENTRIES for BFPQ_F32 (NULL when block_size == 0) */
} bfpq_adam_hparams;
typedef struct bfpq_adam_tensor {
    float* p_dev;
    const float* grad_dev;
    float* exp_avg_dev;
    float* exp_avg_sq_dev;
    float* max_exp_avg_sq_dev;      /* amsgrad only, else ignored */
    int64_t rows, cols;             /* dense row-major; blocks run along cols */
    double step_size;               /* lr * sqrt(1 - beta2^step) / (1 - beta1^step) at this tensor's step */
    uint64_t seed;                  /* stochastic snap: non-zero seed (as _seed_for draws it); else ignored */
} bfpq_adam_tensor;
int bfpq_adam_step_list(const bfpq_adam_hparams* hparams_host, const bfpq_adam_tensor* tensors_host, int n, void* stream);
/* 1 if bfpq_adam_step_list takes this snap configuration (block_size 0: no snap) */
int bfpq_adam_step_list_ok(int block_size, int mant_bits);

/* the first BFPQ_SELECT_STATE_BYTES of ws_dev, as read back by a host that wants tau / counts (little-endian) */
typedef struct bfpq_select_state {
    uint32_t prefix;      /* magnitude bits decided so far (high digits)                         */
    uint32_t prefix_mask; /* which bits of prefix are decided                                    */
    int64_t k_rem;        /* how many of the elements matching prefix are still to be pruned     */
    uint32_t tau;         /* after the last pass: magnitude bit pattern of the threshold         */
    uint32_t done;        /* 1 after the last pass                                               */
    int64_t need;         /* how many elements equal to tau get pruned (over all ranks)          */
    int64_t ties;         /* how many elements equal tau in total (over all ranks)               */
    int64_t k;            /* the k given to the selection                                        */
    int64_t tie_base;     /* elements equal to tau held by lower ranks                           */
    uint32_t flags;       /* bit 0: cut_* below are valid (else the apply launch derives them from the per-segment tie counts);
                             bit 1: the fine histograms inside ws_dev were used (the apply launch clears them) */
    uint32_t cut_lo;      /* this device's elements equal to tau go in lane items (16 B) [0, cut_lo), stay in [cut_hi, end), */
    uint32_t cut_hi;      /* and inside [cut_lo, cut_hi) -- one segment of the histogram launch, or empty -- the first        */
    uint32_t cut_within;  /* cut_within of them (flat order) go                                                              */
    uint32_t cut_total;   /* elements equal to tau inside [cut_lo, cut_hi)                                                   */
    uint32_t reserved;
} bfpq_select_state;

#ifdef __cplusplus
}
#endif
#endif /* BFPQ_H */
