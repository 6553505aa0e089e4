// bfpq_adam.hip -- the fused BFPAdam step (bfpq_adam_step_list): Adam's moment update, the parameter update and the HBFP snap of the
// updated parameter (bfp_optim_lstm.py:62-87 + float_to_bfp_blocked(p, sgd_update=True), bfp_ops.py:46-59) for a LIST of fp32 tensors
// in one launch per 64 tensors.  Per element: read p, grad, exp_avg, exp_avg_sq (+ max_exp_avg_sq), write p, exp_avg, exp_avg_sq
// (+ max_exp_avg_sq): 28 B (36 B) instead of the loop's ~90 B and nine launches per tensor.
//
// Bit for bit the loop on the same GPU:
//   * the moment arithmetic is torch's, including where PyTorch-ROCm's elementwise kernels contract to an FMA (measured on the
//     MI355X): add_(x, alpha=a) = fma(a, x, self); addcmul_(x, y, value=c) = fma(c, x * y, self);
//     addcdiv_(x, y, value=c) = fma(c, x / y, self); sqrt and '/' correctly rounded.  The library builds with -ffp-contract=off, so
//     every FMA below is written out and nothing else is fused;
//   * the snap is the engine's quantizer for that shape: tensors the single-pass kernel takes (cols % block == 0, p 16-byte aligned)
//     run the STREAM form -- 16 B per lane per array, 64-item waves at the same tensor offsets as k_fused_flat, the same
//     fast / step-by-step split per wave and the same dither -- and every other tensor the ROW form of k_quant_rows (one lane per
//     block of a row, the reference's per-row padding, step-by-step arithmetic, dither keyed by the flat element index).
#include "bfpq_device.h"
#include "bfpq_quant_math.h"

namespace {
using namespace bfpq_dev;

constexpr int kAdamMaxList = 64;

// one tensor of a launch (kernel argument; 60 bytes so that 64 of them and the header fit the 4 KB argument segment)
struct __attribute__((packed, aligned(4))) AdamDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* vmax;
    int64_t numel;
    int32_t cols;          // > 0: row form (rows of cols elements); 0: stream form, 16-byte accesses; -1: stream form, element accesses
    float neg_step;        // (float)(-step_size)
    uint32_t seed_key;     // (uint32)seed + (uint32)(seed >> 32): all of the seed rng_item_key reads
};
struct AdamArgs {
    int n;
    float b1, omb1, b2, omb2, eps, wd, eps_q;
    int block, lpb, mant_bits;
    const uint8_t* exp_win;
    AdamDesc d[kAdamMaxList];
};
static_assert(sizeof(AdamArgs) <= 4096, "kernel argument segment");

// chunks of a tensor: 256 lane items of 4 elements (stream form) or 256 blocks (row form)
__host__ __device__ inline int64_t adam_chunks(int64_t numel, int32_t cols, int block)
{
    if (cols > 0) {
        const int64_t nb = (numel / cols) * ((cols + block - 1) / block);
        return (nb + kThreads - 1) / kThreads;
    }
    return ((numel + 3) / 4 + kThreads - 1) / kThreads;
}

// One element of Adam (bfp_optim_lstm.py:62-85), torch's rounding.  Returns the updated (un-snapped) parameter.
template <bool AMS, bool WD>
__device__ __forceinline__ float adam_elem(const AdamArgs& a, float nstep, float p, float g, float& m, float& v, float& vm)
{
    if constexpr (WD) g = __builtin_fmaf(a.wd, p, g);                 // grad.add(p, alpha=wd)
    m = m * a.b1;                                                     // m.mul_(beta1)
    m = __builtin_fmaf(a.omb1, g, m);                                 //  .add_(grad, alpha=1 - beta1)
    v = v * a.b2;                                                     // v.mul_(beta2)
    v = __builtin_fmaf(a.omb2, g * g, v);                             //  .addcmul_(grad, grad, value=1 - beta2)
    float d;
    if constexpr (AMS) { vm = t_max(vm, v); d = __builtin_sqrtf(vm); }   // torch.max(vmax, v, out=vmax); vmax.sqrt()
    else d = __builtin_sqrtf(v);
    d = d + a.eps;                                                    // .add_(eps)
    return __builtin_fmaf(nstep, m / d, p);                           // p.addcdiv_(m, denom, value=-step_size)
}

// SNAP: 0 none, 1 round-half-even, 2 stochastic
template <bool AMS, bool WD, int SNAP>
__global__ void __launch_bounds__(kThreads) k_adam_list(const AdamArgs a)
{
    using T = Traits<BFPQ_F32>;
    __shared__ __attribute__((aligned(16))) uint8_t s_win[512];
    __shared__ uint32_t s_c0[kAdamMaxList + 1];
    const int tid = threadIdx.x;
    if constexpr (SNAP != 0)
        for (int i = tid; i < 512; i += kThreads) s_win[i] = i < BFPQ_EXP_WIN_ENTRIES ? a.exp_win[i] : 0;
    if (tid < 64) {                                                   // first chunk of every tensor: one wave scan
        const uint32_t c = tid < a.n ? (uint32_t)adam_chunks(a.d[tid].numel, a.d[tid].cols, a.block) : 0u;
        const uint32_t incl = wave_incl_scan(c);
        s_c0[tid] = incl - c;
        if (tid == 63) s_c0[kAdamMaxList] = incl;
    }
    __syncthreads();
    const uint32_t total = s_c0[kAdamMaxList];
    int t = 0;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        while (t + 1 < a.n && c >= s_c0[t + 1]) t++;                  // (workgroup-uniform; chunks only move forward)
        t = __builtin_amdgcn_readfirstlane(t);
        const AdamDesc& d = a.d[t];
        const int64_t numel = d.numel;
        const float nstep = d.neg_step;
        const int64_t unit = (int64_t)(c - s_c0[t]) * kThreads + tid;
        if (d.cols <= 0) {
            // ---- stream form: lane item `unit` = elements [4 unit, 4 unit + 4) ----
            const int64_t n_items = (numel + 3) / 4;
            const bool valid = unit < n_items;
            const int64_t item = valid ? unit : n_items - 1;          // past the end: the last item again (k_fused_flat's clamp)
            float p[4], g[4], m[4], v[4], vm[4] = {0.f, 0.f, 0.f, 0.f};
            if (d.cols == 0) {
                const float4 P = reinterpret_cast<const float4*>(d.p)[item], G = reinterpret_cast<const float4*>(d.g)[item];
                const float4 M = reinterpret_cast<const float4*>(d.m)[item], V = reinterpret_cast<const float4*>(d.v)[item];
                p[0] = P.x; p[1] = P.y; p[2] = P.z; p[3] = P.w; g[0] = G.x; g[1] = G.y; g[2] = G.z; g[3] = G.w;
                m[0] = M.x; m[1] = M.y; m[2] = M.z; m[3] = M.w; v[0] = V.x; v[1] = V.y; v[2] = V.z; v[3] = V.w;
                if constexpr (AMS) { const float4 X = reinterpret_cast<const float4*>(d.vmax)[item]; vm[0] = X.x; vm[1] = X.y; vm[2] = X.z; vm[3] = X.w; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int64_t e = item * 4 + j < numel ? item * 4 + j : numel - 1;
                    p[j] = d.p[e]; g[j] = d.g[e]; m[j] = d.m[e]; v[j] = d.v[e];
                    if constexpr (AMS) vm[j] = d.vmax[e];
                }
            }
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; j++) y[j] = adam_elem<AMS, WD>(a, nstep, p[j], g[j], m[j], v[j], vm[j]);
            if constexpr (SNAP != 0) {
                // the single-pass quantizer's per-item body for fp32 (bfpq_fused.h, k_fused_flat, drop-in output)
                uint32_t mx = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) { const uint32_t k = f2u(y[j]) & T::ABS; mx = k > mx ? k : mx; }
                mx = group_max<-1>(mx, a.lpb);
                const FastScale fs = fast_scale<BFPQ_F32>(mx, a.mant_bits, a.eps_q, s_win);
                if (__builtin_expect(__any(!fs.ok), 0)) {
                    const BlockScale bs = block_scale<BFPQ_F32>(mx, a.mant_bits, a.eps_q, s_win);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float dither = SNAP == 2 ? uniform24k(rng_item_key(d.seed_key, (uint64_t)item * 4), (uint32_t)j) - 0.5f : 0.f;
                        float code;
                        y[j] = quant_elem<BFPQ_F32>(y[j], bs, SNAP == 2, dither, &code);
                    }
                } else {
                    [[maybe_unused]] uint32_t rstate = 0u;
                    if constexpr (SNAP == 2) {
                        uint32_t x = rng_item_key(d.seed_key, (uint64_t)item * 4);
                        x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
                        rstate = x | 1u;
                    }
#pragma unroll
                    for (int j = 0; j < 4; j += 2) {
                        float t0, t1;
                        if constexpr (SNAP == 2) {
                            rstate ^= rstate << 13; rstate ^= rstate >> 17; rstate ^= rstate << 5;
                            const float u0 = u2f(0x3f800000u | ((rstate & 0xffffu) << 7)), u1 = u2f(0x3f800000u | ((rstate >> 16) << 7));
                            t0 = __builtin_fmaf(y[j], fs.inv, -1.5f) + u0;
                            t1 = __builtin_fmaf(y[j + 1], fs.inv, -1.5f) + u1;
                        } else { t0 = y[j] * fs.inv; t1 = y[j + 1] * fs.inv; }
                        y[j] = __builtin_amdgcn_fmed3f(rintf(t0), -fs.qmax, fs.qmax) * fs.interval;
                        y[j + 1] = __builtin_amdgcn_fmed3f(rintf(t1), -fs.qmax, fs.qmax) * fs.interval;
                    }
                }
            }
            if (!valid) continue;
            if (d.cols == 0) {
                reinterpret_cast<float4*>(d.p)[item] = make_float4(y[0], y[1], y[2], y[3]);
                reinterpret_cast<float4*>(d.m)[item] = make_float4(m[0], m[1], m[2], m[3]);
                reinterpret_cast<float4*>(d.v)[item] = make_float4(v[0], v[1], v[2], v[3]);
                if constexpr (AMS) reinterpret_cast<float4*>(d.vmax)[item] = make_float4(vm[0], vm[1], vm[2], vm[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int64_t e = item * 4 + j;
                    if (e >= numel) break;
                    d.p[e] = y[j]; d.m[e] = m[j]; d.v[e] = v[j];
                    if constexpr (AMS) d.vmax[e] = vm[j];
                }
            }
        } else {
            // ---- row form: `unit` = block bi of row r (k_quant_rows: the block's share of the row, zero pad cut off) ----
            const int64_t cols = d.cols, nblk = (cols + a.block - 1) / a.block;
            if (unit >= (numel / cols) * nblk) continue;
            const int64_t row = unit / nblk, c0 = (unit - row * nblk) * a.block;
            const int len = (int)(cols - c0 < a.block ? cols - c0 : a.block);
            const int64_t base = row * cols + c0;
            // pass 1: the moments (stored), and the block max of the updated parameter
            uint32_t mx = 0;
            for (int i = 0; i < len; i++) {
                const int64_t e = base + i;
                float m = d.m[e], v = d.v[e], vm = AMS ? d.vmax[e] : 0.f;
                const float y = adam_elem<AMS, WD>(a, nstep, d.p[e], d.g[e], m, v, vm);
                d.m[e] = m; d.v[e] = v;
                if constexpr (AMS) d.vmax[e] = vm;
                if constexpr (SNAP == 0) d.p[e] = y;
                else { const uint32_t k = f2u(y) & T::ABS; mx = k > mx ? k : mx; }
            }
            if constexpr (SNAP != 0) {
                // pass 2: the same update again from the stored moments (this lane's own writes), snapped
                const BlockScale bs = block_scale<BFPQ_F32>(mx, a.mant_bits, a.eps_q, s_win);
                for (int i = 0; i < len; i++) {
                    const int64_t e = base + i;
                    const float den = __builtin_sqrtf(AMS ? d.vmax[e] : d.v[e]) + a.eps;
                    const float y = __builtin_fmaf(nstep, d.m[e] / den, d.p[e]);
                    const float dither = SNAP == 2 ? uniform24(d.seed_key, (uint64_t)e) - 0.5f : 0.f;
                    float code;
                    d.p[e] = quant_elem<BFPQ_F32>(y, bs, SNAP == 2, dither, &code);
                }
            }
        }
    }
}

template <bool AMS, bool WD>
void launch_adam(const AdamArgs& a, int snap, int grid, hipStream_t s)
{
    if (snap == 0) hipLaunchKernelGGL((k_adam_list<AMS, WD, 0>), dim3(grid), dim3(kThreads), 0, s, a);
    else if (snap == 1) hipLaunchKernelGGL((k_adam_list<AMS, WD, 1>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((k_adam_list<AMS, WD, 2>), dim3(grid), dim3(kThreads), 0, s, a);
}

bool adam_snap_ok(int block_size, int mant_bits)
{
    if (block_size == 0) return true;                                 // no snap
    return block_size >= 4 && block_size <= 256 && is_pow2(block_size) && mant_bits >= 1 && mant_bits <= 23;
}

bool overlaps(const void* x, const void* y, int64_t n)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(x), b0 = reinterpret_cast<uintptr_t>(y), len = (uintptr_t)n * 4u;
    return x && y && a0 < b0 + len && b0 < a0 + len;
}
}  // namespace

extern "C" {

int bfpq_adam_step_list_ok(int block_size, int mant_bits) { return adam_snap_ok(block_size, mant_bits) ? 1 : 0; }

int bfpq_adam_step_list(const bfpq_adam_hparams* hp, const bfpq_adam_tensor* ts, int n, void* stream)
{
    if (!hp || n < 0 || (n > 0 && !ts)) return BFPQ_E_ARG;
    if (!adam_snap_ok(hp->block_size, hp->mant_bits) || (hp->block_size > 0 && !hp->exp_win_dev)) return BFPQ_E_ARG;
    const bool ams = hp->amsgrad != 0;
    // every check first: nothing is launched for a list with one bad descriptor
    for (int i = 0; i < n; i++) {
        const bfpq_adam_tensor& t = ts[i];
        if (t.rows < 0 || t.cols < 0) return BFPQ_E_ARG;
        const int64_t numel = t.rows * t.cols;
        if (numel == 0) continue;
        if (!t.p_dev || !t.grad_dev || !t.exp_avg_dev || !t.exp_avg_sq_dev || (ams && !t.max_exp_avg_sq_dev)) return BFPQ_E_ARG;
        if (t.cols > INT32_MAX || adam_chunks(numel, 0, 4) >= ((int64_t)1 << 31)) return BFPQ_E_ARG;
        const void* arr[5] = {t.p_dev, t.grad_dev, t.exp_avg_dev, t.exp_avg_sq_dev, ams ? t.max_exp_avg_sq_dev : nullptr};
        for (int x = 0; x < 5; x++)
            for (int y = x + 1; y < 5; y++)
                if (overlaps(arr[x], arr[y], numel)) return BFPQ_E_ARG;
    }
    AdamArgs a{};
    a.b1 = (float)hp->beta1; a.omb1 = (float)(1.0 - hp->beta1);
    a.b2 = (float)hp->beta2; a.omb2 = (float)(1.0 - hp->beta2);
    a.eps = (float)hp->eps; a.wd = (float)hp->weight_decay;
    const int snap = hp->block_size == 0 ? 0 : (hp->stoch ? 2 : 1);
    a.block = hp->block_size > 0 ? hp->block_size : 4;
    a.lpb = a.block / 4; a.mant_bits = hp->mant_bits; a.eps_q = (float)hp->epsilon; a.exp_win = hp->exp_win_dev;
    const bool wd = hp->weight_decay != 0;
    hipStream_t s = (hipStream_t)stream;
    int64_t chunks = 0;
    auto flush = [&]() -> int {
        if (a.n == 0) return 0;
        const int64_t cap = (int64_t)bfpq_g_max_grid * 2;
        const int grid = (int)(chunks < cap ? chunks : cap);
        if (ams) { if (wd) launch_adam<true, true>(a, snap, grid, s); else launch_adam<true, false>(a, snap, grid, s); }
        else { if (wd) launch_adam<false, true>(a, snap, grid, s); else launch_adam<false, false>(a, snap, grid, s); }
        a.n = 0; chunks = 0;
        return (int)hipGetLastError();
    };
    for (int i = 0; i < n; i++) {
        const bfpq_adam_tensor& t = ts[i];
        const int64_t numel = t.rows * t.cols;
        if (numel == 0) continue;
        AdamDesc d;
        d.p = t.p_dev; d.g = t.grad_dev; d.m = t.exp_avg_dev; d.v = t.exp_avg_sq_dev; d.vmax = ams ? t.max_exp_avg_sq_dev : nullptr;
        d.numel = numel;
        d.neg_step = (float)(-t.step_size);
        d.seed_key = (uint32_t)t.seed + (uint32_t)(t.seed >> 32);
        const bool vec = numel % 4 == 0 && aligned16(t.p_dev, t.grad_dev, t.exp_avg_dev, t.exp_avg_sq_dev) &&
                         (!ams || aligned16(t.max_exp_avg_sq_dev));
        if (snap == 0) d.cols = vec ? 0 : -1;
        else if (aligned16(t.p_dev) && t.cols % hp->block_size == 0) d.cols = vec ? 0 : -1;   // what bfpq_quantize_nm runs in one pass
        else d.cols = (int32_t)t.cols;
        const int64_t c = adam_chunks(numel, d.cols, a.block);
        if (chunks + c >= ((int64_t)1 << 32)) { const int rc = flush(); if (rc) return rc; }
        AdamDesc& d2 = a.d[a.n];                                      // (flush() may have emptied the list: re-seat)
        if (&d2 != &d) d2 = d;
        a.n++;
        chunks += c;
        if (a.n == kAdamMaxList) { const int rc = flush(); if (rc) return rc; }
    }
    return flush();
}

}  // extern "C"
