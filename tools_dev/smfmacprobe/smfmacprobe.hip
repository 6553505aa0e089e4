// Layout probe for v_smfmac_i32_16x16x64_i8 (development tool, as tools_dev/mxprobe): one wave per case, one-hot register images
// built on the host, the lane maps read off the results and checked against the map bfpq_sp24.hip assumes.  Then the issue cycles of
// back-to-back instructions on one SIMD (s_memtime ticks = shader cycles), next to the dense v_mfma_i32_16x16x64_i8.
//
// Every case uses valid index words only: in each half-word, per group of 4 K two distinct ascending positions.
//   hipcc --offload-arch=gfx950 -O2 -o smfmacprobe smfmacprobe.hip && ./smfmacprobe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template <int ABID>
__global__ void k_probe(const v2i* A, const v4i* B, const int* I, v4i* D)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const v4i z = {0, 0, 0, 0};
    D[i] = __builtin_amdgcn_smfmac_i32_16x16x64_i8(A[i], B[i], z, I[i], 0, ABID);
}

// back-to-back issue: 8 independent accumulators, `iters` x 8 instructions; one wave per SIMD (4 waves per workgroup)
template <bool SPARSE>
__global__ void __launch_bounds__(256) k_rate(const v4i* seed, v4i* out, long long* ticks, int iters)
{
    const int l = threadIdx.x;
    const v4i b = seed[l & 63];
    const v2i a = {b.x, b.y};
    const int idx = 0x44444444;                       // positions (0, 1) in every group
    v4i acc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = v4i{j, 0, 0, 0};
    const long long t0 = clock64();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if constexpr (SPARSE) acc[j] = __builtin_amdgcn_smfmac_i32_16x16x64_i8(a, b, acc[j], idx, 0, 0);
            else acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, b, acc[j], 0, 0, 0);
        }
    }
    v4i s = acc[0];
#pragma unroll
    for (int j = 1; j < 8; j++) s += acc[j];
    const long long t1 = clock64();
    out[blockIdx.x * 256 + l] = s;
    if ((l & 63) == 0) ticks[blockIdx.x * 4 + (l >> 6)] = t1 - t0;
}

struct Case { int8_t a[64][8]; int8_t b[64][16]; uint32_t idx[64]; int L, j, pat, bmode; };

// index half-word of pattern s: group g of the lane uses position pair PAIRS[(s + g) % 6]
static const int PAIRS[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
static uint32_t half(int s)
{
    uint32_t h = 0;
    for (int g = 0; g < 4; g++) {
        const int* p = PAIRS[(s + g) % 6];
        h |= (uint32_t)(p[0] | (p[1] << 2)) << (4 * g);
    }
    return h;
}

static int maps(int abid)
{
    std::vector<Case> cs;
    for (int pat = 0; pat < 6; pat++)
        for (int L = 0; L < 64; L++)
            for (int j = 0; j < 8; j++)
                for (int bmode = 0; bmode < 2; bmode++) {
                    Case c;
                    memset(&c, 0, sizeof c);
                    c.L = L, c.j = j, c.pat = pat, c.bmode = bmode;
                    c.a[L][j] = 1;
                    for (int l = 0; l < 64; l++) {
                        // the selected half holds pattern pat, the other one pattern pat + 3 (also valid, different)
                        const uint32_t sel = half(pat), other = half(pat + 3);
                        c.idx[l] = abid == 0 ? (sel | (other << 16)) : (other | (sel << 16));
                        for (int k = 0; k < 16; k++) c.b[l][k] = (int8_t)(bmode == 0 ? 1 + 16 * (l >> 4) + k : 1 + (l & 15));
                    }
                    cs.push_back(c);
                }
    const size_t n = cs.size();
    std::vector<int8_t> A(n * 64 * 8), B(n * 64 * 16);
    std::vector<uint32_t> I(n * 64);
    for (size_t w = 0; w < n; w++) {
        memcpy(&A[w * 512], cs[w].a, 512); memcpy(&B[w * 1024], cs[w].b, 1024); memcpy(&I[w * 64], cs[w].idx, 256);
    }
    void *dA, *dB, *dI, *dD;
    CK(hipMalloc(&dA, A.size())); CK(hipMalloc(&dB, B.size())); CK(hipMalloc(&dI, I.size() * 4)); CK(hipMalloc(&dD, n * 64 * 16));
    CK(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dI, I.data(), I.size() * 4, hipMemcpyHostToDevice));
    if (abid == 0) k_probe<0><<<n, 64>>>((v2i*)dA, (v4i*)dB, (int*)dI, (v4i*)dD);
    else k_probe<1><<<n, 64>>>((v2i*)dA, (v4i*)dB, (int*)dI, (v4i*)dD);
    CK(hipDeviceSynchronize());
    std::vector<int32_t> D(n * 64 * 4);
    CK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dI)); CK(hipFree(dD));
    // expected: A lane L = row L & 15, value j = group j >> 1 of K 16 (L >> 4) .. +15, its position the 2-bit field j of the selected
    // half-word; B lane l = column l & 15, bytes k = 16 (l >> 4) .. +15; D lane l, register i = row 4 (l >> 4) + i, column l & 15
    long bad = 0;
    for (size_t w = 0; w < n; w++) {
        const Case& c = cs[w];
        const int row = c.L & 15, g = c.j >> 1;
        const int pos = PAIRS[(c.pat + g) % 6][c.j & 1];
        const int kb = 16 * (c.L >> 4) + 4 * g + pos;             // the K this value multiplies
        for (int l = 0; l < 64; l++)
            for (int i = 0; i < 4; i++) {
                const int drow = 4 * (l >> 4) + i, dcol = l & 15;
                const int want = drow != row ? 0 : (c.bmode == 0 ? 1 + kb : 1 + dcol);
                const int got = D[(w * 64 + l) * 4 + i];
                if (got != want && bad++ < 8)
                    printf("abid %d: A lane %d value %d pattern %d bmode %d: D lane %d reg %d = %d, expected %d\n", abid, c.L, c.j, c.pat,
                           c.bmode, l, i, got, want);
            }
    }
    printf("abid %d: %zu cases, %ld mismatches against the expected map\n", abid, n, bad);
    return bad != 0;
}

static int rate()
{
    const int iters = 4096, wgs = 1;
    std::vector<int32_t> seed(64 * 4);
    for (size_t i = 0; i < seed.size(); i++) seed[i] = (int32_t)(0x01010101u * (uint32_t)(i % 7 + 1));
    void *ds, *dout, *dt;
    CK(hipMalloc(&ds, seed.size() * 4)); CK(hipMalloc(&dout, wgs * 256 * 16)); CK(hipMalloc(&dt, wgs * 4 * 8));
    CK(hipMemcpy(ds, seed.data(), seed.size() * 4, hipMemcpyHostToDevice));
    for (int sparse = 0; sparse < 2; sparse++) {
        for (int rep = 0; rep < 3; rep++) {
            if (sparse) k_rate<true><<<wgs, 256>>>((v4i*)ds, (v4i*)dout, (long long*)dt, iters);
            else k_rate<false><<<wgs, 256>>>((v4i*)ds, (v4i*)dout, (long long*)dt, iters);
            CK(hipDeviceSynchronize());
        }
        long long t[4];
        CK(hipMemcpy(t, dt, sizeof t, hipMemcpyDeviceToHost));
        printf("%s: %.2f cycles per instruction (4 waves, one per SIMD; per wave %lld %lld %lld %lld ticks for %d)\n",
               sparse ? "v_smfmac_i32_16x16x64_i8" : "v_mfma_i32_16x16x64_i8 ", (double)t[0] / (8.0 * iters), t[0], t[1], t[2], t[3], 8 * iters);
    }
    CK(hipFree(ds)); CK(hipFree(dout)); CK(hipFree(dt));
    return 0;
}

int main()
{
    int rc = maps(0);
    rc |= maps(1);
    return rc | rate();
}
