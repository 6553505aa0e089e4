"""The two GEMMs that consume the packed weight, bit for bit (run with `-m gpu` on an MI355X).

Operands are exact HBFP (tests/gemm_cases.py): codes c with |c| <= 2^m - 1, block exponents that vary over rows and blocks with
period 3.  Each case first asserts the certificate (every fp32 partial sum is exact in any order), so the fp64 product IS the
kernel's fp32 sum and the expected output is that product rounded once to the output dtype:
  * prefill (bfpq_mxgemm.hip): every tile variant, both epilogues, the mixed big/small launch with a ragged seam, split-K with
    parts that do not divide the trips, weight and activation mantissas 1..4, 4-bit and int8 weight codes, N:M weights,
    fp16 overflow, NaN blocks;
  * decode (bfpq_gemm.hip): the untiled kernel at every token count 1..16, the tiled kernel at every row-tile choice,
    PackedBFP.linear across the decode / prefill seam with bias, NaN blocks in x and W, and rows past T of the untiled operand.
"""
import ctypes

import pytest
import torch

import gemm_cases as G
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = (torch.float32, torch.bfloat16, torch.float16)
TUNE_GEMM_ROW_TILES, TUNE_MX8_VARIANT = 1, 2


def L():
    return native.load_library()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def operand(rows, K, m, e0, spread, seed, nm=(0, 0), pattern=(7, 5, 1)):
    return G.hbfp_operand(rows, K, m, e0, spread, seed, nm=nm, pattern=pattern, device=DEV)


def w_operand(N, K, wm, spread, seed, nm=(0, 0), e0=-2):
    return operand(N, K, wm, e0, spread, seed, nm=nm, pattern=(5, 7, 2))


def x_image(xc, xe, xm):
    return native.mx8_from_hbfp(xc.to(torch.int8), xe.to(torch.int8), xc.shape[1], xm, 8)


def w_image(wc, we, wm, code_bits):
    codes = G.pack4(wc) if code_bits == 4 else wc.to(torch.int8)
    return native.mx8_from_hbfp(codes, we.to(torch.int8), wc.shape[1], wm, code_bits)


def make_bias(N, xe, we, xm, wm, dt, seed):
    """integer multiples of 4 q in the output dtype (exact there), so the certificate covers the bias as well"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = 2.0 ** (int(xe.min()) + int(we.min()) - xm - wm)
    b = torch.randint(-60, 61, (N,), generator=g, device=DEV).double() * 4 * q
    assert torch.equal(b.to(dt).double(), b)
    return b.to(dt), b / q


def exact_want(xc, xe, xm, wc, we, wm, bias_over_q=None, bias=None, what=""):
    """fp64 product of the exact operands (+ bias), after asserting the certificate: exact in fp32, so .float() is lossless"""
    G.assert_exact_regime(xc, xe, xm, wc, we, wm, bias_over_q, what)
    want = G.values(xc, xe, xm) @ G.values(wc, we, wm).t()
    if bias is not None:
        want = want + bias.double()
    assert torch.equal(want.float().double(), want), what
    return want


def assert_bits(got, want, what):
    """bit-for-bit equality of two tensors of one dtype; NaN matches NaN (payload and sign of NaN are not part of the contract)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    a, b = got.contiguous().view(it), want.to(got.device).contiguous().view(it)
    ga, wa = torch.isnan(got), torch.isnan(want.to(got.device))
    bad = (ga != wa) | (~ga & (a != b))
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outputs differ; first at {idx}: got {float(got[tuple(idx)])!r} "
                             f"want {float(want[tuple(idx)])!r}")


def mx8_call(x8, xs, w8, ws, bias, out, T, N, K):
    native.check(L().bfpq_hbfp_linear_mx8(ptr(x8), ptr(xs), ptr(w8), ptr(ws), ptr(bias), ptr(out), T, N, K,
                                          native.DTYPE_CODE[out.dtype], stream()), "bfpq_hbfp_linear_mx8")


def splitk_call(x8, xs, w8, ws, bias, out, slabs, parts, T, N, K):
    native.check(L().bfpq_hbfp_linear_mx8_splitk(ptr(x8), ptr(xs), ptr(w8), ptr(ws), ptr(bias), ptr(out), ptr(slabs), parts, T, N, K,
                                                 native.DTYPE_CODE[out.dtype], stream()), "bfpq_hbfp_linear_mx8_splitk")


# ---------------------------------------------------------------------------------------------------------------- prefill

SHAPES = [(1, 1, 256), (1, 264, 4096), (31, 4, 512), (32, 8, 768), (33, 100, 1280), (127, 128, 4096), (128, 129, 256), (129, 256, 512),
          (255, 264, 768), (256, 1500, 1280), (257, 128, 256), (700, 1500, 4096), (31, 1500, 256), (128, 8, 4096), (129, 1, 768),
          (256, 4, 1280), (33, 264, 512), (255, 100, 256), (700, 129, 512), (127, 256, 768), (257, 1500, 512), (32, 129, 4096),
          (700, 8, 1280), (1, 128, 512), (256, 256, 256)]


def test_prefill_every_variant_bit_exact():
    """~25 shapes x every tile variant, both epilogues (16-byte pieces when N % 8 == 0 and out is aligned; lane by lane for a ragged N
    or an out one element into a larger buffer), bias on / off, N:M weights, every output dtype"""
    nms = [(0, 0), (2, 4), (1, 4), (4, 8)]
    try:
        for i, (T, N, K) in enumerate(SHAPES):
            dt = DTS[i % 3]
            xc, xe = operand(T, K, 3, 0, 3, seed=10 + i)
            wc, we = w_operand(N, K, 3, 3, seed=50 + i, nm=nms[i % 4])
            bias, bq = make_bias(N, xe, we, 3, 3, dt, seed=90 + i) if i % 2 else (None, None)
            want = exact_want(xc, xe, 3, wc, we, 3, bq, bias, what=f"shape {T, N, K}").float().to(dt)
            x8, xs = x_image(xc, xe, 3)
            w8, ws = w_image(wc, we, 3, 4)
            for v in range(7):
                assert L().bfpq_tune(TUNE_MX8_VARIANT, v) == 0
                out = torch.empty((T, N), dtype=dt, device=DEV)
                mx8_call(x8, xs, w8, ws, bias, out, T, N, K)
                assert_bits(out, want, f"variant {v} shape {T, N, K} {dt}")
                buf = torch.full((T * N + 2,), 3.0, dtype=dt, device=DEV)         # out one element in: the lane-by-lane epilogue
                mx8_call(x8, xs, w8, ws, bias, buf[1:1 + T * N], T, N, K)
                assert_bits(buf[1:1 + T * N].view(T, N), want, f"variant {v} shape {T, N, K} {dt}, unaligned out")
                assert float(buf[0]) == 3.0 and float(buf[-1]) == 3.0, "write outside out"
    finally:
        L().bfpq_tune(TUNE_MX8_VARIANT, -1)


def test_prefill_mixed_launch_ragged_seam():
    """variant 5 at T = 4096, N = 4100, K = 256: 16 column tiles of 256 x 256 and one 256 x 128 tile holding 4 columns"""
    T, N, K = 4096, 4100, 256
    xc, xe = operand(T, K, 3, 0, 3, seed=3)
    wc, we = w_operand(N, K, 3, 3, seed=4, nm=(2, 4))
    bias, bq = make_bias(N, xe, we, 3, 3, torch.bfloat16, seed=5)
    want = exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="mixed").float().to(torch.bfloat16)
    x8, xs = x_image(xc, xe, 3)
    w8, ws = w_image(wc, we, 3, 4)
    try:
        for v in (5, -1):
            assert L().bfpq_tune(TUNE_MX8_VARIANT, v) == 0
            out = torch.empty((T, N), dtype=torch.bfloat16, device=DEV)
            mx8_call(x8, xs, w8, ws, bias, out, T, N, K)
            assert_bits(out, want, f"variant {v}")
    finally:
        L().bfpq_tune(TUNE_MX8_VARIANT, -1)


@pytest.mark.parametrize("T,N,K", [(100, 256, 1280), (33, 136, 11008)])
def test_prefill_split_k_bit_exact(T, N, K):
    """bfpq_hbfp_linear_mx8_splitk with parts 2, 3, 5, 8, 64 (5 and 43 trips of 256: parts that do not divide the trips, more parts
    than trips), bias on and off, every output dtype"""
    xc, xe = operand(T, K, 3, 0, 3, seed=21)
    wc, we = w_operand(N, K, 3, 3, seed=22, nm=(2, 4))
    x8, xs = x_image(xc, xe, 3)
    w8, ws = w_image(wc, we, 3, 4)
    slabs = torch.empty((64, T, N), dtype=torch.float32, device=DEV)
    for dt in DTS:
        for with_bias in (False, True):
            bias, bq = make_bias(N, xe, we, 3, 3, dt, seed=23) if with_bias else (None, None)
            want = exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="split-K").float().to(dt)
            for parts in (2, 3, 5, 8, 64):
                out = torch.empty((T, N), dtype=dt, device=DEV)
                splitk_call(x8, xs, w8, ws, bias, out, slabs, parts, T, N, K)
                assert_bits(out, want, f"parts {parts} {dt} bias {with_bias}")


def test_prefill_split_k_switch_is_bit_identical():
    """hbfp_linear_mx8 from a tensor (the one-pass activation image of a fixed-point operand) with native.SPLIT_K on and off"""
    T, N, K = 100, 512, 4096
    assert L().bfpq_hbfp_linear_mx8_parts(T, N, K) > 1
    xc, xe = operand(T, K, 3, 0, 3, seed=31)
    wc, we = w_operand(N, K, 3, 3, seed=32)
    x = G.values(xc, xe, 3).to(torch.bfloat16)
    bias, bq = make_bias(N, xe, we, 3, 3, torch.bfloat16, seed=33)
    want = exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="switch").float().to(torch.bfloat16)
    w8, ws = w_image(wc, we, 3, 4)
    native.forget_shared_images()
    split = native.hbfp_linear_mx8(x, w8, ws, 3, bias=bias)
    try:
        native.SPLIT_K = False
        one = native.hbfp_linear_mx8(x, w8, ws, 3, bias=bias)
    finally:
        native.SPLIT_K = True
    assert_bits(split, want, "split")
    assert_bits(one, want, "unsplit")


def test_prefill_mantissa_widths_and_code_widths():
    """weight mantissas 1..4 (4-bit and int8 codes into mx8_from_hbfp), activation mantissas 1..4, N:M weights"""
    T, N, K = 129, 264, 768
    nms = [(0, 0), (2, 4), (1, 4), (4, 8)]
    i = 0
    for wm in (1, 2, 3, 4):
        for xm in (1, 2, 3, 4):
            i += 1
            xc, xe = operand(T, K, xm, 0, 3, seed=100 + i)
            wc, we = w_operand(N, K, wm, 3, seed=200 + i, nm=nms[i % 4])
            dt = DTS[i % 3]
            want = exact_want(xc, xe, xm, wc, we, wm, what=f"wm {wm} xm {xm}").float().to(dt)
            x8, xs = x_image(xc, xe, xm)
            for cb in ((4, 8) if wm <= 3 else (8,)):
                w8, ws = w_image(wc, we, wm, cb)
                out = torch.empty((T, N), dtype=dt, device=DEV)
                mx8_call(x8, xs, w8, ws, None, out, T, N, K)
                assert_bits(out, want, f"wm {wm} xm {xm} code_bits {cb}")


def test_fp16_overflow_is_inf_as_torch_casts_it():
    """sums beyond 65504 become +-inf exactly where torch's fp32 -> fp16 cast makes them inf: prefill (one launch and split-K) and
    both decode kernels"""
    T, N, K = 16, 256, 1280
    xc, xe = operand(T, K, 3, 6, 3, seed=41)
    wc, we = w_operand(N, K, 3, 3, seed=42, e0=4)
    want = exact_want(xc, xe, 3, wc, we, 3, what="overflow").float().to(torch.float16)
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any())
    x8, xs = x_image(xc, xe, 3)
    w8, ws = w_image(wc, we, 3, 4)
    out = torch.empty((T, N), dtype=torch.float16, device=DEV)
    mx8_call(x8, xs, w8, ws, None, out, T, N, K)
    assert_bits(out, want, "mx8")
    slabs = torch.empty((8, T, N), dtype=torch.float32, device=DEV)
    out2 = torch.empty_like(out)
    splitk_call(x8, xs, w8, ws, None, out2, slabs, 3, T, N, K)
    assert_bits(out2, want, "mx8 split-K")
    xq = (xc.to(torch.int8), xe.to(torch.int8))
    dummy = torch.empty((T, K), dtype=torch.float16, device=DEV)
    got = native.hbfp_linear_decode(dummy, G.pack4(wc), we.to(torch.int8), 3, 3, out_dtype=torch.float16, xq=xq)
    assert_bits(got, want, "decode")
    tiles, expt = native.mfma_tiles(G.pack4(wc), we.to(torch.int8))
    got = native.hbfp_linear_decode_tiled(dummy, tiles, expt, N, 3, 3, out_dtype=torch.float16, xq=xq)
    assert_bits(got, want, "decode tiled")


# ---------------------------------------------------------------------------------------------------------------- decode

def decode_spread(K, xm):
    return 2 if (K > 4096 and xm >= 6) else 3


def test_decode_untiled_every_token_count():
    """native.hbfp_linear_decode: T = 1..16, N in {16, 48, 4096}, K in {256, 768, 11008}, weight mantissas 1..3, activation mantissas
    1, 3, 5, 7, every output dtype -- the scale exponent we - wm + xe - xm pinned for every width"""
    for N in (16, 48, 4096):
        for K in (256, 768, 11008):
            for wm in (1, 2, 3):
                wc, we = w_operand(N, K, wm, 3 if K <= 4096 else 2, seed=N + K + wm)
                wcodes, wexps = G.pack4(wc), we.to(torch.int8)
                for xm in (1, 3, 5, 7):
                    xc, xe = operand(16, K, xm, 0, decode_spread(K, xm), seed=7 * K + xm)
                    want = exact_want(xc, xe, xm, wc, we, wm, what=f"N {N} K {K} wm {wm} xm {xm}").float()
                    xc8, xe8 = xc.to(torch.int8), xe.to(torch.int8)
                    for T in range(1, 17):
                        dt = DTS[(T + wm + xm) % 3]
                        dummy = torch.empty((T, K), dtype=dt, device=DEV)
                        got = native.hbfp_linear_decode(dummy, wcodes, wexps, wm, xm, out_dtype=dt, xq=(xc8[:T], xe8[:T]))
                        assert_bits(got, want[:T].to(dt), f"T {T} N {N} K {K} wm {wm} xm {xm} {dt}")


def test_decode_tiled_every_row_tile_choice():
    """native.hbfp_linear_decode_tiled at T in {1, 15, 16, 17, 33, 48, 63, 64}, K in {256, 384 (tiled only), 11008}, with every
    bfpq_tune row-tile choice 0, 1, 2, 4 (N = 48: 2 and 4 fall back to 1; N = 96: 4 falls back; N = 4096: all apply) -- the same
    exact bits from each"""
    widths = [(3, 7), (2, 3), (1, 5), (3, 1)]
    i = 0
    try:
        for K in (256, 384, 11008):
            for N in (48, 96, 4096):
                wm, xm = widths[i % 4]
                i += 1
                wc, we = w_operand(N, K, wm, 3 if K <= 4096 else 2, seed=300 + i, nm=(2, 4) if i % 2 else (0, 0))
                tiles, expt = native.mfma_tiles(G.pack4(wc), we.to(torch.int8))
                xc, xe = operand(64, K, xm, 0, decode_spread(K, xm), seed=400 + i)
                want = exact_want(xc, xe, xm, wc, we, wm, what=f"N {N} K {K}").float()
                xc8, xe8 = xc.to(torch.int8), xe.to(torch.int8)
                for T in (1, 15, 16, 17, 33, 48, 63, 64):
                    dt = DTS[(T + i) % 3]
                    dummy = torch.empty((T, K), dtype=dt, device=DEV)
                    for rt in (0, 1, 2, 4):
                        assert L().bfpq_tune(TUNE_GEMM_ROW_TILES, rt) == 0
                        got = native.hbfp_linear_decode_tiled(dummy, tiles, expt, N, wm, xm, out_dtype=dt, xq=(xc8[:T], xe8[:T]))
                        assert_bits(got, want[:T].to(dt), f"rt {rt} T {T} N {N} K {K} wm {wm} xm {xm} {dt}")
    finally:
        L().bfpq_tune(TUNE_GEMM_ROW_TILES, 0)


@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_packed_linear_across_the_decode_prefill_seam(dname):
    """PackedBFP.linear with bias at 16, 17, 64 (decode: torch adds the bias to the rounded product) and 65 tokens (prefill: the
    bias is added in fp32 before the one rounding); the quantizers reproduce the exact operands"""
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[dname]
    N, K = 256, 1280
    xc, xe = operand(65, K, 3, 0, 3, seed=51)
    wc, we = w_operand(N, K, 3, 3, seed=52, nm=(2, 4))
    x, w = G.values(xc, xe, 3).to(dt), G.values(wc, we, 3).to(dt)
    pw = bfp_ops.PackedBFP.quantize(w, 3, 64, N=2, M=4)
    assert torch.equal(pw.codes, G.pack4(wc)) and torch.equal(pw.exps, we.to(torch.int8))     # fixed points of the quantizer
    bias, bq = make_bias(N, xe, we, 3, 3, dt, seed=53)
    want = exact_want(xc, xe, 3, wc, we, 3, what="seam")
    want_b = exact_want(xc, xe, 3, wc, we, 3, bq, bias, what="seam + bias")
    native.forget_shared_images()
    for T in (16, 17, 64, 65):
        got = pw.linear(x[:T], bias, x_mant_bits=3)
        exp = want[:T].float().to(dt) + bias if T <= 64 else want_b[:T].float().to(dt)
        assert_bits(got, exp, f"T {T}")


def _nan_operands(dname, T=65, N=256, K=512):
    """exact operands in dtype with NaN blocks made the way the quantizer sees them: an inf element (any dtype) and, in fp16, an
    all-zero block (epsilon underflows); the reference product is NaN in exactly their rows / columns"""
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[dname]
    xc, xe = operand(T, K, 3, 0, 3, seed=61)
    wc, we = w_operand(N, K, 3, 3, seed=62)
    xv, wv = G.values(xc, xe, 3), G.values(wc, we, 3)
    x_nan = [(7, 200), (40, 5), (64, 300)]                                # (row, k): an inf there
    w_nan = [(9, 130), (200, 448)]
    if dt == torch.float16:
        x_nan_zero, w_nan_zero = [(2, 1)], [(5, 0)]                       # (row, block): all zeros
    else:
        x_nan_zero, w_nan_zero = [], []
    for v, nans, zeros in ((xv, x_nan, x_nan_zero), (wv, w_nan, w_nan_zero)):
        for r, k in nans:
            v[r, k] = float("inf") if k % 2 else float("-inf")
        for r, b in zeros:
            v[r, 64 * b:64 * b + 64] = 0.0
    x, w = xv.to(dt), wv.to(dt)
    # the reference's fake-quantised operands: every element of a NaN block is NaN
    for v, nans, zeros in ((xv, x_nan, x_nan_zero), (wv, w_nan, w_nan_zero)):
        for r, k in nans:
            v[r, 64 * (k // 64):64 * (k // 64) + 64] = float("nan")
        for r, b in zeros:
            v[r, 64 * b:64 * b + 64] = float("nan")
    want = xv @ wv.t()
    nan_rows = sorted({r for r, _ in x_nan + x_nan_zero})
    nan_cols = sorted({r for r, _ in w_nan + w_nan_zero})
    # outside those rows / columns the certificate holds (the NaN blocks replaced by zeros)
    xc2, wc2 = xc.clone(), wc.clone()
    xc2[nan_rows] = 0
    wc2[nan_cols] = 0
    G.assert_exact_regime(xc2, xe, 3, wc2, we, 3, what="NaN operands")
    return dt, x, w, want, nan_rows, nan_cols


@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_decode_nan_blocks_propagate(dname):
    """a NaN block (exponent byte -128) in x or in W gives NaN exactly where the reference's product is NaN, through the untiled
    and the tiled decode kernels and through PackedBFP.linear at 64 (decode) and 65 (prefill) tokens; exact values elsewhere"""
    dt, x, w, want, nan_rows, nan_cols = _nan_operands(dname)
    N, K = w.shape
    assert int(torch.isnan(want).sum()) == len(nan_rows) * N + len(nan_cols) * x.shape[0] - len(nan_rows) * len(nan_cols)
    pw = bfp_ops.PackedBFP.quantize(w, 3, 64)
    assert int((pw.exps == -128).sum()) == len(nan_cols)                 # the quantizer marks the weight's NaN blocks
    tiles, expt = native.mfma_tiles(pw.codes, pw.exps)
    for xm in (3, 7):
        for t0 in (0, 16, 48):                                          # token groups holding rows 7, 40 and 64 (each 16 rows)
            xs = x[t0:t0 + 16] if t0 < 48 else x[49:65]
            ws = want[t0:t0 + 16] if t0 < 48 else want[49:65]
            got = native.hbfp_linear_decode(xs, pw.codes, pw.exps, 3, xm, out_dtype=torch.float32)
            assert_bits(got, ws.float(), f"untiled xm {xm} rows from {t0}")
        for T in (17, 64):
            got = native.hbfp_linear_decode_tiled(x[:T], tiles, expt, N, 3, xm, out_dtype=dt)
            assert_bits(got, want[:T].float().to(dt), f"tiled xm {xm} T {T}")
        got = native.hbfp_linear_decode_tiled(x[1:65], tiles, expt, N, 3, xm, out_dtype=torch.float32)
        assert_bits(got, want[1:65].float(), f"tiled xm {xm} rows 1..64")
    native.forget_shared_images()
    for T in (64, 65):
        got = pw.linear(x[:T], x_mant_bits=3)
        assert_bits(got, want[:T].float().to(dt), f"PackedBFP.linear T {T}")
    fq = bfp_ops.float_to_bfp_blocked(x, mant_bits=3, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64,
                                      num_format='bfp', weight_mant_bits=15, in_sparsity=False, w_sparsity=False, grad_sparsity=False,
                                      sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s', sparsity_mode='structured',
                                      identifier='in')
    assert torch.isnan(fq).any(1).nonzero().flatten().tolist() == nan_rows         # (the reference's operand: the same NaN rows)


def test_decode_rows_past_t_cannot_leak():
    """rows >= T of the untiled kernel's 16-row operand are never read back: a -128 exponent byte (NaN block marker) and garbage codes
    there leave rows < T exact -- given explicitly through the C entry point, and through the wrapper after the caching allocator
    was handed a block full of 0x80 bytes"""
    N, K, T = 48, 768, 5
    xc, xe = operand(16, K, 3, 0, 3, seed=71)
    wc, we = w_operand(N, K, 3, 3, seed=72)
    want = exact_want(xc, xe, 3, wc, we, 3, what="rows past T").float()
    wcodes, wexps = G.pack4(wc), we.to(torch.int8)
    xc16 = torch.randint(-128, 128, (16, K), device=DEV, dtype=torch.int32).to(torch.int8)
    xe16 = torch.full((16, K // 64), -128, dtype=torch.int8, device=DEV)
    xc16[:T] = xc[:T].to(torch.int8)
    xe16[:T] = xe[:T].to(torch.int8)
    slabs = torch.empty((L().bfpq_hbfp_linear_slices(N, K), 16, N), dtype=torch.float32, device=DEV)
    out = torch.empty((T, N), dtype=torch.float32, device=DEV)
    native.check(L().bfpq_hbfp_linear_decode(ptr(wcodes), ptr(wexps), ptr(xc16), ptr(xe16), ptr(out), ptr(slabs), T, N, K,
                                             native.DTYPE_CODE[torch.float32], 3, 3, stream()), "bfpq_hbfp_linear_decode")
    assert_bits(out, want[:T], "explicit -128 rows")
    junk = torch.full((16, K // 64), -128, dtype=torch.int8, device=DEV)
    junk2 = torch.full((16, K), -128, dtype=torch.int8, device=DEV)
    del junk, junk2
    dummy = torch.empty((T, K), dtype=torch.float32, device=DEV)
    got = native.hbfp_linear_decode(dummy, wcodes, wexps, 3, 3, out_dtype=torch.float32, xq=(xc[:T].to(torch.int8), xe[:T].to(torch.int8)))
    assert_bits(got, want[:T], "recycled 0x80 block")
