"""GPU tests of the batched int8 matrix-unit route of F_matmul_bfp (csrc/bfpq_bmm.hip): the transposed quantizer against the oracle, the
batched GEMM bit for bit on exact operands (tests/gemm_cases.py), fixture G11's matmul and both GPT-2 attention matmuls on random data
against the fake route's operands through the fp32 summation bound."""
import pytest
import torch

import gemm_cases as GC
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import DT, load, from_bits, bits, assert_bits_equal
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ('fp32', 'bf16', 'fp16')


def cfg(**kw):
    base = dict(mant_bits=7, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def _unsigned_zeros(t):
    """an integer code has no sign of zero; the fake-quantised tensor keeps the reference's -0.0"""
    return torch.where(t == 0, torch.zeros_like(t), t)


# ---- the transposed quantizer ---------------------------------------------------------------------------------------------------------
def _decode_t(codes, exps, S, dtype, block, m):
    """codes [B, D, ldk] + exponents [B, D, S/block] -> the [B, D, S] tensor they stand for (native.dequantize)"""
    B, D, ldk = codes.shape
    c = codes.view(B * D, ldk)[:, :S].contiguous()
    return native.dequantize(c, exps.view(B * D, S // block), S, dtype, block, m, 8).view(B, D, S)


def _check_transposed(v, block, m, what):
    B, S, D = v.shape
    codes, exps = native.codes_transposed(v.to(DEV), block, m, 1e-8)
    assert codes.shape == (B, D, native.code_pitch(S)) and exps.shape == (B, D, S // block)
    assert not bool(codes[:, :, S:].any()), f"{what}: non-zero codes in the pad"
    got = _decode_t(codes, exps, S, v.dtype, block, m).cpu()
    want = O.float_to_bfp_blocked(v.transpose(-1, -2).contiguous(), **cfg(mant_bits=m, block_size=block), identifier='w')
    assert_bits_equal(bits(_unsigned_zeros(got)), bits(_unsigned_zeros(want)), v.dtype, what)


@pytest.mark.parametrize("m", (1, 3, 7))
@pytest.mark.parametrize("block", (16, 32, 64))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_transposed_quantizer_matches_the_oracle(dtype, block, m):
    g = torch.Generator().manual_seed(100 * block + m)
    for B, S, D in ((1, 64, 64), (24, 192, 128), (2, 1024, 64), (1, 192, 128)):
        # magnitudes over many binades, so that blocks of one column differ in exponent
        v = (torch.randn(B, S, D, generator=g) * torch.exp2(torch.randint(-6, 4, (B, S, 1), generator=g).float())).to(dtype)
        _check_transposed(v, block, m, f"{dtype} block {block} m {m} [{B},{S},{D}]")
    v = torch.randn(2, 192, 64, generator=g).to(dtype)
    v[0, 64:128, 5] = 0                                   # an all-zero block at every block size
    v[1, 16:32, :] = 0
    _check_transposed(v, block, m, "all-zero blocks")
    v = torch.randn(2, 192, 64, generator=g).to(dtype)
    v[1, 70, 9] = float('nan')
    v[0, 3, 0] = float('inf')
    _check_transposed(v, block, m, "NaN / inf blocks")
    if block == 16:                                       # S % 64 != 0: the kernel writes the zero pad itself
        _check_transposed(torch.randn(3, 48, 32, generator=g).to(dtype), block, m, "S = 48")


# ---- the batched GEMM, bit for bit on exact operands ---------------------------------------------------------------------------------
def _operands(B, rows, K, m, e0, spread, seed, block):
    cs, es = zip(*(GC.hbfp_operand(rows, K, m, e0, spread, seed + 17 * b, pattern=(7 + b, 5 + 2 * b, 1 + b), block=block) for b in range(B)))
    return torch.stack(cs), torch.stack(es)


def _run_exact(B, T, N, K, block, m, spread, out_dtype, seed, nan=False, e0=-3):
    xc, xe = _operands(B, T, K, m, e0, spread, seed, block)
    wc, we = _operands(B, N, K, m, e0 - 1, spread, seed + 1000, block)
    for b in range(B):
        q, worst = GC.exact_certificate(xc[b], xe[b], m, wc[b], we[b], m, block=block)
        assert worst < 2.0 ** 24, f"batch {b}: operands leave the exact fp32 regime ({worst:.4g} >= 2^24)"
    want = torch.stack([GC.values(xc[b], xe[b], m, block=block) @ GC.values(wc[b], we[b], m, block=block).t() for b in range(B)])
    want = want.to(torch.float32).to(out_dtype)                # (exact in fp32 by the certificate: one rounding)
    if nan:                                                    # the NaN block marker on either side
        bt, bn = B - 1, 0
        xe[bt, T // 2, (K // block) - 1] = -128
        we[bn, N - 1, 0] = -128
        want[bt, T // 2, :] = float('nan')
        want[bn, :, N - 1] = float('nan')
    dev = lambda t, n: t.to(torch.int8).view(B * n, -1).to(DEV)
    got = native.hbfp_bmm_i8((dev(xc, T), dev(xe, T)), (dev(wc, N), dev(we, N)), B, T, N, K, m, m, block_size=block, out_dtype=out_dtype)
    assert got.shape == (B, T, N) and got.dtype == out_dtype
    assert_bits_equal(bits(got), bits(want), out_dtype, f"B={B} T={T} N={N} K={K} block {block} m {m} {out_dtype}")


@pytest.mark.parametrize("out_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("block", (16, 32, 64))
def test_bmm_exact_qk_family(block, out_dtype):
    """K = head_dim: one or two 64-byte chunks, T not a multiple of any tile"""
    _run_exact(3, 200, 192, 64, block, 7, 2, out_dtype, 11)
    _run_exact(2, 77, 80, 128, block, 7, 2, out_dtype, 12)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("block", (16, 32, 64))
def test_bmm_exact_pv_family(block, out_dtype):
    """N = head_dim, K in the thousands (m <= 3, or spread 1 at m = 7: the certificate decides)"""
    _run_exact(3, 77, 64, 1024, block, 3, 3, out_dtype, 21)
    _run_exact(2, 130, 128, 1088, block, 7, 1, out_dtype, 22)


@pytest.mark.parametrize("block", (16, 32, 64))
def test_bmm_exact_edges(block):
    _run_exact(1, 1, 16, 64, block, 7, 2, torch.float32, 31)                     # T = 1, B = 1
    _run_exact(1, 1, 64, 2048, block, 3, 3, torch.bfloat16, 32)
    _run_exact(5, 16, 16, 32 if block < 64 else 64, block, 7, 2, torch.float32, 33)    # K = 32: half a chunk of pad
    _run_exact(2, 50, 48, 96 if block < 64 else 192, block, 5, 3, torch.float16, 34)   # K % 64 != 0 at the small blocks
    _run_exact(3, 100, 96, 256, block, 4, 3, torch.float32, 35, nan=True)
    _run_exact(2, 33, 64, 64, block, 7, 2, torch.bfloat16, 36, nan=True)


@pytest.mark.parametrize("block", (16, 32, 64))
def test_bmm_exact_wide_token_tiles(block):
    """problems with enough tiles for the 64- and 32-token waves (the launch picks the tile from the tile count)"""
    _run_exact(24, 1400, 256, 64, block, 7, 2, torch.bfloat16, 41)
    _run_exact(24, 1400, 128, 64, block, 7, 2, torch.float32, 42)


# ---- fixture G11 -------------------------------------------------------------------------------------------------------------------------
KW = dict(mant_bits=7, block_size=16, N=1, M=4, w_sparsity=True, sparsity_mode='structured')


def _tol(dt):
    return dict(rtol=2e-2, atol=2e-2) if dt == torch.bfloat16 else dict(rtol=1e-4, atol=1e-5)      # the G8 tolerances of test_wrappers_gpu.py


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_g11_f_matmul_bfp_on_the_int8_unit(dname, monkeypatch):
    """[2,4,16,32] @ [2,4,32,16], block 16, HBFP8, 1:4 on the second operand: K = 32 is half a chunk, the second operand takes the
    transposed copy + act_codes"""
    monkeypatch.setattr(bfp_ops, 'MATMUL_I8_MIN', {key: 1 for key in bfp_ops.MATMUL_I8_MIN})      # (block 16 is off by default: it measured slower)
    g = load("g11_wrappers.npz")
    dt = DT[dname]
    kw = cfg(**KW)
    a = from_bits(g[f"mm_a_{dname}"], dt).view(2, 4, 16, 32).to(DEV)
    b = from_bits(g[f"mm_b_{dname}"], dt).view(2, 4, 32, 16).to(DEV)
    aq = from_bits(g[f"mm_aq_{dname}"], dt).view(2, 4, 16, 32)
    bq = from_bits(g[f"mm_bq_{dname}"], dt).view(2, 4, 32, 16)
    seen = []
    real = native.hbfp_bmm_i8
    monkeypatch.setattr(native, 'hbfp_bmm_i8', lambda xq, wq, *args, **kwargs: (seen.append((xq, wq)), real(xq, wq, *args, **kwargs))[1])
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
    with torch.no_grad():
        y = mm(a, b)
    assert mm.matmul_stats.i8_calls == 1 and mm.matmul_stats.fake_calls == 0 and len(seen) == 1
    assert y.shape == (2, 4, 16, 16) and y.dtype == dt
    (xc, xe), (wc, we) = seen[0]
    got_a = native.dequantize(xc, xe, 32, dt, 16, 7, 8).view(2, 4, 16, 32).cpu()
    got_b = native.dequantize(wc, we, 32, dt, 16, 7, 8).view(2, 4, 16, 32).transpose(-1, -2).contiguous().cpu()
    assert_bits_equal(bits(_unsigned_zeros(got_a)), bits(_unsigned_zeros(aq)), dt, "G11 first operand")
    assert_bits_equal(bits(_unsigned_zeros(got_b)), bits(_unsigned_zeros(bq)), dt, "G11 second operand")
    want = aq.double() @ bq.double()
    GC.elementwise_bound(y.cpu(), want, aq.double().abs() @ bq.double().abs(), 2, dt)
    torch.testing.assert_close(y.cpu().float(), from_bits(g[f"mm_y_{dname}"], dt).view(2, 4, 16, 16).float(), **_tol(dt))


# ---- both GPT-2 matmuls on random data -----------------------------------------------------------------------------------------------
PRUNING = {
    'dense': {},
    'nm_x': dict(in_sparsity=True, sparsity_mode='structured', N=2, M=4),
    'nm_w': dict(w_sparsity=True, sparsity_mode='structured', N=2, M=4),
    'unstructured_x': dict(in_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5),
}


def _against_fake_operands(mm, x, w, kw, K, block, dt):
    with torch.no_grad():
        y = mm(x, w)
        xq, wq = bfp_ops.MxM_pre_processing(x, w, True, **kw)
    xq, wq = xq.double(), wq.double()
    want = xq @ wq
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(y).all())        # no output is left out of the comparison
    GC.elementwise_bound(y, want, xq.abs() @ wq.abs(), K // block, dt)
    return y


@pytest.mark.parametrize("pruning", sorted(PRUNING))
@pytest.mark.parametrize("block,m", ((64, 7), (64, 3), (16, 7)))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
def test_attention_matmuls_against_the_fake_operands(dtype, block, m, pruning, monkeypatch):
    monkeypatch.setattr(bfp_ops, 'MATMUL_I8_MIN', {key: 1 for key in bfp_ops.MATMUL_I8_MIN})      # every default floor off
    g = torch.Generator().manual_seed(7)
    q, k, v = ((torch.randn(2, 12, 256, 64, generator=g) * s).to(dtype).to(DEV) for s in (1.0, 1.0, 0.5))
    kw = cfg(mant_bits=m, block_size=block, **PRUNING[pruning])
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
    scores = _against_fake_operands(mm, q, k.transpose(-1, -2), kw, 64, block, dtype)
    causal = torch.ones(256, 256, dtype=torch.bool, device=DEV).tril()
    p = torch.softmax((scores.float() / 8.0).masked_fill(~causal, float('-inf')), dim=-1).to(dtype)
    out = _against_fake_operands(mm, p, v, kw, 256, block, dtype)
    assert out.shape == (2, 12, 256, 64)
    assert mm.matmul_stats.i8_calls == 2 and mm.matmul_stats.fake_calls == 0
