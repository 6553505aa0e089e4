"""GPU tests of the HBFP KV cache (csrc/bfpq_kvcache.hip, bfp_ops.HBFPKVCache): the cached codes against the oracle on the concatenation
after every append, the open block re-rounded from original values, both products bit for bit on exact operands (tests/gemm_cases.py),
against the fake route's operands on random data, a greedy decode, and the refusals."""
import math

import pytest
import torch

import gemm_cases as GC
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import bits, assert_bits_equal
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


def _uz(t):
    """an integer code has no sign of zero; the fake-quantised tensor keeps the reference's -0.0"""
    return torch.where(t == 0, torch.zeros_like(t), t)


def _check_contents(cache, k_all, v_all, kw, what):
    """keys() / values() against the oracle on everything appended so far; zero codes from S to the end of the open block"""
    S, blk, dt = cache.length, cache.block, cache.dtype
    assert k_all.shape[2] == S
    want_k = O.float_to_bfp_blocked(k_all, **kw, identifier='w')
    want_v = O.float_to_bfp_blocked(v_all.transpose(-1, -2).contiguous(), **kw, identifier='w').transpose(-1, -2)
    with torch.no_grad():
        got_k, got_v = cache.keys().cpu(), cache.values().cpu()
    assert got_k.shape == k_all.shape and got_v.shape == v_all.shape
    assert_bits_equal(bits(_uz(got_k)), bits(_uz(want_k)), dt, f"{what}: keys at S = {S}")
    assert_bits_equal(bits(_uz(got_v)), bits(_uz(want_v.contiguous())), dt, f"{what}: values at S = {S}")
    end = (S + blk - 1) // blk * blk
    assert not bool(cache.v_codes[..., S:end].any()), f"{what}: non-zero codes behind S = {S} in the open block"


# 63, 64, 65, 70 (S % 16 != 0), 128, 129 are visited; the 70 starts mid-block, spans blocks and ends mid-block at every block size
SCHEDULE = (63, 1, 1, 5, 58, 1, 70, 1, 1, 55)


@pytest.mark.parametrize("m", (3, 7))
@pytest.mark.parametrize("block", (16, 32, 64))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_contents_match_the_oracle_after_every_append(dtype, block, m):
    kw = cfg(mant_bits=m, block_size=block)
    for B, H, D in ((2, 3, 64), (1, 2, 128)):
        g = torch.Generator().manual_seed(1000 * block + 10 * m + D)
        # magnitudes over many binades along the tokens, so that the open block's exponent keeps changing
        k = (torch.randn(B, H, 256, D, generator=g) * torch.exp2(torch.randint(-6, 4, (B, H, 256, 1), generator=g).float())).to(dtype)
        v = (torch.randn(B, H, 256, D, generator=g) * torch.exp2(torch.randint(-6, 4, (B, H, 256, 1), generator=g).float())).to(dtype)
        cache = bfp_ops.HBFPKVCache(B, H, D, 256, dtype=dtype, **kw)
        pos = 0
        with torch.no_grad():
            for t in SCHEDULE:
                assert cache.append(k[:, :, pos:pos + t].to(DEV), v[:, :, pos:pos + t].to(DEV)) == pos + t
                pos += t
                _check_contents(cache, k[:, :, :pos], v[:, :, :pos], kw, f"{dtype} block {block} m {m} D {D}")
            assert pos == 256
            cache.reset()
            assert cache.length == 0
            cache.append(k[:, :, 100:117].to(DEV), v[:, :, 100:117].to(DEV))                # nothing of the first fill shows
            _check_contents(cache, k[:, :, 100:117], v[:, :, 100:117], kw, "after reset")


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
def test_open_block_is_rounded_from_the_original_values(dtype):
    """token 100 of one head is 2^5 times larger than tokens 64..99: the block's exponent rises after 36 tokens were already coded"""
    block, m, D = 64, 3, 64
    kw = cfg(mant_bits=m, block_size=block)
    g = torch.Generator().manual_seed(5)
    k = torch.randn(1, 2, 192, D, generator=g).to(dtype)
    v = torch.randn(1, 2, 192, D, generator=g).to(dtype)
    v[0, 1, 100] *= 32.0
    v[0, 0, 101, 7] = float('nan')
    v[0, 1, 102, 9] = float('inf')
    v[0, :, 128:] = 0                                                # an all-zero block
    # on the CPU: rounding tokens 64..99 first and then the 37 tokens from those values is NOT the rounding of the 37 originals
    q = lambda t: O.float_to_bfp_blocked(t.transpose(-1, -2).contiguous(), **kw, identifier='w').transpose(-1, -2)
    once = q(v[0, 1, 64:101])
    twice = q(torch.cat([q(v[0, 1, 64:100]), v[0, 1, 100:101]]))
    assert not torch.equal(once, twice), "the chosen values do not tell a double rounding apart"
    cache = bfp_ops.HBFPKVCache(1, 2, D, 192, dtype=dtype, **kw)
    pos = 0
    with torch.no_grad():
        for t in (64, 36, 1, 1, 1, 25, 10, 54):
            cache.append(k[:, :, pos:pos + t].to(DEV), v[:, :, pos:pos + t].to(DEV))
            pos += t
            _check_contents(cache, k[:, :, :pos], v[:, :, :pos], kw, f"open block {dtype}")
    assert pos == 192


# ---- both products, bit for bit on exact operands -------------------------------------------------------------------------------------
def _operand(B, rows, K, m, e0, spread, seed, block, valid=None, anchor=False):
    """B exact HBFP operands [rows, K] (GC.hbfp_operand), the codes from `valid` on zeroed; codes, exponents, fp64 values.  A block cut
    short keeps a code of magnitude 2^m - 1 in its first column (anchor: every 16th column has one, for any cut), so that its exponent
    stays e_rb and the values stay fixed points of the quantizer (a block maximum that is a power of two is not one in a 16-bit dtype)."""
    cs, es = zip(*(GC.hbfp_operand(rows, K, m, e0, spread, seed + 17 * b, pattern=(7 + b, 5 + 2 * b, 1 + b), block=block) for b in range(B)))
    c, e = torch.stack(cs), torch.stack(es)
    if anchor:
        c[:, :, ::16] = (1 << m) - 1
    if valid is not None:
        c[:, :, valid:] = 0
        if valid % block:
            c[:, :, valid // block * block] = (1 << m) - 1
    return c, e, torch.stack([GC.values(c[b], e[b], m, block=block) for b in range(B)])


def _assert_fixed_point(x, kw, ident, what):
    """quantizing the operand is the identity (so the cache and the in-kernel quantizer must reproduce it)"""
    qx = O.float_to_bfp_blocked(x, **kw, identifier=ident)
    assert_bits_equal(bits(_uz(qx)), bits(_uz(x)), x.dtype, what)


def _want(xv, wv, xc, xe, wc, we, m, block, dtype):
    for b in range(xv.shape[0]):
        _, worst = GC.exact_certificate(xc[b], xe[b], m, wc[b], we[b], m, block=block)
        assert worst < 2.0 ** 24, f"operands leave the exact fp32 regime ({worst:.4g} >= 2^24)"
    return (xv @ wv.transpose(-1, -2)).to(torch.float32).to(dtype)        # exact in fp32 by the certificate: one rounding


LENGTHS = (1, 63, 64, 65, 200)


@pytest.mark.parametrize("block", (16, 32, 64))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scores_and_context_exact(dtype, block):
    B, H, m = 1, 2, 5
    kw = cfg(mant_bits=m, block_size=block)
    Smax = LENGTHS[-1]
    Sp = (Smax + block - 1) // block * block
    for D in (64, 128):
        kc, ke, kv = _operand(H, Smax, D, m, -3, 2, 11 + D, block)                    # keys [S, D], blocks along D
        vc, ve, vv = _operand(H, D, Sp, m, -4, 2, 23 + D, block, anchor=True)                   # V^T [D, S], blocks along the tokens
        k_all = kv.to(dtype).view(B, H, Smax, D)
        v_all = vv.to(dtype).view(B, H, D, Sp).transpose(-1, -2)
        assert torch.equal(k_all.double().view(H, Smax, D), kv)                       # representable in the dtype
        cache = bfp_ops.HBFPKVCache(B, H, D, Smax, dtype=dtype, **kw)
        pos = 0
        for S in LENGTHS:
            with torch.no_grad():
                cache.append(k_all[:, :, pos:S].to(DEV), v_all[:, :, pos:S].contiguous().to(DEV))
            pos = S
            Sb = (S + block - 1) // block * block
            vcs, ves, vvs = vc[:, :, :Sb].clone(), ve[:, :, :Sb // block], vv[:, :, :S]
            vcs[:, :, S:] = 0
            _assert_fixed_point(k_all[:, :, :S].contiguous(), kw, 'w', "keys are fixed points")
            _assert_fixed_point(v_all[:, :, :S].transpose(-1, -2).contiguous(), kw, 'w', "values are fixed points")
            for Tq in (1, 5, 16, 40):
                qc, qe, qv = _operand(H, Tq, D, m, -2, 2, 31 + Tq + S, block)
                pc, pe, pv = _operand(H, Tq, Sb, m, -5, 2, 47 + Tq + S, block, valid=S)
                q, p = qv.to(dtype).view(B, H, Tq, D), pv[:, :, :S].to(dtype).view(B, H, Tq, S)
                _assert_fixed_point(q, kw, 'in', "q is a fixed point")
                _assert_fixed_point(p.contiguous(), kw, 'in', "p is a fixed point")
                want_s = _want(qv, kv[:, :S], qc, qe, kc[:, :S], ke[:, :S], m, block, dtype)
                want_c = _want(pv[:, :, :S], vvs, pc, pe, vcs, ves, m, block, dtype)
                with torch.no_grad():
                    got_s, got_c = cache.scores(q.to(DEV)), cache.context(p.to(DEV))
                what = f"{dtype} block {block} D {D} S {S} Tq {Tq}"
                assert got_s.shape == (B, H, Tq, S) and got_c.shape == (B, H, Tq, D) and got_s.dtype == dtype and got_c.dtype == dtype
                assert_bits_equal(bits(got_s), bits(want_s), dtype, "scores " + what)
                assert_bits_equal(bits(got_c), bits(want_c), dtype, "context " + what)


@pytest.mark.parametrize("Tq", (5, 40))
@pytest.mark.parametrize("block", (16, 64))
def test_nan_blocks_on_either_side(block, Tq):
    """a NaN in x makes its block's scale NaN (the whole row); a -128 exponent in the cache makes that key's / column's block NaN"""
    B, H, D, S, m, dtype = 1, 2, 64, 100, 5, torch.float32
    kw = cfg(mant_bits=m, block_size=block)
    _, _, kv = _operand(H, S, D, m, -3, 2, 3, block)
    _, _, vv = _operand(H, D, 128, m, -4, 2, 4, block, valid=S)
    _, _, qv = _operand(H, Tq, D, m, -2, 2, 5, block)
    _, _, pv = _operand(H, Tq, 128, m, -5, 2, 6, block, valid=S)
    cache = bfp_ops.HBFPKVCache(B, H, D, 128, dtype=dtype, **kw)
    q, p = qv.float().view(B, H, Tq, D).clone(), pv[:, :, :S].float().view(B, H, Tq, S).clone()
    want_s = (qv @ kv.transpose(-1, -2)).float().view(B, H, Tq, S)
    want_c = (pv[:, :, :S] @ vv[:, :, :S].transpose(-1, -2)).float().view(B, H, Tq, D)
    q[0, 1, 3, 40] = float('nan')
    p[0, 0, 2, 99] = float('nan')                                     # in the ragged last block
    want_s[0, 1, 3, :] = float('nan')
    want_c[0, 0, 2, :] = float('nan')
    with torch.no_grad():
        cache.append(kv.float().view(B, H, S, D).to(DEV), vv[:, :, :S].float().view(B, H, D, S).transpose(-1, -2).contiguous().to(DEV))
        cache.k_exps[0, 0, 77, 0] = -128
        cache.v_exps[0, 1, 9, 1] = -128
        want_s[0, 0, :, 77] = float('nan')
        want_c[0, 1, :, 9] = float('nan')
        got_s, got_c = cache.scores(q.to(DEV)), cache.context(p.to(DEV))
    assert_bits_equal(bits(got_s), bits(want_s), dtype, "scores with NaN blocks")
    assert_bits_equal(bits(got_c), bits(want_c), dtype, "context with NaN blocks")


@pytest.mark.parametrize("out_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("block", (16, 32, 64))
def test_strided_entry_exact(block, out_dtype):
    """native.hbfp_bmm_i8_strided on its own: w read in place from a larger array (row pitch 256 > ldk = 128, exponent pitch nb + 3, 96
    rows from batch to batch, 70 of N = 80 rows valid), a -128 exponent on each side; what lies outside w's valid part is never read"""
    B, T, N, K, m, rows, wbs, w_ld = 2, 40, 80, 128, 5, 70, 96, 256
    nb = K // block
    xc, xe, xv = _operand(B, T, K, m, -3, 2, 61, block)
    wc, we, wv = _operand(B, rows, K, m, -4, 2, 62, block)
    want = _want(xv, wv, xc, xe, wc, we, m, block, out_dtype)
    xe[1, 7, nb - 1] = -128
    we[0, 33, 0] = -128
    want[1, 7, :] = float('nan')
    want[0, :, 33] = float('nan')
    wcb = torch.full((B, wbs, w_ld), 77, dtype=torch.int8)                # rows past 70 and bytes past K: never read
    web = torch.full((B, wbs, nb + 3), -128, dtype=torch.int8)            # (read, they would make every output NaN)
    wcb[:, :rows, :K] = wc.to(torch.int8)
    web[:, :rows, :nb] = we.to(torch.int8)
    got = native.hbfp_bmm_i8_strided((xc.to(torch.int8).view(B * T, K).to(DEV), xe.to(torch.int8).view(B * T, nb).to(DEV)), wcb.to(DEV),
                                     web.to(DEV), B, T, N, K, wbs, rows, m, m, block_size=block, out_dtype=out_dtype)
    assert got.shape == (B, T, N) and got.dtype == out_dtype
    assert_bits_equal(bits(got[:, :, :rows]), bits(want), out_dtype, f"strided block {block} {out_dtype}")
    assert_bits_equal(bits(got[:, :, rows:]), bits(want[:, :, rows - 1:].expand(B, T, N - rows + 1)[:, :, 1:]), out_dtype, "rows past w_rows")


# ---- random data against the fake route's operands ---------------------------------------------------------------------------------
def _bound(got, x, w, kw, terms, dtype):
    with torch.no_grad():
        xq, wq = bfp_ops.MxM_pre_processing(x, w, True, **kw)
    xq, wq = xq.double(), wq.double()
    want = xq @ wq
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all())          # no output is left out of the comparison
    GC.elementwise_bound(got, want, xq.abs() @ wq.abs(), terms, dtype)


@pytest.mark.parametrize("pruning", ('dense', 'nm_x'))
@pytest.mark.parametrize("block,m", ((64, 7), (64, 3), (16, 7)))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
def test_products_against_the_fake_operands(dtype, block, m, pruning, monkeypatch):
    monkeypatch.setattr(bfp_ops, 'MATMUL_I8_MIN', {key: 1 for key in bfp_ops.MATMUL_I8_MIN})      # every default floor off
    B, H, D = 2, 3, 64
    kw = cfg(mant_bits=m, block_size=block, **(dict(in_sparsity=True, sparsity_mode='structured', N=2, M=4) if pruning == 'nm_x' else {}))
    g = torch.Generator().manual_seed(7)
    k, v = ((torch.randn(B, H, 192, D, generator=g) * s).to(dtype).to(DEV) for s in (1.0, 0.5))
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
    cache = mm.kv_cache(B, H, D, 192, dtype=dtype, device=DEV)
    calls = 0
    with torch.no_grad():
        for S, t in ((130, 130), (192, 62)):
            cache.append(k[:, :, S - t:S], v[:, :, S - t:S])
            for Tq in (1, 7):
                q = torch.randn(B, H, Tq, D, generator=g).to(dtype).to(DEV)
                scores = cache.scores(q)
                _bound(scores, q, k[:, :, :S].transpose(-1, -2), kw, D // block, dtype)
                p = torch.softmax(scores.float() / 8.0, dim=-1).to(dtype)
                ctx = cache.context(p)
                _bound(ctx, p, v[:, :, :S], kw, math.ceil(S / block), dtype)
                calls += 2
                if S % block == 0 and S % 16 == 0:
                    # the same codes, the same arithmetic in the same block order (no split of S is taken) as the batched route
                    assert_bits_equal(bits(scores), bits(mm(q, k[:, :, :S].transpose(-1, -2))), dtype, "scores vs matrix_unit='int8'")
                    assert_bits_equal(bits(ctx), bits(mm(p, v[:, :, :S])), dtype, "context vs matrix_unit='int8'")
    assert mm.matmul_stats.cache_calls == calls and mm.matmul_stats.fake_calls == 0


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
def test_greedy_decode_of_one_attention_layer(dtype):
    """70 steps, one token each: scores / 8, softmax, context (causal by construction), against the fake route fed by torch.cat"""
    B, H, D, block = 1, 4, 64, 64
    kw = cfg(mant_bits=7, block_size=block)
    g = torch.Generator().manual_seed(9)
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
    cache = mm.kv_cache(B, H, D, 70, dtype=dtype, device=DEV)
    past_k = past_v = None
    with torch.no_grad():
        for step in range(70):
            q, k, v = (torch.randn(B, H, 1, D, generator=g).to(dtype).to(DEV) for _ in range(3))
            past_k = k if past_k is None else torch.cat([past_k, k], dim=2)
            past_v = v if past_v is None else torch.cat([past_v, v], dim=2)
            assert cache.append(k, v) == step + 1
            scores = cache.scores(q)
            _bound(scores, q, past_k.transpose(-1, -2), kw, D // block, dtype)
            p = torch.softmax(scores.float() / 8.0, dim=-1).to(dtype)
            _bound(cache.context(p), p, past_v, kw, math.ceil((step + 1) / block), dtype)
    assert mm.matmul_stats.cache_calls == 140 and mm.matmul_stats.i8_calls == 0 and mm.matmul_stats.fake_calls == 0


def test_refusals_leave_the_cache_as_it_was():
    kw = cfg()
    cache = bfp_ops.HBFPKVCache(1, 2, 64, 100, dtype=torch.bfloat16, **kw)
    k = torch.randn(1, 2, 60, 64).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        cache.append(k, k)
        before = {name: t.clone() for name, t in cache.buffers.items()}
        with pytest.raises(ValueError, match="capacity"):
            cache.append(k[:, :, :41], k[:, :, :41])                          # 101 > 100, though the buffers hold 128
        with pytest.raises(ValueError):
            cache.append(k.float()[:, :, :1], k.float()[:, :, :1])
        with pytest.raises(ValueError):
            cache.context(torch.zeros(1, 2, 1, 59, dtype=torch.bfloat16, device=DEV))
        with pytest.raises(ValueError):
            cache.scores(k[:, :, :1].cpu())
    for call in (lambda: cache.append(k[:, :, :1], k[:, :, :1]), lambda: cache.scores(k[:, :, :1]),
                 lambda: cache.context(torch.zeros(1, 2, 1, 60, dtype=torch.bfloat16, device=DEV))):
        with pytest.raises(ValueError, match="gradients"):
            call()
    assert cache.length == 60 and cache.stats.cache_calls == 0
    for name, t in cache.buffers.items():
        assert torch.equal(t, before[name]), name
    with pytest.raises(ValueError, match="pruned K / V"):
        bfp_ops.HBFPKVCache(1, 2, 64, 100, dtype=torch.bfloat16, **cfg(w_sparsity=True))
    with pytest.raises(ValueError, match="stochastic"):
        bfp_ops.HBFPKVCache(1, 2, 64, 100, dtype=torch.bfloat16, **cfg(rounding_mode='stoc'))
