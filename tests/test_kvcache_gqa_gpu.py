"""GPU tests of grouped-query attention on the HBFP KV cache (bfp_ops.HBFPKVCache(kv_heads=...), csrc/bfpq_kvcache.hip).
The whole specification is one law: a grouped cache fed k, v equals, bit for bit, a twin HBFPKVCache(batch, heads, ...) without
kv_heads fed repeat_kv(k, g), repeat_kv(v, g) (the reference's modeling_llama.py:264-273: kv head h serves query heads h g .. h g + g - 1),
whose own contents and products the other test_kvcache_*_gpu.py files pin.  Every comparison is torch.equal, NaN-aware where a NaN is
planted.  Shapes: B 3, kv_heads 2 with g 2 or 4 and kv_heads 1 with g 8 (multi-query), D 64, capacity 320; Tq 1, 3 and 16 make
R = g Tq rows per kv head from 2 to 128: one partial tile, tiles that straddle query heads (Tq 3) and up to eight whole tiles."""
import pytest
import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)
B, D, CAP = 3, 64, 320
KVH = {2: 2, 4: 2, 8: 1}               # g -> kv_heads (g = 8 is the multi-query case)
LENS = {False: (0, 70, 200), True: (16, 70, 200)}      # by causal: an empty sequence / rows that see only a part of their sequence
TQS = (1, 3, 16)
CPS = (0, 1, 2)
MAX_LENS = (CAP, 256)
# every dtype with every block and every g with every dtype and every block (a Latin square in place of the 27-fold product)
CASES = [(dn, blk, (2, 4, 8)[(i + j) % 3]) for i, dn in enumerate(DT) for j, blk in enumerate((64, 32, 16))]
CASE_IDS = [f"{dn}-b{blk}-g{g}" for dn, blk, g in CASES]


def cfg(**kw):
    base = dict(mant_bits=7, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _rand(shape, dtype, seed):
    """magnitudes over many binades along the tokens (tests/test_kvcache_device_gpu.py)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-6, 4, shape[:-1] + (1,), generator=g).float())).to(dtype).to(DEV)


def repeat_kv(x, g):
    """the reference's repeat_kv (modeling_llama.py:264-273)"""
    b, h, s, d = x.shape
    return x[:, :, None].expand(b, h, g, s, d).reshape(b, h * g, s, d)


def _same(a, b):
    """torch.equal, any NaN matching any NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0.), b.masked_fill(nb, 0.))


class Pair:
    """a grouped cache and its twin (today's cache with heads = kv_heads g heads, fed repeat_kv), fed the same tokens"""

    def __init__(self, g, dtype, kw, **mode):
        self.g, self.kvh, self.heads = g, KVH[g], KVH[g] * g
        self.gqa = bfp_ops.HBFPKVCache(B, self.heads, D, CAP, dtype=dtype, kv_heads=self.kvh, **mode, **kw)
        self.twin = bfp_ops.HBFPKVCache(B, self.heads, D, CAP, dtype=dtype, **mode, **kw)
        assert self.gqa.nbytes() * g == self.twin.nbytes()

    def append(self, k, v, counts=None):
        args = () if counts is None else (_i32(*counts),)
        with torch.no_grad():
            self.gqa.append(k.contiguous(), v.contiguous(), *args)
            self.twin.append(repeat_kv(k, self.g).contiguous(), repeat_kv(v, self.g).contiguous(), *args)

    def fill(self, k, v, first):
        """ragged appends in chunks of 64, 37 and 1 tokens with counts: lengths (first, 70, 200), first <= 37"""
        self.append(k[:, :, :64], v[:, :, :64], (0, 64, 64))
        self.append(k[:, :, 64:128], v[:, :, 64:128], (0, 0, 64))
        self.append(k[:, :, 128:192], v[:, :, 128:192], (0, 0, 64))
        self.append(k[:, :, 192:229], v[:, :, 192:229], (first, 5, 7))
        self.append(k[:, :, 229:230], v[:, :, 229:230], (0, 1, 1))
        return self

    def both(self, f):
        with torch.no_grad():
            return f(self.gqa), f(self.twin)


def _pair(g, dtype, kw, seed, causal=False, **mode):
    pair = Pair(g, dtype, kw, device_lengths=True, **mode)
    k, v = _rand((B, pair.kvh, 230, D), dtype, seed), _rand((B, pair.kvh, 230, D), dtype, seed + 1)
    return pair.fill(k, v, LENS[causal][0])


def _probs(heads, Tq, L, lens, dtype, seed):
    """rows of probabilities with NaN and Inf past the lengths (what context() must count as zero)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(torch.randn(B, heads, Tq, L, generator=g) * 3, -1).to(dtype).to(DEV)
    for b, n in enumerate(lens):
        p[b, :, :, n:] = float('nan')
        p[b, :, :, n + 1::2] = float('inf')
    return p


# ---- 1. contents ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,block,g", CASES, ids=CASE_IDS)
def test_contents_are_the_twins_first_head_of_every_group(dname, block, g):
    dtype = DT[dname]
    pair = _pair(g, dtype, cfg(mant_bits=5, block_size=block), 10 * block + g)
    what = f"{dname} block {block} g {g}"
    assert pair.gqa.lengths.tolist() == pair.twin.lengths.tolist() == list(LENS[False]), what
    k, v = _rand((B, pair.kvh, 64, D), dtype, 3), _rand((B, pair.kvh, 64, D), dtype, 4)
    pair.append(k, v, (64, 64, 64))                            # sequence 2 would hold 264 ...
    pair.append(k, v, (0, 37, 64))                             # ... and now 328 > 320: refused, left as it is
    assert pair.gqa.lengths.tolist() == pair.twin.lengths.tolist() == [64, 171, 264], what
    assert pair.gqa.overflow.item() == pair.twin.overflow.item() == 1, what
    for name in ('k_codes', 'k_exps', 'v_codes', 'v_exps', 'v_tail'):
        got, want = getattr(pair.gqa, name), getattr(pair.twin, name)[:, ::g]
        assert got.shape == want.shape and got.shape[1] == pair.kvh and _same(got, want), f"{what}: {name}"
    for b in range(B):
        for f in (lambda c: c.keys(b), lambda c: c.values(b)):
            got, want = pair.both(f)
            assert got.shape == (1, pair.kvh, pair.gqa.lengths[b].item(), D) and _same(got, want[:, ::g]), f"{what}: sequence {b}"


# ---- 2. the products ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,block,g", CASES, ids=CASE_IDS)
def test_products_have_the_twins_bits(dname, block, g):
    dtype = DT[dname]
    kw = cfg(mant_bits=7 if g != 4 else 3, block_size=block)
    scale = D ** -0.5
    pairs = {(causal, cps): _pair(g, dtype, kw, 100 * block + g, causal, chunks_per_split=cps) for causal in (False, True) for cps in CPS}
    heads = pairs[False, 0].heads
    for Tq in TQS:
        q = _rand((B, heads, Tq, D), dtype, 7 + Tq)
        for max_len in MAX_LENS:
            p_in = _probs(heads, Tq, max_len, LENS[False], dtype, 11 + Tq)
            for (causal, cps), pair in pairs.items():
                what = f"{dname} block {block} g {g} Tq {Tq} max_len {max_len} causal {causal} chunks_per_split {cps}"
                if not causal:
                    got, want = pair.both(lambda c: c.scores(q, max_len))
                    assert got.shape == (B, heads, Tq, max_len) and _same(got, want), what + ": scores"
                    got, want = pair.both(lambda c: c.context(p_in))
                    assert got.shape == (B, heads, Tq, D) and not bool(torch.isnan(got).any()) and _same(got, want), what + ": context"
                (ctx, p), (wctx, wp) = pair.both(lambda c: c.attend(q, scale, max_len=max_len, causal=causal, return_probs=True))
                assert ctx.shape == (B, heads, Tq, D) and p.shape == (B, heads, Tq, max_len), what
                assert _same(ctx, wctx) and _same(p, wp), what + ": attend with return_probs"
                got, want = pair.both(lambda c: c.attend(q, scale, max_len=max_len, causal=causal))
                assert _same(got, want) and _same(got, ctx), what + ": attend"
    assert all(p.gqa.stats.cache_calls == p.twin.stats.cache_calls > 0 for p in pairs.values())
    assert all(p.gqa.lengths.tolist() == p.twin.lengths.tolist() == list(LENS[c]) and p.gqa.overflow.item() == 0 for (c, _), p in pairs.items())


# ---- 3. the host-length cache ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_sparsity", (False, True), ids=('dense', 'in_sparsity'))
@pytest.mark.parametrize("dname,block", (('fp32', 64), ('bf16', 32), ('fp16', 16)))
def test_host_length_cache_has_the_twins_bits(dname, block, in_sparsity):
    """g = 4: Tq 1 is R = 4 rows in the product kernel (dense; the twin's route too), Tq 16 is R = 64 rows through act_codes and the
    strided batched GEMM while the dense twin stays in the kernel; with in_sparsity (2:4 on q and p) both take the strided route"""
    dtype, g, S = DT[dname], 4, 128
    pair = Pair(g, dtype, cfg(mant_bits=5, block_size=block, in_sparsity=in_sparsity))
    k, v = _rand((B, pair.kvh, S, D), dtype, 31 + block), _rand((B, pair.kvh, S, D), dtype, 32 + block)
    pair.append(k[:, :, :37], v[:, :, :37])
    pair.append(k[:, :, 37:], v[:, :, 37:])
    assert pair.gqa.length == pair.twin.length == S
    for f in (lambda c: c.keys(), lambda c: c.values()):
        got, want = pair.both(f)
        assert _same(got, want[:, ::g])
    for Tq in (1, 16):
        q = _rand((B, pair.heads, Tq, D), dtype, 33 + Tq)
        p = torch.softmax(_rand((B, pair.heads, Tq, S), torch.float32, 35 + Tq), -1).to(dtype)
        what = f"{dname} block {block} in_sparsity {in_sparsity} Tq {Tq}"
        got, want = pair.both(lambda c: c.scores(q))
        assert got.shape == (B, pair.heads, Tq, S) and _same(got, want), what + ": scores"
        got, want = pair.both(lambda c: c.context(p))
        assert got.shape == (B, pair.heads, Tq, D) and _same(got, want), what + ": context"


# ---- 4. a captured step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,block", (('fp32', 64), ('bf16', 16)))
def test_captured_append_and_attend_replay_like_an_eager_twin(dname, block):
    dtype, g, steps, start = DT[dname], 4, 5, (0, 62, 126)
    pair = Pair(g, dtype, cfg(block_size=block), device_lengths=True, max_query_rows=1)
    cache, twin, kvh, heads = pair.gqa, pair.twin, pair.kvh, pair.heads
    k, v = _rand((B, kvh, 126 + steps, D), dtype, 51), _rand((B, kvh, 126 + steps, D), dtype, 52)
    qs = _rand((steps, B, heads, 1, D), dtype, 53)
    ik, iv = (torch.zeros(B, kvh, 1, D, dtype=dtype, device=DEV) for _ in range(2))
    iq = torch.zeros(B, heads, 1, D, dtype=dtype, device=DEV)
    scale = D ** -0.5

    def step():
        cache.append(ik, iv)
        return cache.attend(iq, scale)

    with torch.no_grad():
        step()                                                       # warm-up: code objects, the exponent window table, attend's workspace
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx = step()
        cache.reset()                                                # undo the warm-up and capture-time appends
        pair.append(k[:, :, :126], v[:, :, :126], start)
        for i in range(steps):
            ik.copy_(k[:, :, 126 + i:127 + i]); iv.copy_(v[:, :, 126 + i:127 + i]); iq.copy_(qs[i])
            graph.replay()
            twin.append(repeat_kv(ik, g).contiguous(), repeat_kv(iv, g).contiguous())
            want = twin.attend(iq, scale)
            assert cache.lengths.tolist() == twin.lengths.tolist() == [s + i + 1 for s in start], f"replay {i}"
            assert _same(ctx, want), f"{dname} block {block} replay {i}"
    assert cache.overflow.item() == twin.overflow.item() == 0


# ---- 5. NaN ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq", (1, 3))
@pytest.mark.parametrize("dname,block,g", CASES[::4], ids=CASE_IDS[::4])
def test_nan_in_q_reaches_only_its_own_query_head(dname, block, g, Tq):
    """the query heads of a group share a row tile and every load of the codes; a NaN in one of them stays in its own row"""
    dtype = DT[dname]
    pair = _pair(g, dtype, cfg(mant_bits=5, block_size=block), 600 + block, chunks_per_split=1)
    q = _rand((B, pair.heads, Tq, D), dtype, 61)
    bad = q.clone()
    h, t = g + 1 if pair.kvh > 1 else 1, Tq - 1                      # the second query head of a group
    bad[1, h, t, 5] = float('nan')
    scale = D ** -0.5
    clean, _ = pair.both(lambda c: c.attend(q, scale))
    got, want = pair.both(lambda c: c.attend(bad, scale))
    assert _same(got, want)
    hit = torch.zeros(B, pair.heads, Tq, dtype=torch.bool, device=DEV)
    hit[1, h, t] = True
    # (fp16 scores of these magnitudes can overflow to inf and make a NaN row of their own: the rows are compared with the clean call's)
    assert bool(torch.isnan(got[1, h, t]).all()) and not bool(torch.isnan(clean[1, h, t]).any())
    assert _same(got[~hit], clean[~hit])
    got, want = pair.both(lambda c: c.scores(bad))
    clean, _ = pair.both(lambda c: c.scores(q))
    assert _same(got, want) and bool(torch.isnan(got[1, h, t, :70]).all()) and _same(got[~hit], clean[~hit])


# ---- 6. memory ------------------------------------------------------------------------------------------------------------------------
def test_no_allocation_after_prepare_attend_and_the_twins_workspaces():
    dtype, g = torch.bfloat16, 4
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **cfg())
    cache = mm.kv_cache(B, 8, D, CAP, dtype=dtype, device_lengths=True, max_query_rows=3, kv_heads=2)
    twin = mm.kv_cache(B, 8, D, CAP, dtype=dtype, device_lengths=True, max_query_rows=3)
    assert (cache.kv_heads, cache.group) == (2, g) and cache.nbytes() * g == twin.nbytes() and cache._att_ws is None
    assert cache._ws.numel() == twin._ws.numel()
    k, v = _rand((B, 2, 200, D), dtype, 71), _rand((B, 2, 200, D), dtype, 72)
    q = _rand((B, 8, 3, D), dtype, 73)
    with torch.no_grad():
        cache.append(k, v, _i32(*LENS[False]))
        cache.prepare_attend()
        twin.prepare_attend()
        ws = cache._att_ws
        assert ws.numel() == twin._att_ws.numel() == B * 8 * 3 * CAP * 4                 # fp32 [B heads, max_query_rows, cap]
        ctx = cache.attend(q, 0.125)                                                     # (code objects, the exponent window table)
        del ctx
        calls, held = mm.matmul_stats.cache_calls, torch.cuda.memory_allocated()
        for i in range(2):
            ctx, p = cache.attend(q, 0.125, max_len=256, causal=bool(i), return_probs=True)
            del ctx, p
        assert torch.cuda.memory_allocated() == held and cache._att_ws is ws
        assert mm.matmul_stats.cache_calls == calls + 4
        with pytest.raises(ValueError, match="max_query_rows"):
            cache.attend(_rand((B, 8, 4, D), dtype, 74), 0.125)
        with pytest.raises(ValueError):
            cache.attend(q[:, :2], 0.125)                                                # q with kv_heads heads
        with pytest.raises(ValueError):
            cache.append(repeat_kv(k, g), repeat_kv(v, g))                               # k_new with heads heads
