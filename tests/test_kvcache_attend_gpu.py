"""GPU tests of HBFPKVCache.attend (bfp_ops.HBFPKVCache(device_lengths=True), csrc/bfpq_kvcache.hip): one call for the
scores, the scale, the softmax and the context of a decode step.  What is pinned bit for bit is everything downstream of the
probabilities p (against cache.context(p), tests/test_kvcache_device_gpu.py pins that to the host-length cache) and, on exact operands,
the whole call against the composition it replaces; the softmax itself is measured against float64 next to torch's own."""
import pytest
import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import bits, assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ('fp32', 'bf16', 'fp16')
B, H, CAP = 3, 2, 320
LENS = (1, 70, 200)                    # a 64-token chunk crossed, a ragged last block, a slice boundary (chunks_per_split 1, 2)
DBLK = ((64, 64), (64, 32), (32, 16))
TQS = (1, 3, 16)
CPS = (0, 1, 2)
MAX_LENS = (CAP, 256)
ULP_HALF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # the spacing of the dtype at 1/2
TINY = {dt: torch.finfo(dt).tiny for dt in DTYPES}


def cfg(**kw):
    base = dict(mant_bits=7, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _tokens(b, h, S, D, dtype, seed):
    """the inputs of tests/test_kvcache_device_gpu.py: magnitudes over many binades along the tokens"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.randn(b, h, S, D, generator=g) * torch.exp2(torch.randint(-6, 4, (b, h, S, 1), generator=g).float())).to(dtype).to(DEV)
    return mk(), mk()


def _queries(Tq, D, dtype, seed):
    return _tokens(B, H, Tq, D, dtype, seed)[0]


def _cache(D, dtype, kw, k, v, lens, **mode):
    c = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=dtype, device_lengths=True, **mode, **kw)
    with torch.no_grad():
        c.append(k, v, _i32(*lens))
    return c


def _visible(lens, Tq, max_len, causal):
    """[B, 1, Tq, max_len] bool: the keys each query row sees"""
    n = torch.arange(max_len, device=DEV).view(1, 1, 1, -1)
    L = torch.tensor(lens, device=DEV).view(-1, 1, 1, 1)
    t = torch.arange(Tq, device=DEV).view(1, 1, -1, 1)
    return (n <= L - Tq + t) & (n < L) if causal else (n < L).expand(-1, 1, Tq, -1)


def _masked_scores(cache, q, scale, max_len, causal, lens):
    s = cache.scores(q, max_len).float() * scale
    return s.masked_fill(~_visible(lens, q.shape[2], max_len, causal), float('-inf'))


def _plus_zero(p, vis, what):
    hidden = p[(~vis).expand_as(p)]
    assert not bool(hidden.any()) and not bool(torch.signbit(hidden).any()), f"{what}: p is not +0 at a key the row does not see"


# ---- 1. downstream of p, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (3, 7))
@pytest.mark.parametrize("D,block", DBLK)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_context_has_the_bits_of_context_of_p(dtype, D, block, m):
    kw = cfg(mant_bits=m, block_size=block)
    k, v = _tokens(B, H, max(LENS), D, dtype, 100 * block + m)
    caches = [_cache(D, dtype, kw, k, v, LENS, chunks_per_split=cps) for cps in CPS]
    scale = D ** -0.5
    for Tq in TQS:
        q = _queries(Tq, D, dtype, 7 + Tq)
        for max_len in MAX_LENS:
            vis = _visible(LENS, Tq, max_len, False)
            first = None
            for cache, cps in zip(caches, CPS):
                what = f"{dtype} D {D} block {block} m {m} Tq {Tq} max_len {max_len} chunks_per_split {cps}"
                with torch.no_grad():
                    ctx, p = cache.attend(q, scale, max_len=max_len, return_probs=True)
                    alone = cache.attend(q, scale, max_len=max_len)
                    want = cache.context(p)
                assert ctx.shape == (B, H, Tq, D) and ctx.dtype == dtype and p.shape == (B, H, Tq, max_len) and p.dtype == dtype, what
                assert_bits_equal(bits(ctx), bits(want), dtype, what + ": attend against context(p)")
                assert_bits_equal(bits(alone), bits(ctx), dtype, what + ": with and without return_probs")
                _plus_zero(p, vis, what)
                if first is None:
                    first = (bits(ctx), bits(p))
                else:
                    assert_bits_equal(bits(ctx), first[0], dtype, what + ": against chunks_per_split 0")
                    assert_bits_equal(bits(p), first[1], dtype, what + ": p against chunks_per_split 0")
            if max_len == CAP:
                with torch.no_grad():
                    assert_bits_equal(bits(caches[0].attend(q, scale)), bits(ctx), dtype, what + ": max_len defaults to the capacity")


# ---- 2. the softmax against float64 -------------------------------------------------------------------------------------------------------
def _rel_err(p, truth, ok):
    return float(((p.double() - truth).abs() / truth)[ok].max())


@pytest.mark.parametrize("m", (3, 7))
@pytest.mark.parametrize("D,block", DBLK)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_softmax_is_as_accurate_as_torchs(dtype, D, block, m):
    """the largest relative error of p over the visible keys whose true probability is a normal number of the dtype: the kernel's may be
    at most twice that of torch.softmax(s, -1).to(dtype) on the same s (another exp and another summation order move a few fp32 ulps;
    for the 16-bit dtypes both sit near half an ulp of the dtype).  Measured on an MI355X, kernel / torch, the worst of each dtype
    over all cases: fp32 3.92e-06 / 3.95e-06 (the ratio of one case at most 1.43), bf16 3.88e-03 / 3.88e-03, fp16 4.81e-04 / 4.81e-04
    (DESIGN 5l)."""
    kw = cfg(mant_bits=m, block_size=block)
    k, v = _tokens(B, H, max(LENS), D, dtype, 200 * block + m)
    cache = _cache(D, dtype, kw, k, v, LENS)
    scale = D ** -0.5
    for Tq in TQS:
        q = _queries(Tq, D, dtype, 17 + Tq)
        for max_len in MAX_LENS:
            for causal in (False, True):
                what = f"{dtype} D {D} block {block} m {m} Tq {Tq} max_len {max_len} causal {causal}"
                vis = _visible(LENS, Tq, max_len, causal)
                with torch.no_grad():
                    s = _masked_scores(cache, q, scale, max_len, causal, LENS)
                    _, p = cache.attend(q, scale, max_len=max_len, causal=causal, return_probs=True)
                seen = vis.any(-1, keepdim=True).expand_as(s)                              # (rows that see no key: p is all +0, no softmax)
                truth = torch.softmax(s.double(), -1)
                torchs = torch.softmax(s, -1).to(dtype)
                ok = vis.expand_as(s) & seen & (truth > TINY[dtype])
                assert bool(ok.any()), what
                ours, theirs = _rel_err(p, truth, ok), _rel_err(torchs, truth, ok)
                print(f"softmax {what}: kernel {ours:.3e} torch {theirs:.3e}")
                assert ours <= 2 * theirs, f"{what}: kernel {ours:.3e}, torch {theirs:.3e}"
                rows = vis.sum(-1).expand(B, H, Tq)
                err = (p.double().sum(-1) - 1).abs()
                assert bool((err[rows > 0] <= rows[rows > 0] * ULP_HALF[dtype]).all()), f"{what}: a row of p does not sum to 1"


# ---- 3. exact operands, end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ((1, 64, 128), (0, 64, 128)), ids=('full', 'one_empty'))
@pytest.mark.parametrize("D,block", DBLK)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_equal_scores_give_the_composition_bit_for_bit(dtype, D, block, lens):
    """every key of a sequence is the same row: all its scores are equal, exp is exactly 1, the sum exactly the length (a power of two)
    and p exactly 1 / length in every dtype and for any summation order -- so the whole call must equal the composition it replaces"""
    kw = cfg(mant_bits=7, block_size=block)
    k, v = _tokens(B, H, max(lens), D, dtype, 300 + block)
    k = k[:, :, :1].expand(-1, -1, max(lens), -1).contiguous()
    cache = _cache(D, dtype, kw, k, v, lens)
    scale = D ** -0.5
    for Tq in TQS:
        q = _queries(Tq, D, dtype, 27 + Tq)
        for max_len in MAX_LENS:
            what = f"{dtype} D {D} block {block} lengths {lens} Tq {Tq} max_len {max_len}"
            with torch.no_grad():
                ctx, p = cache.attend(q, scale, max_len=max_len, return_probs=True)
                want = cache.context(torch.softmax(cache.scores(q, max_len).float() * scale, -1).to(dtype))
            assert_bits_equal(bits(ctx), bits(want), dtype, what)
            for b, n in enumerate(lens):
                if n:
                    assert bool((p[b, :, :, :n] == torch.tensor(1.0 / n).to(dtype)).all()), what + f": p of sequence {b} is not 1 / {n}"
                else:
                    assert not bool(ctx[b].any()) and not bool(torch.signbit(ctx[b]).any()), what + ": the empty sequence's context is not zero"
            _plus_zero(p[[b for b, n in enumerate(lens) if n]], _visible([n for n in lens if n], Tq, max_len, False), what)


# ---- 4. causal ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,block", DBLK)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_causal_rows_are_the_rows_of_shorter_caches(dtype, D, block):
    """row t of the causal p against the non-causal p of a twin cache that holds only the lengths[b] - Tq + 1 + t tokens the row sees
    (key rows are final once appended, so this is exact); the sequence of length 1 has rows that see nothing: all of p is +0 there"""
    Tq = 4
    kw = cfg(mant_bits=5, block_size=block)
    k, v = _tokens(B, H, max(LENS), D, dtype, 400 + block)
    q = _queries(Tq, D, dtype, 41)
    scale = D ** -0.5
    seen = [[max(0, n - Tq + 1 + t) for n in LENS] for t in range(Tq)]
    twins = [_cache(D, dtype, kw, k, v, seen[t]) for t in range(Tq)]
    first = None
    for cps in CPS:
        cache = _cache(D, dtype, kw, k, v, LENS, chunks_per_split=cps)
        for max_len in MAX_LENS:
            what = f"causal {dtype} D {D} block {block} chunks_per_split {cps} max_len {max_len}"
            with torch.no_grad():
                ctx, p = cache.attend(q, scale, max_len=max_len, causal=True, return_probs=True)
                assert_bits_equal(bits(ctx), bits(cache.context(p)), dtype, what + ": attend against context(p)")
                assert_bits_equal(bits(cache.attend(q, scale, max_len=max_len, causal=True)), bits(ctx), dtype, what + ": without return_probs")
                _plus_zero(p, _visible(LENS, Tq, max_len, True), what)
                for t in range(Tq):
                    _, pt = twins[t].attend(q, scale, max_len=max_len, return_probs=True)
                    for b, n in enumerate(seen[t]):
                        assert_bits_equal(bits(p[b, :, t, :n]), bits(pt[b, :, t, :n]), dtype, what + f": row {t} of sequence {b} over {n} keys")
            if max_len == CAP:
                if first is None:
                    first = bits(ctx)
                assert_bits_equal(bits(ctx), first, dtype, what + ": against chunks_per_split 0")


# ---- 5. a captured step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,block", DBLK)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_captured_append_and_attend_advance_on_every_replay(dtype, D, block):
    start, steps = (0, 62, 126), 5                                   # blocks close during the replays (16: 62 -> 64, 126 -> 128)
    kw = cfg(block_size=block)
    scale = D ** -0.5
    k, v = _tokens(B, H, max(start) + steps, D, dtype, 500 + block)
    qs = torch.stack([_queries(1, D, dtype, 51 + i) for i in range(steps)])
    cache = _cache(D, dtype, kw, k[:, :, :max(start)], v[:, :, :max(start)], start)
    twin = _cache(D, dtype, kw, k[:, :, :max(start)], v[:, :, :max(start)], start)
    sk, sv, sq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(3))
    ik, iv, iq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(3))

    def step():
        sk.copy_(ik); sv.copy_(iv); sq.copy_(iq)
        cache.append(sk, sv)
        return cache.attend(sq, scale)

    with torch.no_grad():
        step()                                                       # warm-up: code objects, the exponent window table, attend's workspace
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx = step()
        cache.reset()                                                # undo the warm-up and capture-time appends
        cache.append(k[:, :, :max(start)].contiguous(), v[:, :, :max(start)].contiguous(), _i32(*start))
        for i in range(steps):
            n = max(start) + i
            ik.copy_(k[:, :, n:n + 1]); iv.copy_(v[:, :, n:n + 1]); iq.copy_(qs[i])
            graph.replay()
            twin.append(ik, iv)
            want = twin.attend(iq, scale)
            assert cache.lengths.tolist() == [s + i + 1 for s in start], f"replay {i}"
            assert_bits_equal(bits(ctx), bits(want), dtype, f"{dtype} D {D} block {block} replay {i}")
    assert cache.overflow.item() == 0 and twin.lengths.tolist() == cache.lengths.tolist()


# ---- 6. NaN ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("D,block", DBLK)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_in_q_stays_in_its_row(dtype, D, block, causal):
    lens, Tq = (5, 70, 200), 3
    kw = cfg(mant_bits=5, block_size=block)
    k, v = _tokens(B, H, max(lens), D, dtype, 600 + block)
    cache = _cache(D, dtype, kw, k, v, lens, chunks_per_split=1)
    q = _queries(Tq, D, dtype, 61)
    bad = q.clone()
    bad[1, 1, 2, 5] = float('nan')
    scale = D ** -0.5
    with torch.no_grad():
        clean, got = cache.attend(q, scale, causal=causal), cache.attend(bad, scale, causal=causal)
        want = cache.context(torch.softmax(_masked_scores(cache, bad, scale, CAP, causal, lens), -1).to(dtype))
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got[1, 1, 2]).all())
    keep = torch.ones(B, H, Tq, dtype=torch.bool)
    keep[1, 1, 2] = False
    assert_bits_equal(bits(got.cpu()[keep]), bits(clean.cpu()[keep]), dtype, f"{dtype} D {D} block {block}: the rows without the NaN")


# ---- 7. refusals, statistics, memory ------------------------------------------------------------------------------------------------------
def test_refusals_statistics_and_memory():
    D, dtype = 64, torch.bfloat16
    kw = cfg()
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
    k, v = _tokens(B, H, max(LENS), D, dtype, 700)
    q = _queries(2, D, dtype, 71)
    host = mm.kv_cache(B, H, D, CAP, dtype=dtype)
    cache = mm.kv_cache(B, H, D, CAP, dtype=dtype, device_lengths=True, max_query_rows=2)
    assert cache._att_ws is None                                                       # no workspace for caches that never attend
    with torch.no_grad():
        cache.append(k, v, _i32(*LENS))
        with pytest.raises(ValueError, match="attend needs device_lengths=True"):
            host.attend(q, 0.125)
        with pytest.raises(ValueError, match="max_query_rows"):
            cache.attend(_queries(3, D, dtype, 72), 0.125)
        with pytest.raises(ValueError, match="query rows"):
            cache.attend(_queries(17, D, dtype, 73), 0.125)
        for bad in (float('nan'), float('inf'), -float('inf'), None, '1', True, 1j):
            with pytest.raises(ValueError, match="scale"):
                cache.attend(q, bad)
        for bad in (0, CAP + 1, -1, 64.0, True):
            with pytest.raises(ValueError, match="max_len"):
                cache.attend(q, 0.125, max_len=bad)
        for bad in (q.float(), q[:, :1], q[..., :32], q[0], q.cpu()):
            with pytest.raises(ValueError):
                cache.attend(bad, 0.125)
    with pytest.raises(ValueError, match="gradients"):
        cache.attend(q, 0.125)
    assert mm.matmul_stats.cache_calls == 0 and cache._att_ws is None
    with torch.no_grad():
        ctx = cache.attend(q, 0.125)
        assert mm.matmul_stats.cache_calls == 2
        ws = cache._att_ws
        assert ws is not None and ws.numel() == B * H * 2 * CAP * 4                    # fp32 [B H, max_query_rows, cap], made once
        del ctx
        held = torch.cuda.memory_allocated()
        for i in range(2):
            ctx, p = cache.attend(q, 0.125, max_len=256, causal=bool(i), return_probs=True)
            del ctx, p
        assert torch.cuda.memory_allocated() == held and cache._att_ws is ws
        assert mm.matmul_stats.cache_calls == 6
