"""GPU tests of the KV-cache and batched int8 kernels (csrc/bfpq_kvcache.hip, csrc/bfpq_bmm.hip) where their 64-bit addressing and their
grid-stride loops do something: buffers past 2^31 and 2^32 bytes, more heads, tiles or batches than a grid dimension, and live tokens at
the end of a 2^20-token capacity (the geometries are tests/large_cases.py, their premises tests/test_large_offsets_host.py).

The reference for addressing is the same operation on a small buffer: every sequence, head or batch of a big call holds its own random
data and is compared, bit for bit, with a twin that holds only a slab of them -- all of them, since an offset that wraps at 2^32 lands
in another sequence's region and shows in the victim or in the culprit.  Twins share the kernels, so each case also holds two sequences
to the oracle's quantizer and one scores and one context result to the fp64 product of the fake-quantized operands.  The work is
zero-filling and short lengths, never the full capacity; each test prints its peak memory and wall time."""
import math
import time

import pytest
import torch

import gemm_cases as GC
import large_cases as LC
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import bits, assert_bits_equal
from oracle import oracle as O
from test_kvcache_gpu import cfg, _bound, _uz
from test_kvcache_device_gpu import _check_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPE = torch.bfloat16
CODES = ('k_codes', 'k_exps', 'v_codes', 'v_exps')


@pytest.fixture(autouse=True)
def _measured(request):
    """peak memory and wall time of every test, printed; nothing is held over to the next test.  The cache is inference only: the tests
    run without gradient recording"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    with torch.no_grad():
        yield
    torch.cuda.synchronize()
    seconds, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated()
    print(f"\nlarge offsets {request.node.name}: peak {peak / LC.GiB:.2f} GiB, {seconds:.2f} s")
    torch.cuda.empty_cache()
    assert peak <= LC.BUDGET, f"{request.node.name} held {peak / LC.GiB:.2f} GiB"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _tokens(shape, g):
    """random rows whose magnitudes spread over ten binades (tests/test_kvcache_attend_gpu.py: _tokens), made on the device"""
    x = torch.randn(shape, generator=g, device=DEV)
    e = torch.randint(-6, 4, tuple(shape[:-1]) + (1,), generator=g, device=DEV)
    return (x * torch.exp2(e.float())).to(DTYPE)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _same(got, want, what, dtype=DTYPE):
    """assert_bits_equal, the common case decided on the device"""
    assert got.shape == want.shape and got.dtype == want.dtype == dtype, (what, got.shape, want.shape)
    iv = torch.int32 if dtype == torch.float32 else torch.int16
    if torch.equal(got.contiguous().view(iv), want.contiguous().view(iv)):
        return
    assert_bits_equal(bits(got), bits(want), dtype, what)


def _same_buffers(big, twin, s0, s1, what):
    """the five arrays of the twin against the slab's part of the big cache's, whole: codes, exponents, zeros and all"""
    for name in CODES:
        assert torch.equal(getattr(big, name)[s0:s1], getattr(twin, name)), f"{what}: {name}"
    _same(big.v_tail[s0:s1], twin.v_tail, f"{what}: v_tail")


def _untouched(cache, lo, hi, w0, w1, what, stale=0):
    """Nothing written out of place: sequence b holds the tokens lo[b] <= n < hi[b] (int64 [B] on the device), all of them inside
    [w0, w1) (multiples of 64); every byte of k_codes, k_exps and v_codes at another token is zero, and so is every byte of v_exps at a
    token block that holds none.  Reductions on the device: the bulk outside the window as 64-bit words, the window under a mask.
    stale: the first `stale` tokens of k_codes, k_exps and v_exps hold an earlier fill that reset() leaves; the caller holds those."""
    B, H, cap, D, blk = cache.batch, cache.kv_heads, cache.cap, cache.head_dim, cache.block
    assert w0 % 64 == 0 and w1 % 64 == 0 and stale % 64 == 0 and 0 <= stale <= w0 < w1 <= cap
    assert bool(((lo >= w0) & (hi <= w1) & (lo <= hi)).all())
    tok = torch.arange(w0, w1, device=DEV)
    dead = ~((tok >= lo.view(-1, 1)) & (tok < hi.view(-1, 1)))                       # [B, tokens of the window]
    for name in ('k_codes', 'k_exps'):
        t = getattr(cache, name)
        rowb = t.shape[-1]
        words = t.view(B, H, cap * rowb).view(torch.int64)
        assert not bool(words[:, :, stale * rowb // 8:w0 * rowb // 8].any()), f"{what}: {name} below token {w0}"
        assert not bool(words[:, :, w1 * rowb // 8:].any()), f"{what}: {name} from token {w1} on"
        assert not bool(((t[:, :, w0:w1] != 0).any(-1) & dead[:, None, :]).any()), f"{what}: {name} at a token its sequence does not hold"
    words = cache.v_codes.view(torch.int64)
    assert not bool(words[..., :w0 // 8].any()) and not bool(words[..., w1 // 8:].any()), f"{what}: v_codes outside tokens {w0}..{w1}"
    assert not bool(((cache.v_codes[..., w0:w1] != 0) & dead[:, None, None, :]).any()), f"{what}: v_codes at a token its sequence does not hold"
    jb = torch.arange(w0 // blk, w1 // blk, device=DEV)
    dead_b = ~((jb * blk < hi.view(-1, 1)) & ((jb + 1) * blk > lo.view(-1, 1)) & (hi > lo).view(-1, 1))
    assert not bool(cache.v_exps[..., stale // blk:w0 // blk].any()) and not bool(cache.v_exps[..., w1 // blk:].any()), f"{what}: v_exps outside"
    assert not bool(((cache.v_exps[..., w0 // blk:w1 // blk] != 0) & dead_b[:, None, None, :]).any()), f"{what}: v_exps at an empty token block"
    if cache.device_lengths:
        assert int(cache.overflow.item()) == 0, f"{what}: overflow is set"


def _visible(lens, Tq, max_len, causal):
    """[B, 1, Tq, max_len] bool: the keys each query row sees (tests/test_kvcache_attend_gpu.py), lens on the device"""
    n = torch.arange(max_len, device=DEV).view(1, 1, 1, -1)
    L = lens.view(-1, 1, 1, 1)
    t = torch.arange(Tq, device=DEV).view(1, 1, -1, 1)
    return (n <= L - Tq + t) & (n < L) if causal else (n < L).expand(-1, 1, Tq, -1)


def _bound_scores(scores, q, k_all, kw):
    """one sequence's scores [1, heads, Tq, >= S] against the fp64 product of the fake-quantized q and keys k_all [1, kv_heads, S, D]"""
    S, g = k_all.shape[2], q.shape[1] // k_all.shape[1]
    _bound(scores[..., :S], q, k_all.repeat_interleave(g, 1).transpose(-1, -2), kw, k_all.shape[-1] // kw['block_size'], DTYPE)


def _bound_context(ctx, p, v_all, kw):
    S, g = v_all.shape[2], p.shape[1] // v_all.shape[1]
    _bound(ctx, p[..., :S].contiguous(), v_all.repeat_interleave(g, 1), kw, math.ceil(S / kw['block_size']), DTYPE)


def _slab(inp, s0, s1):
    return {name: t[s0:s1] for name, t in inp.items()}


# ---- A: many sequences, device lengths, grouped heads ---------------------------------------------------------------------------------------
def _serving(cache, inp, c, scale):
    """what case A runs on a cache, big or twin: the two appends, scores, attend for every (Tq, causal), context of a returned p"""
    with torch.no_grad():
        if cache.starts is not None:
            cache.starts.copy_(inp['starts'])
        cache.append(inp['k1'], inp['v1'], inp['counts'])
        cache.append(inp['k2'], inp['v2'])
        out = {'lengths': cache.lengths.clone(), 'scores': cache.scores(inp['q3'], c['max_len'])}
        for Tq in c['tqs']:
            for causal in (False, True):
                out[f'ctx Tq {Tq} causal {causal}'], out[f'p Tq {Tq} causal {causal}'] = cache.attend(
                    inp[f'q{Tq}'], scale, max_len=c['max_len'], causal=causal, return_probs=True)
        out['context'] = cache.context(out['p Tq 3 causal False'])
    return out


@pytest.mark.parametrize("mode", ('plain', 'starts_window'))
def test_a_serving_batch_past_4gib_of_codes(mode):
    """k_kv_append<.., true>, k_kv_bmm_dec kDev / kAtt, k_kv_pv_split and k_kv_pv_combine at 640 sequences x 8 kv heads x 8000 tokens x
    128: 5.24 GB of k_codes and of v_codes; sequence 262 holds byte 2^31 and sequence 524 byte 2^32 of either"""
    c, kw = LC.A, cfg(block_size=LC.A['block'])
    B, Hq, H, D, t = c['batch'], c['heads'], c['kv_heads'], c['head_dim'], c['chunk']
    extra = dict(starts=True, window=c['window']) if mode == 'starts_window' else {}
    make = lambda batch: bfp_ops.HBFPKVCache(**dict(LC.cache_kwargs(c, batch), **extra), dtype=DTYPE, **kw)
    g = _gen(11)
    counts = LC.ragged_counts(B, t)
    inp = dict(k1=_tokens((B, H, t, D), g), v1=_tokens((B, H, t, D), g), k2=_tokens((B, H, 1, D), g), v2=_tokens((B, H, 1, D), g),
               q1=_tokens((B, Hq, 1, D), g), q3=_tokens((B, Hq, 3, D), g), counts=_i32(counts),
               starts=_i32((3 * b) % 40 for b in range(B)))                      # (some past their sequence's length: rows that see nothing)
    scale = D ** -0.5
    big = make(B)
    assert big.k_codes.numel() > LC.P32 and big.v_codes.numel() > LC.P32
    got = _serving(big, inp, c, scale)
    lens = torch.tensor([n + 1 for n in counts], device=DEV)
    assert torch.equal(got['lengths'].long(), lens)
    _untouched(big, torch.zeros_like(lens), lens, 0, 128, f"A {mode}")
    _same(got['ctx Tq 3 causal False'], got['context'], f"A {mode}: attend against context(p)")
    for s0 in range(0, B, c['slab']):
        s1, what = s0 + c['slab'], f"A {mode}, sequences {s0}..{s0 + c['slab'] - 1}"
        twin = make(c['slab'])
        want = _serving(twin, _slab(inp, s0, s1), c, scale)
        assert torch.equal(got['lengths'][s0:s1], want['lengths']), what
        for name in want:
            if name != 'lengths':
                _same(got[name][s0:s1], want[name], f"{what}: {name}")
        _same_buffers(big, twin, s0, s1, what)
        for i in range(c['slab']):
            _same(big.keys(s0 + i), twin.keys(i), f"{what}: keys({s0 + i})")
            _same(big.values(s0 + i), twin.values(i), f"{what}: values({s0 + i})")
        del twin, want
    # the anchors: the sequence that holds byte 2^32 and the last one against the oracle; the first one's products against fp64
    for b in c['anchors']:
        k_all = torch.cat([inp['k1'][b:b + 1, :, :counts[b]], inp['k2'][b:b + 1]], 2)
        v_all = torch.cat([inp['v1'][b:b + 1, :, :counts[b]], inp['v2'][b:b + 1]], 2)
        _check_oracle(big, b, k_all, v_all, kw, f"A {mode}")
        if b == c['anchors'][0]:
            _bound_scores(got['scores'][b:b + 1], inp['q3'][b:b + 1], k_all, kw)
            _bound_context(got['context'][b:b + 1], got['p Tq 3 causal False'][b:b + 1], v_all, kw)


# ---- B and F (i): host-length caches ---------------------------------------------------------------------------------------------------------
def _products(cache, inp, c, scale):
    """the two appends, then scores and context for every Tq; the p of a Tq is made once, from the first cache's scores"""
    out = {}
    with torch.no_grad():
        cache.append(inp['k1'], inp['v1'])
        cache.append(inp['k2'], inp['v2'])
        for Tq in c['tqs']:
            out[f'scores Tq {Tq}'] = s = cache.scores(inp[f'q{Tq}'])
            if f'p{Tq}' not in inp:
                inp[f'p{Tq}'] = torch.softmax(s.float() * scale, -1).to(DTYPE)
            out[f'context Tq {Tq}'] = cache.context(inp[f'p{Tq}'])
    return out


def _host_length_case(c, kw, label, seed):
    B, Hq, H, D, t = c['batch'], c['heads'], c['kv_heads'], c['head_dim'], c['chunk']
    make = lambda batch: bfp_ops.HBFPKVCache(**LC.cache_kwargs(c, batch), dtype=DTYPE, **kw)
    g = _gen(seed)
    inp = dict(k1=_tokens((B, H, t, D), g), v1=_tokens((B, H, t, D), g), k2=_tokens((B, H, 1, D), g), v2=_tokens((B, H, 1, D), g))
    for Tq in c['tqs']:
        inp[f'q{Tq}'] = _tokens((B, Hq, Tq, D), g)
    scale = D ** -0.5
    big = make(B)
    got = _products(big, inp, c, scale)
    S = t + 1
    assert big.length == S
    hi = torch.full((B,), S, device=DEV)
    _untouched(big, torch.zeros_like(hi), hi, 0, 64 if S <= 64 else 128, label)
    with torch.no_grad():
        all_k, all_v = big.keys(), big.values()
    for s0 in range(0, B, c['slab']):
        s1, what = s0 + c['slab'], f"{label}, sequences {s0}..{s0 + c['slab'] - 1}"
        twin = make(c['slab'])
        want = _products(twin, _slab(inp, s0, s1), c, scale)
        for name in want:
            _same(got[name][s0:s1], want[name], f"{what}: {name}")
        _same_buffers(big, twin, s0, s1, what)
        with torch.no_grad():
            _same(all_k[s0:s1], twin.keys(), f"{what}: keys()")
            _same(all_v[s0:s1], twin.values(), f"{what}: values()")
        del twin, want
    Tq = c['tqs'][0]
    for b in c['anchors']:
        k_all, v_all = (torch.cat([inp[a][b:b + 1], inp[z][b:b + 1]], 2) for a, z in (('k1', 'k2'), ('v1', 'v2')))
        want_k = O.float_to_bfp_blocked(k_all.cpu(), **kw, identifier='w')
        want_v = O.float_to_bfp_blocked(v_all.cpu().transpose(-1, -2).contiguous(), **kw, identifier='w').transpose(-1, -2)
        assert_bits_equal(bits(_uz(all_k[b:b + 1])), bits(_uz(want_k)), DTYPE, f"{label}: keys of sequence {b} against the oracle")
        assert_bits_equal(bits(_uz(all_v[b:b + 1])), bits(_uz(want_v.contiguous())), DTYPE, f"{label}: values of sequence {b} against the oracle")
        if b == c['anchors'][0]:
            _bound_scores(got[f'scores Tq {Tq}'][b:b + 1], inp[f'q{Tq}'][b:b + 1], k_all, kw)
            _bound_context(got[f'context Tq {Tq}'][b:b + 1], inp[f'p{Tq}'][b:b + 1], v_all, kw)


def test_b_host_length_batch_past_4gib_of_codes():
    """k_kv_append<.., false> and k_kv_bmm_dec kHost (Tq 3: 12 rows per kv head), act_codes and hbfp_bmm_i8_strided (Tq 40: 160 rows,
    the batch stride b * wbs * ldw past 2^32) on case A's buffers"""
    _host_length_case(LC.B, cfg(block_size=LC.B['block']), "B", 21)


@pytest.mark.parametrize("block", LC.F_BLOCKS)
def test_f_host_length_heads_past_a_grid_dimension(block):
    """65600 heads: the second trip of k_kv_bmm_dec's loop over blockIdx.y, both families; head 65535 is in the anchor sequence"""
    _host_length_case(LC.with_block(LC.F_HOST, block), cfg(block_size=block), f"F host block {block}", 61 + block)


# ---- C: long sequences, the panel route, late positions ---------------------------------------------------------------------------------------
def _attends(cache, q, scale, max_len, tqs):
    """attend, causal, for every Tq: with p on the 16-row route (Tq 1), without on the panel route (at the full capacity p is 2 GB)"""
    out = {}
    with torch.no_grad():
        for Tq in tqs:
            if Tq <= native.KV_DEC_MAX_TOKENS:
                out[f'ctx Tq {Tq}'], out[f'p Tq {Tq}'] = cache.attend(q[Tq], scale, max_len=max_len, causal=True, return_probs=True)
            else:
                out[f'ctx Tq {Tq}'] = cache.attend(q[Tq], scale, max_len=max_len, causal=True)
    return out


def test_c_long_sequences_panels_and_late_positions():
    """k_kv_qk_rows, k_kv_pv_rows and row_stats<4> (Tq 40: three panels of 16) and the 16-row route (Tq 1) at 3 x 8 heads x 2^20 tokens x
    256: 6 GiB per code buffer, head 8 starts at byte 2^31 and head 16 at byte 2^32.  Phase 1 holds the tokens at positions 0 ..; phase 2
    at P0 = capacity - 1024 .., the largest n * ldw the geometry has, against a twin of capacity 1024 that holds them at 0 ..: P0 is a
    multiple of 64 and of 1024, so token blocks and row_stats' columns per thread coincide and the masked blocks in front add +0."""
    c, kw = LC.C, cfg(block_size=LC.C['block'])
    B, Hq, H, D, cap, P0 = c['batch'], c['heads'], c['kv_heads'], c['head_dim'], c['capacity'], c['late_at']
    lens, n = c['lens'], max(c['lens'])
    make = lambda capacity: bfp_ops.HBFPKVCache(**LC.cache_kwargs(c, capacity=capacity), dtype=DTYPE, **kw)
    g = _gen(31)
    k, v = _tokens((B, H, n, D), g), _tokens((B, H, n, D), g)
    q = {Tq: _tokens((B, Hq, Tq, D), g) for Tq in c['tqs']}
    scale, counts = D ** -0.5, _i32(lens)
    hi = torch.tensor(lens, device=DEV)
    big = make(cap)
    assert big.k_codes.numel() == big.v_codes.numel() == 6 * LC.GiB
    # phase 1: early positions
    with torch.no_grad():
        big.starts.copy_(_i32(c['early_starts']))
        big.append(k, v, counts)
    got = _attends(big, q, scale, c['early_capacity'], c['tqs'])
    _untouched(big, torch.zeros_like(hi), hi, 0, 256, "C early")
    twin = make(c['early_capacity'])
    with torch.no_grad():
        twin.starts.copy_(_i32(c['early_starts']))
        twin.append(k, v, counts)
    want = _attends(twin, q, scale, c['early_capacity'], c['tqs'])
    for name in want:
        _same(got[name], want[name], f"C early: {name}")
    for b in range(B):
        _check_oracle(big, b, k[b:b + 1, :, :lens[b]], v[b:b + 1, :, :lens[b]], kw, "C early")
        with torch.no_grad():
            _same(big.keys(b), twin.keys(b), f"C early: keys({b})")
            _same(big.values(b), twin.values(b), f"C early: values({b})")
    early_k, early_ke, early_ve = big.k_codes[:, :, :256].clone(), big.k_exps[:, :, :256].clone(), big.v_exps[..., :256 // big.block].clone()
    del twin, got, want
    # phase 2: the same tokens at P0 ..
    with torch.no_grad():
        big.reset()
        big.lengths.fill_(P0)
        big.starts.fill_(P0)
        big.append(k, v, counts)
        assert big.lengths.tolist() == [P0 + s for s in lens]
        got = _attends(big, q, scale, cap, c['tqs'])
        got['scores'] = big.scores(q[1], cap)[..., P0:P0 + n]
        p = torch.zeros(B, Hq, 1, cap, dtype=DTYPE, device=DEV)
        p[..., P0:] = torch.softmax(_tokens((B, Hq, 1, c['late_capacity']), g).float(), -1).to(DTYPE)
        got['context'] = big.context(p)
    _untouched(big, torch.full_like(hi, P0), hi + P0, P0, P0 + 256, "C late", stale=256)
    assert torch.equal(big.k_codes[:, :, :256], early_k) and torch.equal(big.k_exps[:, :, :256], early_ke), "C late: the early keys changed"
    assert torch.equal(big.v_exps[..., :256 // big.block], early_ve), "C late: the early v_exps changed"
    twin = make(c['late_capacity'])
    with torch.no_grad():
        twin.append(k, v, counts)
        want = _attends(twin, q, scale, c['late_capacity'], c['tqs'])
        want['scores'] = twin.scores(q[1], c['late_capacity'])[..., :n]
        want['context'] = twin.context(p[..., P0:].contiguous())
    for name in want:
        if name.startswith('p '):
            assert not bool(got[name][..., :P0].view(torch.int16).any()), f"C late: {name} is not +0 below P0"
            _same(got[name][..., P0:], want[name], f"C late: {name}")
        else:
            _same(got[name], want[name], f"C late: {name}")
    _same(got['ctx Tq 1'], big.context(got['p Tq 1']), "C late: attend against context(p)")
    for name in CODES[:2]:
        assert torch.equal(getattr(big, name)[:, :, P0:P0 + 256], getattr(twin, name)[:, :, :256]), f"C late: {name}"
    assert torch.equal(big.v_codes[..., P0:P0 + 256], twin.v_codes[..., :256]), "C late: v_codes"
    assert torch.equal(big.v_exps[..., P0 // big.block:(P0 + 256) // big.block], twin.v_exps[..., :256 // big.block]), "C late: v_exps"
    b = B - 1                                                                     # (heads 16..23: past byte 2^32 of both code buffers)
    _bound_scores(got['scores'][b:b + 1, ..., :lens[b]], q[1][b:b + 1], k[b:b + 1, :, :lens[b]], kw)
    _bound_context(got['context'][b:b + 1], p[b:b + 1, ..., P0:], v[b:b + 1, :, :lens[b]], kw)


# ---- D: workspaces and p past 4 GiB -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", (False, True))
def test_d_workspaces_and_probs_past_4gib(causal):
    """attend's fp32 score rows (4.33 GB) and int32 block sums (4.39 GB) and a p of 2.2 GB at a cache of 0.7 GB: 33 sequences x 16
    heads x 16 rows x 128000 keys, kv_heads 2 (k_kv_bmm_dec kAtt GRP, k_kv_pv_split ATT GRP, k_kv_pv_combine)"""
    c, kw = LC.D, cfg(block_size=LC.D['block'])
    B, Hq, H, D, cap, Tq = c['batch'], c['heads'], c['kv_heads'], c['head_dim'], c['capacity'], c['tq']
    make = lambda batch: bfp_ops.HBFPKVCache(**LC.cache_kwargs(c, batch), dtype=DTYPE, **kw)
    g = _gen(41 + causal)
    lens = [200 - 6 * b for b in range(B)]                                        # distinct, 200 .. 8
    k, v, q = _tokens((B, H, 200, D), g), _tokens((B, H, 200, D), g), _tokens((B, Hq, Tq, D), g)
    counts, hi = _i32(lens), torch.tensor(lens, device=DEV)
    scale = D ** -0.5
    big = make(B)
    with torch.no_grad():
        big.append(k, v, counts)
        ctx, p = big.attend(q, scale, max_len=cap, causal=causal, return_probs=True)
        assert big._att_ws.numel() > LC.P32 and big._ws.numel() > LC.P32 and p.numel() * p.element_size() > LC.P31
        small = big.context(p[..., :256].contiguous())
        scores = big.scores(q, 256)
    _untouched(big, torch.zeros_like(hi), hi, 0, 256, "D")
    _same(ctx, small, "D: attend against context(p)")
    # p is +0 wherever a row sees no key: the whole of it from column 256 on as 64-bit words, the columns below under the mask
    assert not bool(p.view(torch.int64)[..., 256 // 4:].any()), "D: p is not +0 from column 256 on"
    head = p[..., :256]
    assert not bool((head.view(torch.int16) != 0)[(~_visible(hi, Tq, 256, causal)).expand_as(head)].any()), "D: p is not +0 at a key the row does not see"
    for s0 in range(0, B, c['slab']):
        s1, what = s0 + c['slab'], f"D causal {causal}, sequences {s0}..{s0 + c['slab'] - 1}"
        twin = make(c['slab'])
        with torch.no_grad():
            twin.append(k[s0:s1], v[s0:s1], counts[s0:s1])
            tctx, tp = twin.attend(q[s0:s1], scale, max_len=cap, causal=causal, return_probs=True)
        _same(ctx[s0:s1], tctx, what + ": ctx")
        _same(p[s0:s1], tp, what + ": p")
        _same_buffers(big, twin, s0, s1, what)
        with torch.no_grad():
            for i in range(c['slab']):
                _same(big.keys(s0 + i), twin.keys(i), f"{what}: keys({s0 + i})")
                _same(big.values(s0 + i), twin.values(i), f"{what}: values({s0 + i})")
        del twin, tctx, tp
    for b in (LC.holder(LC.per_sequence(c, 'score_ws'), LC.P31)[0], B - 1):       # the sequences whose score rows hold bytes 2^31 and 2^32
        _check_oracle(big, b, k[b:b + 1, :, :lens[b]], v[b:b + 1, :, :lens[b]], kw, "D")
    b = B - 1
    _bound_scores(scores[b:b + 1], q[b:b + 1], k[b:b + 1, :, :lens[b]], kw)
    _bound_context(ctx[b:b + 1], p[b:b + 1, ..., :256], v[b:b + 1, :, :lens[b]], kw)


# ---- E: the batched matmul's output past 4 GiB ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", LC.E['blocks'])
def test_e_bmm_output_past_4gib(block):
    """k_bmm_i8's store4 at ob + t N + n: 160 batches of [4080, 64] x [64, 4096] make 5.35 GB of bf16; batch 64 holds byte 2^31 and
    batch 128 byte 2^32.  Codes and exponents are drawn on the device; with K = 64 a sum has at most four block terms in block order,
    so the tile the launcher picks from B cannot change a bit and a slab of 8 batches is the reference"""
    e = LC.E
    B, T, N, K, m, slab = e['B'], e['T'], e['N'], e['K'], e['mant_bits'], e['slab']
    nb, cmax = K // block, (1 << m) - 1
    g = _gen(51 + block)
    draw = lambda rows, lo, hi, cols: torch.randint(lo, hi + 1, (rows, cols), dtype=torch.int8, device=DEV, generator=g)
    xc, xe, wc, we = draw(B * T, -cmax, cmax, K), draw(B * T, -3, 3, nb), draw(B * N, -cmax, cmax, K), draw(B * N, -3, 3, nb)
    (bx, tx), (bw, nw) = e['x_marker'], e['w_marker']
    xe[bx * T + tx, nb - 1] = -128                                                # the NaN block marker, one on each side
    we[bw * N + nw, 0] = -128
    run = lambda b0, b1: native.hbfp_bmm_i8((xc[b0 * T:b1 * T], xe[b0 * T:b1 * T]), (wc[b0 * N:b1 * N], we[b0 * N:b1 * N]), b1 - b0, T, N, K, m, m,
                                            block_size=block, out_dtype=DTYPE)
    out = run(0, B)
    assert out.shape == (B, T, N) and out.numel() * out.element_size() > LC.P32
    # the markers give NaN in exactly their row and their column; every other output is finite
    assert bool(torch.isnan(out[bx, tx]).all()) and bool(torch.isnan(out[bw, :, nw]).all())
    finite = 0
    for b0 in range(0, B, slab):
        _same(out[b0:b0 + slab], run(b0, b0 + slab), f"E block {block}: batches {b0}..{b0 + slab - 1}")
        finite += int(torch.isfinite(out[b0:b0 + slab]).sum())                    # (by slabs: isfinite of the whole would hold 3 x 5 GB)
    assert finite == out.numel() - N - T
    b = LC.holder(e['out_batch_bytes'], LC.P32)[0]                                # the batch that holds byte 2^32 against fp64
    xv = GC.values(xc[b * T:(b + 1) * T].int(), xe[b * T:(b + 1) * T].int(), m, block=block)
    wv = GC.values(wc[b * N:(b + 1) * N].int(), we[b * N:(b + 1) * N].int(), m, block=block)
    assert bool(torch.isfinite(out[b]).all())
    GC.elementwise_bound(out[b], xv @ wv.t(), xv.abs() @ wv.abs().t(), nb, DTYPE)


# ---- F (ii), (iii): more tiles and batches than a grid dimension ---------------------------------------------------------------------------------
@pytest.mark.parametrize("block", LC.F_BLOCKS)
def test_f_device_length_tiles_past_a_grid_dimension(block):
    """66000 tiles of 16 rows (33000 kv heads x group 2 x Tq 16): the second trip of k_kv_bmm_dec's loop over (head, tile), kDev GRP.
    The lengths are ragged, 0 included, and differ between tile y and tile y + 65535, so rows(No) and the empty-wave `continue`
    differ across the trips.  scores() only: attend() and context() refuse that many tiles"""
    c, kw = LC.with_block(LC.F_DEV, block), cfg(block_size=block)
    B, Hq, H, D, cap, Tq = c['batch'], c['heads'], c['kv_heads'], c['head_dim'], c['capacity'], c['tq']
    make = lambda batch: bfp_ops.HBFPKVCache(**LC.cache_kwargs(c, batch), dtype=DTYPE, **kw)
    g = _gen(71 + block)
    lens = LC.f_dev_lengths(B, cap)
    k, v, q = _tokens((B, H, cap, D), g), _tokens((B, H, cap, D), g), _tokens((B, Hq, Tq, D), g)
    counts, hi = _i32(lens), torch.tensor(lens, device=DEV)
    big = make(B)
    with torch.no_grad():
        big.append(k, v, counts)
        scores = big.scores(q)
    assert torch.equal(big.lengths.long(), hi)
    _untouched(big, torch.zeros_like(hi), hi, 0, 64, f"F device block {block}")
    assert torch.equal(torch.isinf(scores) & (scores < 0), ~_visible(hi, Tq, cap, False).expand_as(scores)), "-inf exactly from the length on"
    for s0 in range(0, B, c['slab']):
        s1, what = s0 + c['slab'], f"F device block {block}, sequences {s0}..{s0 + c['slab'] - 1}"
        twin = make(c['slab'])
        with torch.no_grad():
            twin.append(k[s0:s1], v[s0:s1], counts[s0:s1])
            _same(scores[s0:s1], twin.scores(q[s0:s1]), what + ": scores")
        assert torch.equal(big.lengths[s0:s1], twin.lengths), what
        _same_buffers(big, twin, s0, s1, what)
        del twin
    b = LC.GRID // 2                                                              # tile 65535, the first of the second trip, is its head 1
    _check_oracle(big, b, k[b:b + 1, :, :lens[b]], v[b:b + 1, :, :lens[b]], kw, f"F device block {block}")
    _bound_scores(scores[b:b + 1], q[b:b + 1], k[b:b + 1, :, :lens[b]], kw)


@pytest.mark.parametrize("block", LC.F_BLOCKS)
def test_f_bmm_batches_past_a_grid_dimension(block):
    """66000 batches of [16, 64] x [64, 16]: the second trip of k_bmm_i8's loop over blockIdx.y and of k_codes_t's over blockIdx.z"""
    f, kw = LC.F_BMM, cfg(block_size=block)
    B, T, N, K, m, slab, eps = f['B'], f['T'], f['N'], f['K'], f['mant_bits'], f['slab'], kw['epsilon']
    g = _gen(81 + block)
    x, w = _tokens((B, T, K), g), _tokens((B, K, N), g)

    def run(b0, b1):
        xq = native.act_codes(x[b0:b1].reshape((b1 - b0) * T, K), m, eps, None, block_size=block)
        wq = native.codes_transposed(w[b0:b1], block, m, eps)
        return xq, wq, native.hbfp_bmm_i8(xq, wq, b1 - b0, T, N, K, m, m, block_size=block, out_dtype=DTYPE)

    xq, wq, out = run(0, B)
    for b0 in range(0, B, slab):
        b1, what = b0 + slab, f"F bmm block {block}, batches {b0}..{b0 + slab - 1}"
        txq, twq, tout = run(b0, b1)
        for i in (0, 1):
            assert torch.equal(xq[i][b0 * T:b1 * T], txq[i]), what + ": x codes / exponents"
            assert torch.equal(wq[i][b0:b1], twq[i]), what + ": w codes / exponents (codes_transposed)"
        _same(out[b0:b1], tout, what)
    b = LC.GRID                                                                   # the first batch of the second trip
    _bound(out[b:b + 1], x[b:b + 1], w[b:b + 1], kw, K // block, DTYPE)
