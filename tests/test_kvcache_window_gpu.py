"""GPU tests of the first visible key per row on the HBFP KV cache (bfp_ops.HBFPKVCache(window=W, starts=True), csrc/bfpq_kvcache.hip,
DESIGN 5o): left-padded batches and sliding-window attention in attend(), on both its routes.  Row t of sequence b sees the keys
lo <= n < hi, hi what it saw before and lo = max(0, starts[b], v(t) - W).  Everything is pinned bit for bit (assert_bits_equal, any NaN
matching any NaN) against code that existed before -- the attend() of a cache without window / starts whose masked keys score so low
that expf is exactly +0 there, and context(p) -- except the softmax itself, which is measured against float64 next to torch's own.
Shapes: B 3, 2 heads (and 4 heads over 2 kv heads), D 64 / 64 / 32 at blocks 64 / 32 / 16, capacity 320, lengths (200, 70, 200)."""
import pytest
import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)
B, H, CAP = 3, 2, 320
LENS = (200, 70, 200)
DBLK = ((64, 64), (64, 32), (32, 16))
# every dtype with every (D, block), the two mantissa widths alternating (a Latin square, as tests/test_kvcache_prompt_gpu.py)
CASES = [(dn, D, blk, (3, 7)[(i + j) % 2]) for i, dn in enumerate(DT) for j, (D, blk) in enumerate(DBLK)]
CASE_IDS = [f"{dn}-d{D}-b{blk}-m{m}" for dn, D, blk, m in CASES]
# the plain heads for every case, 4 query heads over 2 kv heads for every other one
GROUPED = [c + (2, None) for c in CASES] + [c + (4, 2) for c in CASES[::2]]
GROUPED_IDS = CASE_IDS + [i + "-gqa" for i in CASE_IDS[::2]]
# a bound inside the first tile, on a chunk boundary, inside a block of 16 / 32, in a later slice; start == len; a single visible key
STARTS = ((0, 37, 130), (64, 70, 199))
WINDOWS = (1, 16, 50, 64, 100, 400)                                  # 400: larger than any length
MODES = [(s, None) for s in STARTS] + [(None, w) for w in WINDOWS] + [(STARTS[0], 50), (STARTS[1], 100)]
TQS, LONG_TQS = (1, 3, 16), (17, 48, 80)                             # up to 16 rows; panels (prompt_rows 16 and 32)
PANELS = (16, 32)
CPS = (0, 1, 2)
MAX_LENS = (CAP, 256)
ULP_HALF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # the spacing of the dtype at 1/2
TINY = {dt: torch.finfo(dt).tiny for dt in DT.values()}
Q0, KMASK = 64.0, -512.0            # coordinate 0 of every query row, and of the key row that stands for a masked token in a twin
KTINY = 2.0 ** -14                  # the least normal number of fp16


def cfg(**kw):
    base = dict(mant_bits=7, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _tokens(b, h, S, D, dtype, seed):
    """the inputs of tests/test_kvcache_attend_gpu.py: magnitudes over many binades along the tokens"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.randn(b, h, S, D, generator=g) * torch.exp2(torch.randint(-6, 4, (b, h, S, 1), generator=g).float())).to(dtype).to(DEV)
    return mk(), mk()


def _queries(heads, Tq, D, dtype, seed, batch=B):
    """query rows with the power of two Q0 at coordinate 0: above every other magnitude, so it is a code of its block at any mant_bits"""
    q = _tokens(batch, heads, Tq, D, dtype, seed)[0]
    q[..., 0] = Q0
    return q


def _cache(dtype, D, kw, k, v, lens=LENS, heads=H, kv_heads=None, starts=None, window=None, cap=CAP, **mode):
    """a device-length cache holding the first lens[b] tokens of k, v [B, kv_heads, S, D]; starts: a tuple (then cache.starts is set)"""
    c = bfp_ops.HBFPKVCache(len(lens), heads, D, cap, dtype=dtype, device_lengths=True, kv_heads=kv_heads, window=window,
                            starts=starts is not None, **mode, **kw)
    with torch.no_grad():
        c.append(k[:, :, :max(lens)].contiguous(), v[:, :, :max(lens)].contiguous(), _i32(*lens))
        if starts is not None:
            c.starts.copy_(_i32(*starts))
    return c


def _bounds(lens, Tq, max_len, causal, starts, window):
    """(lo, hi), each [B][Tq]: the semantics of the class docstring, restated"""
    lo, hi = [], []
    for b, n in enumerate(lens):
        v = [n - Tq + t + 1 if causal else n for t in range(Tq)]
        hi.append([min(max(x, 0), min(n, max_len)) for x in v])
        lo.append([max(0, starts[b] if starts else 0, x - window if window else 0) for x in v])
    return lo, hi


def _visible(lo, hi, max_len):
    """[B, 1, Tq, max_len] bool"""
    n = torch.arange(max_len, device=DEV).view(1, 1, -1)
    lo, hi = (torch.tensor(x, device=DEV).unsqueeze(-1) for x in (lo, hi))
    return ((n >= lo) & (n < hi)).unsqueeze(1)


def _plus_zero(p, vis, what):
    hidden = p[(~vis).expand_as(p)]
    assert not bool(hidden.any()) and not bool(torch.signbit(hidden).any()), f"{what}: p is not +0 at a key the row does not see"


def _tiles(Tq):
    return [(i, min(i + 16, Tq)) for i in range(0, Tq, 16)]


def _context_per_tile(ref, p):
    return torch.cat([ref.context(p[:, :, i:j].contiguous()) for i, j in _tiles(p.shape[2])], 2)


class Bench:
    """one (dtype, D, block, mant_bits, heads, kv_heads): the tokens, a plain cache (the parent's routes) and, per mode, three caches that
    differ in chunks_per_split and prompt_rows"""
    VARIANTS = ((0, 16), (1, 32), (2, 16))                           # (chunks_per_split, prompt_rows)

    def __init__(self, dname, D, block, mant, heads, kvh):
        self.dtype, self.D, self.block, self.heads, self.kvh = DT[dname], D, block, heads, kvh
        self.kw = cfg(mant_bits=mant, block_size=block)
        self.scale = D ** -0.5
        self.k, self.v = _tokens(B, kvh or heads, max(LENS), D, self.dtype, 1000 * block + 10 * mant + heads)
        self.ref = self.make()
        self.what = f"{dname} D {D} block {block} mant_bits {mant} heads {heads}/{kvh or heads}"
        self._modes = {}

    def make(self, k=None, **mode):
        return _cache(self.dtype, self.D, self.kw, self.k if k is None else k, self.v, heads=self.heads, kv_heads=self.kvh, **mode)

    def mode(self, starts, window):
        key = (starts, window)
        if key not in self._modes:
            self._modes[key] = [self.make(starts=starts, window=window, chunks_per_split=cps, prompt_rows=P) for cps, P in self.VARIANTS]
        return self._modes[key]

    def q(self, Tq):
        return _queries(self.heads, Tq, self.D, self.dtype, 7 + Tq)


_BENCHES = {}


def _bench(*key):
    if key not in _BENCHES:
        _BENCHES.clear()                                             # (one at a time: the caches of a finished case are dropped)
        _BENCHES[key] = Bench(*key)
    return _BENCHES[key]


# ---- 1. against the parent's code ---------------------------------------------------------------------------------------------------------
def _masked_twin(bench, twin, lo_of_b):
    """the twin's cache refilled with K whose tokens n < lo_of_b[b] are the row KMASK e_0 (K is quantized per token: no other key's
    codes move; V is untouched).  Where D holds several blocks, the first coordinate of every further block is KTINY, not zero: fp16
    rounds the epsilon 1e-8 to zero, and an all-zero block is then a NaN block"""
    k = bench.k.clone()
    for b, lo in enumerate(lo_of_b):
        k[b, :, :lo] = 0
        k[b, :, :lo, ::bench.block] = KTINY
        k[b, :, :lo, 0] = KMASK
    twin.reset()
    twin.append(k, bench.v, _i32(*LENS))


def _premise(twin, q, scale, max_len, vis_rows, masked_rows, what):
    """with the twin's own scores(): every masked key lies at least 200 below the row's maximum over its visible keys, so expf of the
    difference is exactly +0 in fp32.  vis_rows / masked_rows [B, 1, Tq, max_len] bool, rows that are not compared all False in both"""
    s = torch.cat([twin.scores(q[:, :, i:j].contiguous(), max_len) for i, j in _tiles(q.shape[2])], 2).float() * scale
    top = s.masked_fill(~vis_rows.expand_as(s), float('-inf')).amax(-1, keepdim=True)
    gap = (top - s)[masked_rows.expand_as(s)]
    assert gap.numel() == 0 or float(gap.min()) >= 200.0, f"{what}: a masked key scores only {float(gap.min())} below the row's maximum"


def _crossing_row(lo, Tq):
    """a row whose lo lies in another 64-key tile than the row before it in the same tile of 16 rows, or None"""
    for t in range(1, Tq):
        if t % 16 and any(l[t] // 64 != l[t - 1] // 64 for l in lo):
            return t
    return None


@pytest.mark.parametrize("dname,D,block,mant,heads,kvh", GROUPED, ids=GROUPED_IDS)
def test_rows_are_the_rows_of_a_cache_whose_masked_keys_score_low(dname, D, block, mant, heads, kvh):
    """the law that decides the route: a plain twin holds, in place of the keys below lo, key rows that score at least 200 below the
    row's maximum; there expf is exactly +0, so the twin's attend() -- the parent's code -- must give the new route's p and context bit
    for bit.  Non-causal with starts alone: all rows at once.  Otherwise the mask differs per row: the twin is refilled per tested row
    (the first, the last, one whose lo crosses a 64-key tile inside a 16-row tile) and that row is compared"""
    bench = _bench(dname, D, block, mant, heads, kvh)
    dtype, scale = bench.dtype, bench.scale
    twins = [bench.make(chunks_per_split=cps, prompt_rows=P) for cps, P in Bench.VARIANTS]
    crossed = 0
    with torch.no_grad():
        for mi, (starts, window) in enumerate(MODES):
            for ci, causal in enumerate((False, True)):
                for ti, Tq in enumerate(TQS + LONG_TQS):
                    vi = (mi + ci + ti) % 3
                    cache, twin, max_len = bench.mode(starts, window)[vi], twins[vi], MAX_LENS[(mi + ti) % 2]
                    q = bench.q(Tq)
                    what = f"{bench.what} starts {starts} window {window} causal {causal} Tq {Tq} max_len {max_len} variant {Bench.VARIANTS[vi]}"
                    lo, hi = _bounds(LENS, Tq, max_len, causal, starts, window)
                    ctx, p = cache.attend(q, scale, max_len=max_len, causal=causal, return_probs=True)
                    cross = _crossing_row(lo, Tq)
                    crossed += cross is not None
                    rows = [None] if not causal and window is None else sorted({0, Tq - 1} | ({cross} if cross is not None else set()))
                    for t in rows:
                        ts = slice(None) if t is None else slice(t, t + 1)
                        _masked_twin(bench, twin, [l[0 if t is None else t] for l in lo])
                        sel = torch.zeros(B, 1, Tq, 1, dtype=torch.bool, device=DEV)
                        sel[:, :, ts] = True
                        sel &= torch.tensor([[[[l[i] < h[i]] for i in range(Tq)]] for l, h in zip(lo, hi)], device=DEV)   # rows that see a key
                        vis = _visible(lo, hi, max_len)
                        below = torch.arange(max_len, device=DEV).view(1, 1, 1, -1) < torch.tensor(lo, device=DEV).view(B, 1, Tq, 1)
                        _premise(twin, q, scale, max_len, vis & sel, below & sel & _visible([[0] * Tq] * B, hi, max_len), what)
                        wctx, wp = twin.attend(q, scale, max_len=max_len, causal=causal, return_probs=True)
                        rows_sel = sel.expand(B, heads, Tq, 1).squeeze(-1)
                        assert bool(rows_sel.any()) or starts == STARTS[1], what
                        assert_bits_equal(bits(p[rows_sel]), bits(wp[rows_sel]), dtype, what + f": p, row {t}")
                        assert_bits_equal(bits(ctx[rows_sel]), bits(wctx[rows_sel]), dtype, what + f": context, row {t}")
    assert crossed >= 4, bench.what


# ---- 2 and 3a. context(p), +0 outside the range, and nothing depends on the slice or the panel ---------------------------------------------
@pytest.mark.parametrize("dname,D,block,mant,heads,kvh", GROUPED, ids=GROUPED_IDS)
def test_context_of_p_plus_zero_and_invariance(dname, D, block, mant, heads, kvh):
    """ctx == context(p) (per 16 rows where there are more), the call without return_probs gives the same ctx, p is +0 outside
    [lo, hi), and every chunks_per_split / prompt_rows gives the first one's bits"""
    bench = _bench(dname, D, block, mant, heads, kvh)
    dtype, scale = bench.dtype, bench.scale
    with torch.no_grad():
        for starts, window in MODES:
            caches = bench.mode(starts, window)
            for causal in (False, True):
                for Tq in TQS + LONG_TQS:
                    q = bench.q(Tq)
                    for max_len in MAX_LENS:
                        lo, hi = _bounds(LENS, Tq, max_len, causal, starts, window)
                        vis = _visible(lo, hi, max_len)
                        first = None
                        for cache, variant in zip(caches, Bench.VARIANTS):
                            what = f"{bench.what} starts {starts} window {window} causal {causal} Tq {Tq} max_len {max_len} variant {variant}"
                            ctx, p = cache.attend(q, scale, max_len=max_len, causal=causal, return_probs=True)
                            if first is None:
                                first = bits(ctx), bits(p)
                                assert ctx.shape == (B, heads, Tq, D) and p.shape == (B, heads, Tq, max_len) and ctx.dtype == p.dtype == dtype
                                want = cache.context(p) if Tq <= 16 else _context_per_tile(bench.ref, p)
                                assert_bits_equal(first[0], bits(want), dtype, what + ": attend against context(p)")
                                _plus_zero(p, vis, what)
                            else:
                                assert_bits_equal(bits(ctx), first[0], dtype, what + ": against the first variant")
                                assert_bits_equal(bits(p), first[1], dtype, what + ": p against the first variant")
                            alone = cache.attend(q, scale, max_len=max_len, causal=causal)
                            assert_bits_equal(bits(alone), first[0], dtype, what + ": without return_probs")


# ---- 2b. max_len below the lengths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,D,block,mant,heads,kvh", GROUPED, ids=GROUPED_IDS)
def test_max_len_cuts_the_range_from_above(dname, D, block, mant, heads, kvh):
    """max_len 128 lies below the lengths 200: hi is cut by it, a start of 130 or 199 lies at or past it (the row sees nothing) and a
    window ends past it (row t sees what is left of [v - W, v) below 128, nothing for most windows).  p is +0 outside
    [lo, min(hi, 128)), ctx == context(p), every variant gives the first one's bits, and for non-causal starts the rows are the twin's"""
    bench = _bench(dname, D, block, mant, heads, kvh)
    dtype, scale, max_len = bench.dtype, bench.scale, 128
    twins = [bench.make(chunks_per_split=cps, prompt_rows=P) for cps, P in Bench.VARIANTS]
    empty_and_seen = [False, False]
    with torch.no_grad():
        for starts, window in MODES:
            caches = bench.mode(starts, window)
            for causal in (False, True):
                for Tq in (3, 16, 48):
                    q = bench.q(Tq)
                    lo, hi = _bounds(LENS, Tq, max_len, causal, starts, window)
                    assert max(max(h) for h in hi) == max_len
                    vis = _visible(lo, hi, max_len)
                    for b in (0, 2):                                 # the sequences of 200 tokens
                        empty_and_seen[0] |= any(l >= h > 0 for l, h in zip(lo[b], hi[b]))
                        empty_and_seen[1] |= any(0 < l < h for l, h in zip(lo[b], hi[b]))
                    first = None
                    for vi, (cache, variant) in enumerate(zip(caches, Bench.VARIANTS)):
                        what = f"{bench.what} starts {starts} window {window} causal {causal} Tq {Tq} max_len {max_len} variant {variant}"
                        ctx, p = cache.attend(q, scale, max_len=max_len, causal=causal, return_probs=True)
                        if first is None:
                            first = bits(ctx), bits(p)
                            assert_bits_equal(first[0], bits(_context_per_tile(bench.ref, p)), dtype, what + ": attend against context(p)")
                            _plus_zero(p, vis, what)
                        else:
                            assert_bits_equal(bits(ctx), first[0], dtype, what + ": against the first variant")
                            assert_bits_equal(bits(p), first[1], dtype, what + ": p against the first variant")
                        assert_bits_equal(bits(cache.attend(q, scale, max_len=max_len, causal=causal)), first[0], dtype, what + ": without return_probs")
                        if not causal and window is None:
                            _masked_twin(bench, twins[vi], [l[0] for l in lo])
                            sel = torch.tensor([[[[l[i] < h[i]] for i in range(Tq)]] for l, h in zip(lo, hi)], device=DEV)
                            below = torch.arange(max_len, device=DEV).view(1, 1, 1, -1) < torch.tensor(lo, device=DEV).view(B, 1, Tq, 1)
                            _premise(twins[vi], q, scale, max_len, vis & sel, below & sel & _visible([[0] * Tq] * B, hi, max_len), what)
                            wctx, wp = twins[vi].attend(q, scale, max_len=max_len, return_probs=True)
                            rows_sel = sel.expand(B, heads, Tq, 1).squeeze(-1)
                            assert_bits_equal(bits(p[rows_sel]), bits(wp[rows_sel]), dtype, what + ": p against the twin")
                            assert_bits_equal(bits(ctx[rows_sel]), bits(wctx[rows_sel]), dtype, what + ": context against the twin")
    assert all(empty_and_seen), bench.what


# ---- 3b-d. rows of a long call, the modes that mask nothing, grouped heads ------------------------------------------------------------------
@pytest.mark.parametrize("dname,D,block,mant", CASES, ids=CASE_IDS)
def test_rows_of_a_long_call_are_the_16_row_call(dname, D, block, mant):
    """rows i .. i + 15 of a long attend() are the 16-row attend() of those rows: every tile without causal (lo and hi do not depend on
    the row then), the last 16 rows with it (the 16-row call takes its rows to be the last tokens held)"""
    bench = _bench(dname, D, block, mant, 2, None)
    dtype, scale = bench.dtype, bench.scale
    with torch.no_grad():
        for starts, window in MODES[::3] + MODES[-2:]:
            long, short = bench.mode(starts, window)[1], bench.mode(starts, window)[0]
            for Tq in LONG_TQS:
                q = bench.q(Tq)
                for causal in (False, True):
                    what = f"{bench.what} starts {starts} window {window} causal {causal} Tq {Tq}"
                    ctx, p = long.attend(q, scale, max_len=256, causal=causal, return_probs=True)
                    for i, j in ([(Tq - 16, Tq)] if causal else [(i, j) for i, j in _tiles(Tq)]):
                        wctx, wp = short.attend(q[:, :, i:j].contiguous(), scale, max_len=256, causal=causal, return_probs=True)
                        assert_bits_equal(bits(ctx[:, :, i:j]), bits(wctx), dtype, what + f": rows {i}..{j - 1}")
                        assert_bits_equal(bits(p[:, :, i:j]), bits(wp), dtype, what + f": p of rows {i}..{j - 1}")


@pytest.mark.parametrize("dname,D,block,mant,heads,kvh", GROUPED, ids=GROUPED_IDS)
def test_starts_of_zero_and_a_window_past_every_length_are_the_plain_cache(dname, D, block, mant, heads, kvh):
    bench = _bench(dname, D, block, mant, heads, kvh)
    dtype, scale = bench.dtype, bench.scale
    plain = bench.make(prompt_rows=32)
    with torch.no_grad():
        for starts, window in (((0, 0, 0), None), (None, 400), ((0, -5, 0), 400)):   # (a negative start counts as 0)
            cache = bench.make(starts=starts, window=window, prompt_rows=32)
            for Tq in (1, 16, 48):
                q = bench.q(Tq)
                for causal in (False, True):
                    what = f"{bench.what} starts {starts} window {window} causal {causal} Tq {Tq}"
                    got, want = (c.attend(q, scale, causal=causal, return_probs=True) for c in (cache, plain))
                    assert_bits_equal(bits(got[0]), bits(want[0]), dtype, what)
                    assert_bits_equal(bits(got[1]), bits(want[1]), dtype, what + ": p")


@pytest.mark.parametrize("dname,D,block,mant", CASES[::2], ids=CASE_IDS[::2])
def test_grouped_cache_has_the_bits_of_the_repeated_twin(dname, D, block, mant):
    dtype, kvh, heads, scale = DT[dname], 2, 4, D ** -0.5
    g = heads // kvh
    kw = cfg(mant_bits=mant, block_size=block)
    k, v = _tokens(B, kvh, max(LENS), D, dtype, 31 + block)
    with torch.no_grad():
        for mi, (starts, window) in enumerate(MODES):
            mode = dict(starts=starts, window=window, prompt_rows=PANELS[mi % 2], chunks_per_split=CPS[mi % 3])
            cache = _cache(dtype, D, kw, k, v, heads=heads, kv_heads=kvh, **mode)
            twin = _cache(dtype, D, kw, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), heads=heads, **mode)
            for Tq in (3, 16, 17, 80):                               # (17 and 80 at g = 2: tiles that straddle two query heads)
                q = _queries(heads, Tq, D, dtype, 33 + Tq)
                for causal in (False, True):
                    got, want = (c.attend(q, scale, max_len=256, causal=causal, return_probs=True) for c in (cache, twin))
                    what = f"{dname} D {D} block {block} mant_bits {mant} starts {starts} window {window} Tq {Tq} causal {causal}"
                    assert_bits_equal(bits(got[0]), bits(want[0]), dtype, what)
                    assert_bits_equal(bits(got[1]), bits(want[1]), dtype, what + ": p")


# ---- 4. rows that see nothing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,D,block,mant,heads,kvh", GROUPED, ids=GROUPED_IDS)
def test_rows_that_see_nothing(dname, D, block, mant, heads, kvh):
    """start >= hi (the second sequence of STARTS[1]: start == len) and the pad rows of a causal prompt, whose own position is below
    start: p is all +0 and the context what context() makes of a p of zeros -- NaN in fp16, whose epsilon 1e-8 rounds to zero, as
    today"""
    bench = _bench(dname, D, block, mant, heads, kvh)
    dtype, scale = bench.dtype, bench.scale
    seen_pad_rows = False
    with torch.no_grad():
        for starts, window in ((STARTS[1], None), (STARTS[0], None), (STARTS[1], 100)):
            for cache, variant in zip(bench.mode(starts, window), Bench.VARIANTS):
                for Tq in (3, 16, 48, 80):
                    q = bench.q(Tq)
                    for causal in (False, True):
                        what = f"{bench.what} starts {starts} window {window} causal {causal} Tq {Tq} variant {variant}"
                        lo, hi = _bounds(LENS, Tq, CAP, causal, starts, window)
                        empty = torch.tensor([[l[t] >= h[t] for t in range(Tq)] for l, h in zip(lo, hi)], device=DEV)   # [B, Tq]
                        if not bool(empty.any()):
                            continue
                        seen_pad_rows |= causal and bool((empty.any(1) & ~empty.all(1)).any())
                        rows = empty.unsqueeze(1).expand(B, heads, Tq)
                        ctx, p = cache.attend(q, scale, causal=causal, return_probs=True)
                        assert not bool(p[rows].any()) and not bool(torch.signbit(p[rows]).any()), what + ": p of a row that sees nothing"
                        zeros = _context_per_tile(bench.ref, torch.zeros_like(p))
                        assert_bits_equal(bits(ctx[rows]), bits(zeros[rows]), dtype, what + ": the context of a row that sees nothing")
                        if dtype == torch.float16:
                            assert bool(torch.isnan(ctx[rows]).all()), what
    assert seen_pad_rows, bench.what


# ---- 5. the softmax against float64 -------------------------------------------------------------------------------------------------------
def _rel_err(p, truth, ok):
    return float(((p.double() - truth).abs() / truth)[ok].max())


@pytest.mark.parametrize("dname,D,block,mant", CASES, ids=CASE_IDS)
def test_softmax_is_as_accurate_as_torchs(dname, D, block, mant):
    """the criterion of tests/test_kvcache_attend_gpu.py unchanged: the largest relative error of p over the visible keys whose true
    probability is a normal number of the dtype is at most twice that of torch.softmax on the same scores masked to [lo, hi), and the
    rows sum to 1 within rows * ULP_HALF"""
    bench = _bench(dname, D, block, mant, 2, None)
    dtype, scale = bench.dtype, bench.scale
    with torch.no_grad():
        for starts, window in MODES:
            cache = bench.mode(starts, window)[1]
            for Tq in (3, 16, 48):
                q = _tokens(B, 2, Tq, D, dtype, 17 + Tq)[0]
                for max_len in MAX_LENS:
                    for causal in (False, True):
                        what = f"{bench.what} starts {starts} window {window} Tq {Tq} max_len {max_len} causal {causal}"
                        lo, hi = _bounds(LENS, Tq, max_len, causal, starts, window)
                        vis = _visible(lo, hi, max_len)
                        s = torch.cat([bench.ref.scores(q[:, :, i:j].contiguous(), max_len) for i, j in _tiles(Tq)], 2).float() * scale
                        s = s.masked_fill(~vis.expand_as(s), float('-inf'))
                        _, p = cache.attend(q, scale, max_len=max_len, causal=causal, return_probs=True)
                        seen = vis.any(-1, keepdim=True).expand_as(s)                  # (rows that see no key: p is all +0, no softmax)
                        truth = torch.softmax(s.double(), -1)
                        torchs = torch.softmax(s, -1).to(dtype)
                        ok = vis.expand_as(s) & seen & (truth > TINY[dtype])
                        assert bool(ok.any()), what
                        ours, theirs = _rel_err(p, truth, ok), _rel_err(torchs, truth, ok)
                        print(f"softmax {what}: kernel {ours:.3e} torch {theirs:.3e}")
                        assert ours <= 2 * theirs, f"{what}: kernel {ours:.3e}, torch {theirs:.3e}"
                        rows = vis.sum(-1).expand(B, 2, Tq)
                        err = (p.double().sum(-1) - 1).abs()
                        assert bool((err[rows > 0] <= rows[rows > 0] * ULP_HALF[dtype]).all()), f"{what}: a row of p does not sum to 1"


# ---- 6. NaN containment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,D,block,mant", CASES, ids=CASE_IDS)
def test_nan_below_every_rows_first_key(dname, D, block, mant):
    """one NaN in V in a block below every row's lo (token 5 of the first sequence, whose start is 64) poisons the context exactly as
    context(p) does: that block of V is a NaN block and context() walks every block of the sequence.  One NaN in a key below lo changes
    nothing"""
    dtype, scale, heads, kvh = DT[dname], D ** -0.5, 4, 2
    kw = cfg(mant_bits=mant, block_size=block)
    k, v = _tokens(B, kvh, max(LENS), D, dtype, 51 + block)
    vbad, kbad = v.clone(), k.clone()
    vbad[0, 1, 5, 3] = float('nan')
    kbad[0, 1, 5, 2] = float('nan')
    hit = torch.zeros(B, heads, 1, D, dtype=torch.bool, device=DEV)
    hit[0, 2:4, :, 3] = True                                         # kv head 1 serves query heads 2 and 3
    with torch.no_grad():
        for starts, window in ((STARTS[1], None), (STARTS[1], 16)):
            for cps in (1, 0):                                       # (1: the first slice lies below every lo of the sequence and is skipped)
                mode = dict(heads=heads, kv_heads=kvh, starts=starts, window=window, chunks_per_split=cps, prompt_rows=32)
                clean, badv, badk = (_cache(dtype, D, kw, kk, vv, **mode) for kk, vv in ((k, v), (k, vbad), (kbad, v)))
                for Tq in (3, 48):
                    q = _queries(heads, Tq, D, dtype, 53 + Tq)
                    for causal in (False, True):
                        what = f"{dname} D {D} block {block} mant_bits {mant} starts {starts} window {window} cps {cps} Tq {Tq} causal {causal}"
                        want_ctx, want_p = clean.attend(q, scale, causal=causal, return_probs=True)
                        ctx, p = badv.attend(q, scale, causal=causal, return_probs=True)
                        assert_bits_equal(bits(p), bits(want_p), dtype, what + ": p does not read V")
                        assert_bits_equal(bits(ctx), bits(_context_per_tile(badv, p)), dtype, what + ": NaN in V against context(p)")
                        if dtype != torch.float16:                   # (fp16: epsilon rounds to 0 and an all-zero block of p is a NaN block too)
                            assert torch.equal(torch.isnan(ctx), hit.expand_as(ctx)), what
                        ctx, p = badk.attend(q, scale, causal=causal, return_probs=True)
                        assert_bits_equal(bits(ctx), bits(want_ctx), dtype, what + ": NaN in a key below lo")
                        assert_bits_equal(bits(p), bits(want_p), dtype, what + ": NaN in a key below lo, p")


# ---- 7. a row longer than the walker's stride -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq", (1, 16))
def test_the_second_stride_is_the_first_one_a_thread_uses(Tq):
    """length 1100 with start 1030: the threads that own columns 1024 .. 1099 skip their first stride of row_stats.  Laws 1 and 2"""
    dtype, D, cap, n, start = torch.bfloat16, 64, 1152, 1100, 1030
    kw = cfg()
    scale = D ** -0.5
    k, v = _tokens(1, 1, n, D, dtype, 71)
    q = _queries(1, Tq, D, dtype, 72, batch=1)
    kt = k.clone()
    kt[:, :, :start] = 0
    kt[:, :, :start, 0] = KMASK
    cache = _cache(dtype, D, kw, k, v, lens=(n,), heads=1, starts=(start,), cap=cap)
    twin = _cache(dtype, D, kw, kt, v, lens=(n,), heads=1, cap=cap)
    below = torch.arange(cap, device=DEV).view(1, 1, 1, -1) < start
    every = torch.ones(1, 1, Tq, 1, dtype=torch.bool, device=DEV)
    with torch.no_grad():
        _premise(twin, q, scale, cap, _visible([[start] * Tq], [[n] * Tq], cap) & every, below & every, "length 1100")
        ctx, p = cache.attend(q, scale, return_probs=True)
        wctx, wp = twin.attend(q, scale, return_probs=True)
        assert_bits_equal(bits(p), bits(wp), dtype, f"Tq {Tq}: p against the twin")
        assert_bits_equal(bits(ctx), bits(wctx), dtype, f"Tq {Tq}: context against the twin")
        for causal in (False, True):
            ctx, p = cache.attend(q, scale, causal=causal, return_probs=True)
            assert_bits_equal(bits(ctx), bits(cache.context(p)), dtype, f"Tq {Tq} causal {causal}: attend against context(p)")
            assert_bits_equal(bits(cache.attend(q, scale, causal=causal)), bits(ctx), dtype, f"Tq {Tq} causal {causal}: without return_probs")
            lo, hi = _bounds((n,), Tq, cap, causal, (start,), None)
            _plus_zero(p, _visible(lo, hi, cap), f"Tq {Tq} causal {causal}")


# ---- 8. captured steps, memory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname,D,block", (('fp32', 64, 64), ('bf16', 32, 16)))
def test_captured_decode_step_with_a_window(dname, D, block):
    dtype, steps, start, scale = DT[dname], 5, (0, 62, 126), D ** -0.5
    kw = cfg(block_size=block)
    k, v = _tokens(B, H, max(start) + steps, D, dtype, 81 + block)
    qs = torch.stack([_queries(H, 1, D, dtype, 82 + i) for i in range(steps)])
    cache, twin = (_cache(dtype, D, kw, k, v, lens=start, window=50) for _ in range(2))
    ik, iv, iq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(3))

    def step():
        cache.append(ik, iv)
        return cache.attend(iq, scale)

    with torch.no_grad():
        step()                                                       # warm-up: code objects, the exponent window table, the workspaces
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
            assert_bits_equal(bits(ctx), bits(want), dtype, f"{dname} block {block} replay {i}")
    assert cache.overflow.item() == 0


@pytest.mark.parametrize("dname,D,block", (('fp32', 64, 64), ('bf16', 32, 16)))
def test_captured_prompt_chunk_follows_starts_between_replays(dname, D, block):
    dtype, C, steps, start, scale = DT[dname], 32, 5, (0, 70, 10), D ** -0.5
    pads = ((0, 37, 5), (3, 80, 0))                                  # cache.starts for replays 0-1, then for replays 2-4
    kw = cfg(block_size=block)
    mk = lambda: bfp_ops.HBFPKVCache(B, 4, D, CAP, dtype=dtype, device_lengths=True, kv_heads=2, prompt_rows=16, starts=True, **kw)
    cache, twin, stale = mk(), mk(), mk()
    k, v = _tokens(B, 2, 70 + C * steps, D, dtype, 91 + block)
    qs = torch.stack([_queries(4, C, D, dtype, 92 + i) for i in range(steps)])
    ik, iv = (torch.zeros(B, 2, C, D, dtype=dtype, device=DEV) for _ in range(2))
    iq = torch.zeros(B, 4, C, D, dtype=dtype, device=DEV)

    def step():
        cache.append(ik, iv)
        return cache.attend(iq, scale, causal=True)

    with torch.no_grad():
        cache.prepare_attend()
        step()                                                       # warm-up: code objects, the exponent window table
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx = step()
        cache.reset()                                                # undo the warm-up and capture-time appends; starts are zero again
        assert cache.starts.tolist() == [0, 0, 0]
        for c in (cache, twin, stale):
            c.append(k[:, :, :70].contiguous(), v[:, :, :70].contiguous(), _i32(*start))
            c.starts.copy_(_i32(*pads[0]))
        differed = False
        for i in range(steps):
            s = slice(70 + C * i, 70 + C * (i + 1))
            ik.copy_(k[:, :, s]); iv.copy_(v[:, :, s]); iq.copy_(qs[i])
            if i == 2:
                cache.starts.copy_(_i32(*pads[1]))                   # written between two replays: the kernels read it at launch
                twin.starts.copy_(_i32(*pads[1]))
            graph.replay()
            twin.append(ik, iv)
            stale.append(ik, iv)
            want, old = twin.attend(iq, scale, causal=True), stale.attend(iq, scale, causal=True)
            assert cache.lengths.tolist() == twin.lengths.tolist() == [n + C * (i + 1) for n in start], f"replay {i}"
            assert_bits_equal(bits(ctx), bits(want), dtype, f"{dname} block {block} replay {i}")
            differed |= i >= 2 and not torch.equal(torch.nan_to_num(ctx), torch.nan_to_num(old))
        assert differed, "the change of cache.starts did not show"
    assert cache.overflow.item() == twin.overflow.item() == 0


def test_no_allocation_after_prepare_attend():
    dtype, D, P = torch.bfloat16, 64, 32
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **cfg())
    cache = mm.kv_cache(B, 4, D, CAP, dtype=dtype, device_lengths=True, kv_heads=2, prompt_rows=P, window=50, starts=True)
    plain = mm.kv_cache(B, 4, D, CAP, dtype=dtype, device_lengths=True, kv_heads=2, prompt_rows=P)
    assert cache.nbytes() == plain.nbytes() and cache._rows_ws is None and cache._att_ws is None
    k, v = _tokens(B, 2, 200, D, dtype, 95)
    with torch.no_grad():
        cache.append(k, v, _i32(*LENS))
        cache.starts.copy_(_i32(*STARTS[0]))
        cache.prepare_attend()
        plain.prepare_attend()
        ws, att = cache._rows_ws, cache._att_ws
        assert ws.numel() == plain._rows_ws.numel() and att.numel() == plain._att_ws.numel() and cache._ws.numel() == plain._ws.numel()
        for Tq in (16, 80):
            q = _queries(4, Tq, D, dtype, 96 + Tq)
            ctx = cache.attend(q, D ** -0.5)                         # (code objects, the exponent window table)
            del ctx
            calls, held = mm.matmul_stats.cache_calls, torch.cuda.memory_allocated()
            for i in range(2):
                ctx, p = cache.attend(q, D ** -0.5, max_len=256, causal=bool(i), return_probs=True)
                del ctx, p
            assert torch.cuda.memory_allocated() == held and cache._rows_ws is ws and cache._att_ws is att
            assert mm.matmul_stats.cache_calls == calls + 4
