"""GPU tests of the device-length HBFP KV cache (bfp_ops.HBFPKVCache(device_lengths=True), csrc/bfpq_kvcache.hip).  The
yardstick is the host-length HBFPKVCache, one batch = 1 cache per sequence fed the same tokens (tests/test_kvcache_gpu.py pins its
contents to the oracle and its products to k_bmm_i8); every comparison is bit for bit.  One case goes to the oracle's quantization of the
concatenation directly."""
import pytest
import torch
import torch.nn.functional as F

from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import bits, assert_bits_equal
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ('fp32', 'bf16', 'fp16')
NAMES = ('k_codes', 'k_exps', 'v_codes', 'v_exps')


def cfg(**kw):
    base = dict(mant_bits=7, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=64, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')
    base.update(kw)
    return base


def _uz(t):
    return torch.where(t == 0, torch.zeros_like(t), t)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _tokens(B, H, S, D, dtype, seed):
    """magnitudes over many binades along the tokens, so that the open block's exponent keeps changing"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.randn(B, H, S, D, generator=g) * torch.exp2(torch.randint(-6, 4, (B, H, S, 1), generator=g).float())).to(dtype).to(DEV)
    return mk(), mk()


class Pair:
    """a device-length cache and its yardstick: one host-length batch = 1 cache per sequence"""

    def __init__(self, B, H, D, capacity, dtype, kw, **mode):
        self.dev = bfp_ops.HBFPKVCache(B, H, D, capacity, dtype=dtype, device_lengths=True, **mode, **kw)
        self.hosts = [bfp_ops.HBFPKVCache(1, H, D, capacity, dtype=dtype, **kw) for _ in range(B)]
        self.B = B

    def append(self, k, v, counts=None):
        t = k.shape[2]
        with torch.no_grad():
            assert self.dev.append(k, v, None if counts is None else _i32(*counts)) is None
            for b, h in enumerate(self.hosts):
                n = t if counts is None else counts[b]
                if n:
                    h.append(k[b:b + 1, :, :n].contiguous(), v[b:b + 1, :, :n].contiguous())

    def lengths(self):
        return [h.length for h in self.hosts]

    def check(self, what, fresh=True):
        """lengths, the four code arrays whole (untouched regions are zero on both sides), the live rows of v_tail, zeros behind.
        fresh=False, after a reset(), which leaves all but v_codes stale: the tokens held, and v_codes whole"""
        d = self.dev
        assert d.lengths.tolist() == self.lengths(), what
        for b, h in enumerate(self.hosts):
            S, blk = h.length, d.block
            live, nb = S % blk, (S + blk - 1) // blk
            for name in NAMES:
                held = (lambda t: t) if fresh or name == 'v_codes' else (lambda t: t[:, :S] if name[0] == 'k' else t[:, :, :nb])
                assert torch.equal(held(getattr(d, name)[b]), held(getattr(h, name)[0])), f"{what}: {name} of sequence {b}"
            assert_bits_equal(bits(d.v_tail[b, :, :live]), bits(h.v_tail[0, :, :live]), d.dtype, f"{what}: v_tail of sequence {b}")
            if not fresh:
                continue
            assert not bool(d.k_codes[b, :, S:].any()) and not bool(d.k_exps[b, :, S:].any()) and not bool(d.v_codes[b, :, :, S:].any())
            assert not bool(d.v_exps[b, :, :, (S + blk - 1) // blk:].any()), f"{what}: sequence {b} behind S = {S}"
            if S == 0:
                assert not bool(d.v_tail[b].any()), f"{what}: the empty sequence {b} has a tail"


def _check_oracle(cache, b, k_all, v_all, kw, what):
    """keys(b) / values(b) against the oracle on everything sequence b was given (tests/test_kvcache_gpu.py: _check_contents)"""
    dt = cache.dtype
    want_k = O.float_to_bfp_blocked(k_all.cpu(), **kw, identifier='w')
    want_v = O.float_to_bfp_blocked(v_all.cpu().transpose(-1, -2).contiguous(), **kw, identifier='w').transpose(-1, -2)
    with torch.no_grad():
        got_k, got_v = cache.keys(b).cpu(), cache.values(b).cpu()
    assert got_k.shape == k_all.shape and got_v.shape == v_all.shape, what
    assert_bits_equal(bits(_uz(got_k)), bits(_uz(want_k)), dt, f"{what}: keys of sequence {b}")
    assert_bits_equal(bits(_uz(got_v)), bits(_uz(want_v.contiguous())), dt, f"{what}: values of sequence {b}")


# ---- 1. ragged contents ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (3, 7))
@pytest.mark.parametrize("D,block", ((64, 64), (64, 32), (32, 16)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ragged_contents(dtype, D, block, m):
    B, H = 3, 2
    kw = cfg(mant_bits=m, block_size=block)
    what = f"{dtype} D {D} block {block} m {m}"
    k, v = _tokens(B, H, 165, D, dtype, 1000 * block + 10 * m)
    pair = Pair(B, H, D, 256, dtype, kw)
    given = [[] for _ in range(B)]                                # per sequence, the slices of k / v it has taken

    def step(lo, t, counts=None):
        pair.append(k[:, :, lo:lo + t], v[:, :, lo:lo + t], counts)
        for b in range(B):
            n = t if counts is None else counts[b]
            given[b].append((lo, lo + n))

    step(0, 130, (0, 37, 130))
    assert pair.lengths() == [0, 37, 130]
    pair.check(what + " after the prefill")
    for i in range(30):                                           # the sequences cross their block boundaries at different steps
        step(130 + i, 1)
    assert pair.lengths() == [30, 67, 160]
    pair.check(what + " after 30 single tokens")
    step(160, 5, (5, 0, 2))
    assert pair.lengths() == [35, 67, 162]
    pair.check(what + " at the end")
    assert pair.dev.overflow.item() == 0
    for b in range(B):
        cat = lambda x: torch.cat([x[b:b + 1, :, lo:hi] for lo, hi in given[b]], dim=2)
        _check_oracle(pair.dev, b, cat(k), cat(v), kw, what)


# ---- 2. the open block ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
def test_open_block_is_rounded_from_the_original_values(dtype):
    """the construction of tests/test_kvcache_gpu.py on sequence 0 of a ragged batch -- token 100 of one head 2^5 times larger than tokens
    64..99, after 36 of them were coded -- while sequence 1 sits at a block boundary (64 tokens) and takes nothing more"""
    block, m, D = 64, 3, 64
    kw = cfg(mant_bits=m, block_size=block)
    g = torch.Generator().manual_seed(5)
    k = torch.randn(2, 2, 192, D, generator=g).to(dtype)
    v = torch.randn(2, 2, 192, D, generator=g).to(dtype)
    v[0, 1, 100] *= 32.0
    v[0, 0, 101, 7] = float('nan')
    v[0, 1, 102, 9] = float('inf')
    v[0, :, 128:] = 0
    q = lambda t: O.float_to_bfp_blocked(t.transpose(-1, -2).contiguous(), **kw, identifier='w').transpose(-1, -2)
    once = q(v[0, 1, 64:101])
    twice = q(torch.cat([q(v[0, 1, 64:100]), v[0, 1, 100:101]]))
    assert not torch.equal(once, twice), "the chosen values do not tell a double rounding apart"
    k, v = k.to(DEV), v.to(DEV)
    pair = Pair(2, 2, D, 192, dtype, kw)
    pos = 0
    for t in (64, 36, 1, 1, 1, 25, 10, 54):
        pair.append(k[:, :, pos:pos + t], v[:, :, pos:pos + t], (t, 64 if pos == 0 else 0))
        pos += t
        assert pair.lengths() == [pos, 64]
        pair.check(f"open block {dtype} at {pos}")
        _check_oracle(pair.dev, 0, k[:1, :, :pos], v[:1, :, :pos], kw, f"open block {dtype} at {pos}")
    assert pos == 192
    _check_oracle(pair.dev, 1, k[1:, :, :64], v[1:, :, :64], kw, "the sequence at the block boundary")


# ---- 3. scores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (16, 32, 64))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
def test_scores(dtype, block):
    lens, H, D = (1, 64, 65, 200), 2, 64
    kw = cfg(mant_bits=5, block_size=block)
    k, v = _tokens(4, H, 200, D, dtype, 31 + block)
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **dict(kw))
    pair = Pair(4, H, D, 256, dtype, kw, stats=mm.matmul_stats)
    pair.append(k, v, lens)
    g = torch.Generator().manual_seed(3)
    calls = 0
    for Tq in (1, 5, 16):
        q = torch.randn(4, H, Tq, D, generator=g).to(dtype).to(DEV)
        with torch.no_grad():
            want = [h.scores(q[b:b + 1]) for b, h in enumerate(pair.hosts)]
            for max_len in (200, 256):
                got = pair.dev.scores(q, max_len=max_len)
                calls += 1
                assert got.shape == (4, H, Tq, max_len) and got.dtype == dtype
                for b, S in enumerate(lens):
                    assert_bits_equal(bits(got[b, :, :, :S]), bits(want[b][0]), dtype, f"scores {dtype} block {block} Tq {Tq} sequence {b}")
                    assert bool((got[b, :, :, S:] == float('-inf')).all()), f"columns past {S} of sequence {b} at max_len {max_len}"
            assert torch.equal(pair.dev.scores(q), got)                               # max_len defaults to the capacity
            calls += 1
    assert mm.matmul_stats.cache_calls == calls                                      # the op's statistics count the new calls too
    pair.check("scores change nothing")


# ---- 4. context and the split ---------------------------------------------------------------------------------------------------------
CTX_LENS = (1, 64, 127, 128, 129, 300, 512)


@pytest.mark.parametrize("cps", (1, 2, 0))
@pytest.mark.parametrize("block", (16, 32, 64))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
def test_context_and_the_split(dtype, block, cps):
    B, H, D, cap = len(CTX_LENS), 1, 64, 512
    kw = cfg(mant_bits=5, block_size=block)
    k, v = _tokens(B, H, cap, D, dtype, 47 + block)
    pair = Pair(B, H, D, cap, dtype, kw, chunks_per_split=cps)
    pair.append(k, v, CTX_LENS)
    g = torch.Generator().manual_seed(4)
    for Tq in (1, 16):
        p = (torch.rand(B, H, Tq, cap, generator=g) * torch.exp2(torch.randint(-8, 0, (B, H, Tq, cap // 16), generator=g).float())
             .repeat_interleave(16, -1)).to(dtype).to(DEV)
        what = f"context {dtype} block {block} chunks_per_split {cps} Tq {Tq}"
        with torch.no_grad():
            want = torch.cat([h.context(p[b:b + 1, :, :, :S].contiguous()) for (b, h), S in zip(enumerate(pair.hosts), CTX_LENS)])
            got = pair.dev.context(p)
            assert got.shape == (B, H, Tq, D) and got.dtype == dtype
            assert_bits_equal(bits(got), bits(want), dtype, what)
            # whatever p holds at and past a sequence's length counts as zero
            junk = p.clone()
            for b, S in enumerate(CTX_LENS):
                junk[b, :, :, S:] = float('nan')
                junk[b, :, :, S + 1:] = float('inf')
            assert_bits_equal(bits(pair.dev.context(junk)), bits(want), dtype, what + " with NaN and Inf past the lengths")
            # L = 300 (rows that are not 16-byte aligned in bf16): min(length, 300) tokens.  For the sequence of 512 the yardstick takes
            # p zero-padded: zero codes against the cached ones, blocks that add 0
            want300 = torch.cat([h.context(F.pad(p[b:b + 1, :, :, :min(S, 300)], (0, S - min(S, 300)))) for (b, h), S in zip(enumerate(pair.hosts), CTX_LENS)])
            assert_bits_equal(bits(pair.dev.context(p[..., :300].contiguous())), bits(want300), dtype, what + " at L = 300")
    pair.check("context changes nothing")
    with torch.no_grad():
        pair.dev.reset()
        assert pair.dev.lengths.tolist() == [0] * B
        zero = pair.dev.context(p)
    assert zero.shape == (B, H, 16, D) and not bool(zero.any()) and not bool(torch.signbit(zero).any()), "sequences of length 0 give zeros"


@pytest.mark.parametrize("Tq", (5, 16))
@pytest.mark.parametrize("block", (16, 64))
def test_nan_blocks_on_either_side(block, Tq):
    """a NaN in x inside the live range makes its block's scale NaN (the whole row); a -128 exponent in the cache makes that key's /
    column's block NaN -- in another slice of the tokens than the one that is finite"""
    B, H, D, dtype, lens = 2, 2, 64, torch.float32, (100, 200)
    kw = cfg(mant_bits=5, block_size=block)
    k, v = _tokens(B, H, 200, D, dtype, 77)
    pair = Pair(B, H, D, 256, dtype, kw, chunks_per_split=1)
    pair.append(k, v, lens)
    g = torch.Generator().manual_seed(6)
    q = torch.randn(B, H, Tq, D, generator=g).to(DEV)
    p = torch.rand(B, H, Tq, 256, generator=g).to(DEV)
    q[0, 1, 3, 40] = float('nan')
    p[0, 0, 2, 99] = float('nan')                                     # in the ragged last block of sequence 0
    p[1, 1, 4, 130] = float('nan')                                    # in the third chunk of sequence 1
    for b, (h, n) in enumerate(((0, 77), (1, 150))):                  # key n of head h; column 9 + 2 b of the other head, the block of token n
        pair.dev.k_exps[b, h, n, 0] = pair.hosts[b].k_exps[0, h, n, 0] = -128
        pair.dev.v_exps[b, 1 - h, 9 + 2 * b, n // block] = pair.hosts[b].v_exps[0, 1 - h, 9 + 2 * b, n // block] = -128
    with torch.no_grad():
        got_s, got_c = pair.dev.scores(q), pair.dev.context(p)
        for b, (h, S) in enumerate(zip(pair.hosts, lens)):
            assert_bits_equal(bits(got_s[b, :, :, :S]), bits(h.scores(q[b:b + 1])[0]), dtype, f"scores with NaN blocks, sequence {b}")
            assert_bits_equal(bits(got_c[b]), bits(h.context(p[b:b + 1, :, :, :S].contiguous())[0]), dtype, f"context with NaN blocks, sequence {b}")
    nan = torch.isnan
    assert bool(nan(got_s[0, 1, 3, :100]).all()) and bool(nan(got_s[0, 0, :, 77]).all()) and bool(nan(got_s[1, 1, :, 150]).all())
    assert bool(nan(got_c[0, 0, 2]).all()) and bool(nan(got_c[0, 1, :, 9]).all()) and bool(nan(got_c[1, 1, 4]).all())
    assert bool(nan(got_c[1, 0, :, 11]).all())


# ---- 5. overflow ----------------------------------------------------------------------------------------------------------------------
def test_overflow_leaves_the_sequence_untouched():
    B, H, D, dtype = 2, 2, 64, torch.bfloat16
    kw = cfg()
    k, v = _tokens(B, H, 80, D, dtype, 8)
    pair = Pair(B, H, D, 64, dtype, kw)
    pair.append(k[:, :, :60], v[:, :, :60], (60, 10))
    snap = lambda: {name: t[0].clone() for name, t in pair.dev.buffers.items()}
    before = snap()
    with torch.no_grad():
        pair.dev.append(k[:, :, 60:68], v[:, :, 60:68])                              # 60 + 8 > 64: sequence 0 is refused whole
        pair.hosts[1].append(k[1:, :, 60:68], v[1:, :, 60:68])
    assert pair.dev.lengths.tolist() == [60, 18] and pair.dev.overflow.item() == 1
    for name, t in snap().items():
        assert torch.equal(t, before[name]), f"{name} of the refused sequence"
    pair.check("after the refused append")
    pair.append(k[:, :, 68:70], v[:, :, 68:70], (2, 1))                              # it still takes what fits; the flag stays
    assert pair.dev.lengths.tolist() == [62, 19] and pair.dev.overflow.item() == 1
    pair.check("after the next append")
    with torch.no_grad():
        pair.dev.reset()
        assert pair.dev.overflow.item() == 0 and pair.dev.lengths.tolist() == [0, 0]
        after_reset = snap()
        for h in pair.hosts:
            h.reset()
        for bad in (9, -1):                                                           # a count outside 0..t: the same
            pair.dev.append(k[:, :, :8], v[:, :, :8], _i32(bad, 3))
            assert pair.dev.overflow.item() == 1
            pair.dev.overflow.zero_()
        pair.hosts[1].append(k[1:, :, :3], v[1:, :, :3])
        pair.hosts[1].append(k[1:, :, :3], v[1:, :, :3])
    assert pair.dev.lengths.tolist() == [0, 6]
    for name, t in snap().items():                                                    # (reset() zeroes v_codes alone: the rest is stale)
        assert torch.equal(t, after_reset[name]), f"{name} of the sequence with a bad count"
    for name in NAMES:                                                                # (the yardstick has been through the same appends)
        assert torch.equal(getattr(pair.dev, name)[1], getattr(pair.hosts[1], name)[0]), name


# ---- 6. a captured decode step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (16, 64))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
def test_captured_decode_advances_on_every_replay(dtype, block):
    B, H, D, cap, steps = 2, 2, 64, 256, 70
    kw = cfg(block_size=block)
    scale = 1.0 / 8.0
    k, v = _tokens(B, H, 62 + steps, D, dtype, 9 + block)
    g = torch.Generator().manual_seed(10)
    qs = torch.randn(steps, B, H, 1, D, generator=g).to(dtype).to(DEV)
    pair = Pair(B, H, D, cap, dtype, kw)
    cache = pair.dev
    sk, sv, sq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(3))
    ik, iv, iq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(3))

    def step():
        sk.copy_(ik); sv.copy_(iv); sq.copy_(iq)
        cache.append(sk, sv)
        scores = cache.scores(sq, max_len=cap)
        p = torch.softmax(scores.float() * scale, dim=-1).to(dtype)
        return scores, p, cache.context(p)

    with torch.no_grad():
        cache.append(k[:, :, :62], v[:, :, :62], _i32(5, 62))
        step()                                                           # warm-up: code objects and the exponent window table
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            scores, p, ctx = step()
        cache.reset()                                                    # undo the warm-up and capture-time appends
        pair.append(k[:, :, :62], v[:, :, :62], (5, 62))
        pair.check("before the first replay", fresh=False)
        for i in range(steps):
            ik.copy_(k[:, :, 62 + i:63 + i]); iv.copy_(v[:, :, 62 + i:63 + i]); iq.copy_(qs[i])
            graph.replay()
            lens = [5 + i + 1, 62 + i + 1]
            assert cache.lengths.tolist() == lens, f"replay {i}"
            ws = []
            for b, h in enumerate(pair.hosts):
                h.append(ik[b:b + 1], iv[b:b + 1])
                ws.append(F.pad(h.scores(iq[b:b + 1]), (0, cap - lens[b]), value=float('-inf')))
            want_s = torch.cat(ws)
            want_p = torch.softmax(want_s.float() * scale, dim=-1).to(dtype)         # the same call on the same shape as in the graph
            what = f"{dtype} block {block} replay {i}"
            assert_bits_equal(bits(scores), bits(want_s), dtype, "scores " + what)
            assert_bits_equal(bits(p), bits(want_p), dtype, "softmax " + what)
            for b, h in enumerate(pair.hosts):
                assert_bits_equal(bits(ctx[b]), bits(h.context(want_p[b:b + 1, :, :, :lens[b]].contiguous())[0]), dtype, f"context {what} sequence {b}")
    assert cache.overflow.item() == 0
    pair.check("after the last replay", fresh=False)
