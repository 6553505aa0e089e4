"""GPU tests of the paged HBFP KV cache (bfp_ops.HBFPKVCache(page_tokens=P, pages=N), csrc/bfpq_kvcache.hip).  The yardstick
of every case is the cache that existed before -- device_lengths=True without pages -- given the same calls, and equality is
torch.equal on the raw bits: paging changes where the bytes lie, not what they are.

Shapes: P 64, capacity 256 (a table four entries wide), blocks 64 and 16, D 64 and 128, bf16 and fp32, 4 query heads over 4 and 2 kv
heads, batch 3 (4 where the four decode lengths 1, 64, 65 and 130 share a batch).  The pool is filled with 0x7f bytes before its first
use and the pages of a released sequence again before they are reused, so stale page contents would show; the table is scattered and
interleaved -- sequence b's i-th page is page 11 - b - 3 i (15 - b - 4 i at batch 4): consecutive tokens lie on pages that are neither
adjacent nor increasing."""
import pytest
import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops
import test_kvcache_pinned_gpu as pinned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, CAP, PT = 4, 256, 64
W = CAP // PT
# dtype, block, D, kv_heads: every value of each with both values of its neighbours somewhere
CASES = ((torch.bfloat16, 64, 64, 4), (torch.float32, 16, 128, 2), (torch.bfloat16, 16, 64, 2), (torch.float32, 64, 128, 4))
IDS = [f"{str(dt).split('.')[-1]}-b{blk}-d{D}-kv{kvh}" for dt, blk, D, kvh in CASES]
BUFFERS = ("k_codes", "k_exps", "v_codes", "v_exps")


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


def same(a, b):
    """the raw bits"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def scattered(b, B):
    """sequence b's pages, in token order"""
    return [W * B - 1 - b - B * i for i in range(W)]


def stale(c, pages=None):
    """0x7f in every byte of the pool, or of these pages"""
    for name in BUFFERS:
        if pages is None:
            getattr(c, name).fill_(0x7f)
        else:
            getattr(c, name)[torch.tensor(pages, device=DEV)] = 0x7f


def pair(dtype, block, D, kvh, B=3, give=None, **mode):
    """(the paged cache, its contiguous twin); give: pages per sequence (default: all four, scattered)"""
    kw = cfg(block_size=block)
    c = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=dtype, device_lengths=True, kv_heads=kvh, page_tokens=PT, pages=W * B + 2, **mode, **kw)
    twin = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=dtype, device_lengths=True, kv_heads=kvh, **mode, **kw)
    stale(c)
    for b in range(B):
        c.assign(b, scattered(b, B)[:W if give is None else give[b]])
    assert c.page_table.tolist() == c._table_host.tolist()
    return c, twin


def held_equal(c, twin, what):
    assert c.lengths.tolist() == twin.lengths.tolist(), what
    for b in range(c.batch):
        assert same(c.keys(b), twin.keys(b)), f"{what}: keys of sequence {b}"
        assert same(c.values(b), twin.values(b)), f"{what}: values of sequence {b}"


# (rows of the chunk, what each sequence takes of it): ragged counts; 70 tokens from position 60 -- three pages, and the open block handed
# over at 64 and at 128; single tokens taking sequence 1 over 63 -> 64 -> 65
APPENDS = ((63, (60, 63, 17)), (70, (70, 0, 33)), (1, (0, 1, 1)), (1, (1, 1, 0)))


def run_appends(c, twin, k, v, steps, what):
    s0 = 0
    for i, (t, counts) in enumerate(steps):
        for x in (c, twin):
            x.append(k[:, :, s0:s0 + t].contiguous(), v[:, :, s0:s0 + t].contiguous(), _i32(*counts))
        held_equal(c, twin, f"{what}: append {i}")
        s0 += t
    assert c.overflow.item() == 0 and twin.overflow.item() == 0, what


def decode_equal(c, twin, D, dtype, seed, what):
    B, scale = c.batch, D ** -0.5
    for Tq in (1, 16):
        q = _rand((B, H, Tq, D), dtype, seed + Tq)
        for max_len in (None, 192):
            ctx, p = c.attend(q, scale, max_len=max_len, causal=True, return_probs=True)
            want, pw = twin.attend(q, scale, max_len=max_len, causal=True, return_probs=True)
            assert same(ctx, want) and same(p, pw), f"{what}: attend Tq {Tq} max_len {max_len}"
            assert same(c.attend(q, scale, max_len=max_len, causal=True), want), f"{what}: attend without p, Tq {Tq} max_len {max_len}"
            assert same(c.scores(q, max_len), twin.scores(q, max_len)), f"{what}: scores Tq {Tq} max_len {max_len}"
            assert same(c.context(pw), twin.context(pw)), f"{what}: context Tq {Tq} L {pw.shape[-1]}"
    held_equal(c, twin, what + ": after the products")


# ---- 1. append -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block,D,kvh", CASES, ids=IDS)
def test_append_fills_scattered_pages_as_the_contiguous_cache(dtype, block, D, kvh):
    c, twin = pair(dtype, block, D, kvh)
    S = sum(t for t, _ in APPENDS)
    k, v = _rand((3, kvh, S, D), dtype, 100 + block), _rand((3, kvh, S, D), dtype, 101 + block)
    with torch.no_grad():
        run_appends(c, twin, k, v, APPENDS, "append")
    assert c.lengths.tolist() == [131, 65, 51]


# ---- 2. decode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block,D,kvh", CASES, ids=IDS)
def test_decode_products_equal_the_contiguous_cache(dtype, block, D, kvh):
    lens = (1, 64, 65, 130)
    c, twin = pair(dtype, block, D, kvh, B=4)
    k, v = _rand((4, kvh, max(lens), D), dtype, 200 + block), _rand((4, kvh, max(lens), D), dtype, 201 + block)
    with torch.no_grad():
        for x in (c, twin):
            x.append(k, v, _i32(*lens))
        decode_equal(c, twin, D, dtype, 210, "decode")


# ---- 3. the prompt route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block,D", [x[:3] for x in CASES], ids=[i.rsplit('-', 1)[0] for i in IDS])
def test_prompt_panels_equal_the_contiguous_cache(dtype, block, D):
    Tq, scale = 130, D ** -0.5
    k, v, q = (_rand((3, n, Tq, D), dtype, 300 + block + i) for i, n in enumerate((2, 2, H)))
    with torch.no_grad():
        c, twin = pair(dtype, block, D, 2, prompt_rows=64)
        for x in (c, twin):
            x.append(k, v)
        ctx, p = c.attend(q, scale, causal=True, return_probs=True)
        want, pw = twin.attend(q, scale, causal=True, return_probs=True)
        assert same(ctx, want) and same(p, pw), "the prompt whole"
        assert same(c.attend(q, scale, max_len=192), twin.attend(q, scale, max_len=192)), "the prompt whole, not causal, max_len 192"
        c, twin = pair(dtype, block, D, 2, prompt_rows=64)
        for s0 in range(0, Tq, 50):
            s1 = min(s0 + 50, Tq)
            for x in (c, twin):
                x.append(k[:, :, s0:s1].contiguous(), v[:, :, s0:s1].contiguous())
            got, p = c.attend(q[:, :, s0:s1].contiguous(), scale, causal=True, return_probs=True)
            want, pw = twin.attend(q[:, :, s0:s1].contiguous(), scale, causal=True, return_probs=True)
            assert same(got, want) and same(p, pw), f"the chunk from {s0}"
        held_equal(c, twin, "the prompt in chunks")


# ---- 4. a captured step follows the table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block,D,kvh", CASES[:2], ids=IDS[:2])
def test_captured_step_crosses_pages_and_follows_the_table(dtype, block, D, kvh):
    B, start, steps, scale = 3, (62, 5, 127), 4, D ** -0.5
    k, v = _rand((B, kvh, max(start) + steps + 2, D), dtype, 400 + block), _rand((B, kvh, max(start) + steps + 2, D), dtype, 401 + block)
    qs = [_rand((B, H, 1, D), dtype, 410 + i) for i in range(steps + 2)]
    c, twin = pair(dtype, block, D, kvh, give=(2, 1, 3))                                     # every page the replays reach, before the capture
    sk, sv = (torch.zeros(B, kvh, 1, D, dtype=dtype, device=DEV) for _ in range(2))
    ik, iv = (torch.zeros(B, kvh, 1, D, dtype=dtype, device=DEV) for _ in range(2))
    sq, iq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(2))

    def step():
        sk.copy_(ik); sv.copy_(iv); sq.copy_(iq)
        c.append(sk, sv)
        return c.attend(sq, scale, causal=True)

    def fill(x):
        x.append(k[:, :, :max(start)].contiguous(), v[:, :, :max(start)].contiguous(), _i32(*start))

    def replay_equal(i, what):
        n = max(start) + i
        ik.copy_(k[:, :, n:n + 1]); iv.copy_(v[:, :, n:n + 1]); iq.copy_(qs[i])
        graph.replay()
        twin.append(ik, iv)
        assert same(ctx, twin.attend(iq, scale, causal=True)), what
        held_equal(c, twin, what)

    with torch.no_grad():
        step()                                                       # warm-up: code objects, the exponent window table, attend's workspace
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx = step()
        for b in range(B):                                           # undo the warm-up and capture-time appends; the same pages again
            c.release(b)
        c.overflow.zero_()
        stale(c)
        for b, n in enumerate((2, 1, 3)):
            c.assign(b, scattered(b, B)[:n])
        fill(c)
        fill(twin)
        for i in range(steps):                                       # sequence 0: 62 -> 66, into its second page; sequence 2: 127 -> 131
            replay_equal(i, f"replay {i}")
        assert c.lengths.tolist() == [s + steps for s in start] and c.overflow.item() == 0
        # sequence 0 moves to other pages between two replays, and holds a fresh prompt there
        old = list(c._owned[0])
        c.release(0)
        stale(c, old)
        c.assign(0, [c.page_count - 1, c.page_count - 2])
        assert not set(c._owned[0]) & set(old)
        twin.lengths[0:1].zero_()
        for x in (c, twin):
            x.append(v[:, :, :70].contiguous(), k[:, :, :70].contiguous(), _i32(70, 0, 0))
        held_equal(c, twin, "the fresh prompt")
        for i in range(steps, steps + 2):
            replay_equal(i, f"replay {i}, after the table changed")
    assert c.lengths.tolist() == [72, 5 + steps + 2, 127 + steps + 2] and c.overflow.item() == 0 and twin.overflow.item() == 0


# ---- 5. refusal ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block,D,kvh", CASES[:2], ids=IDS[:2])
def test_a_sequence_without_a_page_for_its_chunk_is_refused(dtype, block, D, kvh):
    c, twin = pair(dtype, block, D, kvh, give=(1, 2, 2))
    k, v = _rand((3, kvh, 90, D), dtype, 500 + block), _rand((3, kvh, 90, D), dtype, 501 + block)

    def owned(b):
        return [getattr(c, name)[torch.tensor(c._owned[b], device=DEV)].clone() for name in BUFFERS] + [c.v_tail[b].clone()]

    with torch.no_grad():
        for x in (c, twin):
            x.append(k[:, :, :60].contiguous(), v[:, :, :60].contiguous(), _i32(60, 60, 3))
        assert c.page_table[0].tolist() == [scattered(0, 3)[0], -1, -1, -1]
        for t, twin_counts, lens in ((10, (0, 10, 10), [60, 70, 13]),       # tokens 60 .. 69 of sequence 0: the last six have no page
                                     (4, (4, 4, 4), [64, 74, 17]),           # up to the end of its page: taken
                                     (1, (0, 1, 1), [64, 75, 18])):          # token 64: no page
            refused = twin_counts[0] == 0
            before, k0, v0 = owned(0), c.keys(0), c.values(0)
            c.overflow.zero_()
            c.append(k[:, :, 60:60 + t].contiguous(), v[:, :, 60:60 + t].contiguous())
            twin.append(k[:, :, 60:60 + t].contiguous(), v[:, :, 60:60 + t].contiguous(), _i32(*twin_counts))
            assert c.lengths.tolist() == lens and c.overflow.item() == int(refused), f"a chunk of {t}"
            held_equal(c, twin, f"a chunk of {t}")
            if refused:
                assert same(c.keys(0), k0) and same(c.values(0), v0), f"a chunk of {t}: sequence 0 was touched"
                assert all(same(a, b) for a, b in zip(before, owned(0))), f"a chunk of {t}: the bytes of sequence 0's page or tail changed"
        q = _rand((3, H, 1, D), dtype, 510)
        assert same(c.attend(q, D ** -0.5), twin.attend(q, D ** -0.5))
    assert twin.overflow.item() == 0


# ---- 6. reuse --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block,D,kvh", CASES, ids=IDS)
def test_released_pages_serve_a_new_sequence(dtype, block, D, kvh):
    S = sum(t for t, _ in APPENDS)
    k, v = _rand((3, kvh, S, D), dtype, 600 + block), _rand((3, kvh, S, D), dtype, 601 + block)
    k2, v2 = _rand((3, kvh, S, D), dtype, 602 + block), _rand((3, kvh, S, D), dtype, 603 + block)
    only1 = tuple((t, (0, n[0], 0)) for t, n in APPENDS)             # sequence 1 takes what sequence 0 took: 60 + 70, then a token
    with torch.no_grad():
        c, twin = pair(dtype, block, D, kvh)
        run_appends(c, twin, k, v, APPENDS, "first use")
        old = list(c._owned[1])
        c.release(1)
        assert c.pages_free == 2 + W and c.lengths.tolist() == [131, 0, 51]
        stale(c, old)
        c.assign(1, old[::-1])                                        # the same pages, the other way round
        fresh = bfp_ops.HBFPKVCache(3, H, D, CAP, dtype=dtype, device_lengths=True, kv_heads=kvh, **cfg(block_size=block))
        s0 = 0
        for t, counts in APPENDS:                                     # the fresh twin: sequences 0 and 2 as before, sequence 1 empty
            fresh.append(k[:, :, s0:s0 + t].contiguous(), v[:, :, s0:s0 + t].contiguous(), _i32(counts[0], 0, counts[2]))
            s0 += t
        run_appends(c, fresh, k2, v2, only1, "reuse")
        assert c.lengths.tolist() == [131, 131, 51]
        decode_equal(c, fresh, D, dtype, 610, "reuse")


# ---- 7. the cache without pages is the cache it was ---------------------------------------------------------------------------------------
def test_the_cache_without_pages_keeps_its_recorded_bits():
    import json
    case, kvh = pinned.CASES[1], 2                                    # bf16, block 32, D 64, mant_bits 3
    want = json.load(open(pinned.FIXTURE))[pinned._key(*case, kvh)]
    got = pinned.digests(*case, kvh)
    assert list(got) == list(want) and not [step for step in got if got[step] != want[step]]
