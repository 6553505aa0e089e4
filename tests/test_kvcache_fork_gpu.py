"""GPU tests of page sharing on the paged HBFP KV cache (HBFPKVCache.fork / reorder, csrc/bfpq_kvpages.hip).  The yardstick of
every case is a *contiguous* HBFPKVCache with the same arguments, fed the concatenated history of what each row logically holds, and
equality is torch.equal on the raw bits: sharing pages changes who names the bytes, not what a sequence is.

Shapes: 4 sequences, 4 query heads over 2 kv heads, D 64, capacity 256, bf16 at block 64 and fp32 at block 16, pages of 64 and 128
tokens.  The pool (16 pages unless a test says otherwise) is filled with 0x7f bytes before its first use, so a page that was not
copied would show, and the sequences' pages are scattered and decreasing: sequence b's i-th page is page 15 - b - 4 i."""
import pytest
import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, KVH, D, CAP = 4, 4, 2, 64, 256
SCALE = D ** -0.5
FORMATS = ((torch.bfloat16, 64), (torch.float32, 16))
FIDS = ["bf16-b64", "f32-b16"]
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


def scattered(b, n):
    return [15 - b - 4 * i for i in range(n)]


def make(dtype, block, PT, pages=16, **mode):
    c = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=dtype, device_lengths=True, kv_heads=KVH, page_tokens=PT, pages=pages, **mode,
                            **cfg(block_size=block))
    for name in BUFFERS:
        getattr(c, name).fill_(0x7f)
    return c


class Rows:
    """a paged cache and, per row, the keys and values it logically holds ([KVH, tokens, D] each): what the contiguous twin is fed"""

    def __init__(self, c, dtype, block, **mode):
        self.c, self.dtype, self.block, self.mode = c, dtype, block, mode
        self.hist = [(torch.zeros(KVH, 0, D, dtype=dtype, device=DEV),) * 2 for _ in range(B)]

    def lens(self):
        return [h[0].shape[1] for h in self.hist]

    def chunk(self, new):
        """new {row: (k, v) [KVH, t, D]} as the arguments of append: [B, KVH, t, D] twice and the counts"""
        t = max(k.shape[1] for k, _ in new.values())
        ks, vs = (torch.zeros(B, KVH, t, D, dtype=self.dtype, device=DEV) for _ in range(2))
        for b, (k, v) in new.items():
            ks[b, :, :k.shape[1]], vs[b, :, :k.shape[1]] = k, v
        return ks, vs, _i32(*[new[b][0].shape[1] if b in new else 0 for b in range(B)])

    def append(self, new):
        ks, vs, counts = self.chunk(new)
        self.c.append(ks, vs, counts)
        for b, (k, v) in new.items():
            self.hist[b] = (torch.cat([self.hist[b][0], k], 1), torch.cat([self.hist[b][1], v], 1))

    def reordered(self, index):
        self.hist = [self.hist[s] for s in index]

    def twin(self):
        """the contiguous cache of the rows' histories"""
        t = bfp_ops.HBFPKVCache(B, H, D, CAP, dtype=self.dtype, device_lengths=True, kv_heads=KVH, **self.mode, **cfg(block_size=self.block))
        if max(self.lens()):
            ks, vs, counts = self.chunk({b: h for b, h in enumerate(self.hist)})
            t.append(ks, vs, counts)
        return t

    def check(self, what, seed=7):
        c, t = self.c, self.twin()
        assert c.lengths.tolist() == self.lens() == t.lengths.tolist(), what
        assert c.overflow.item() == 0 and t.overflow.item() == 0, what
        for b in range(B):
            assert same(c.keys(b), t.keys(b)), f"{what}: keys of row {b}"
            assert same(c.values(b), t.values(b)), f"{what}: values of row {b}"
        for Tq in (1, 3):
            q = _rand((B, H, Tq, D), self.dtype, seed + Tq)
            ctx, p = c.attend(q, SCALE, causal=True, return_probs=True)
            want, pw = t.attend(q, SCALE, causal=True, return_probs=True)
            assert same(ctx, want) and same(p, pw), f"{what}: attend with probs, Tq {Tq}"
            assert same(c.attend(q, SCALE), t.attend(q, SCALE)), f"{what}: attend, Tq {Tq}"
        return t


def new_tokens(rows, t, dtype, seed):
    return {b: (_rand((KVH, t, D), dtype, seed + 2 * b), _rand((KVH, t, D), dtype, seed + 2 * b + 1)) for b in rows}


def fill(r, lens, pt, seed):
    """rows of `lens` tokens on scattered pages, exactly the pages those tokens need"""
    for b, n in enumerate(lens):
        if n:
            r.c.assign(b, scattered(b, (n + pt - 1) // pt))
    new = new_tokens([b for b, n in enumerate(lens) if n], max(lens), r.dtype, seed)
    r.append({b: (k[:, :lens[b]], v[:, :lens[b]]) for b, (k, v) in new.items()})


def pool_bytes(c):
    return [getattr(c, name).clone() for name in BUFFERS]


# ---- 1. fork: the destination is the source, then each goes its own way -------------------------------------------------------------------
@pytest.mark.parametrize("PT,L", [(64, 70), (64, 64), (64, 130), (64, 128), (128, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype,block", FORMATS, ids=FIDS)
def test_fork_then_diverge(dtype, block, PT, L):
    lens = [L, 33, 0, 70]
    with torch.no_grad():
        r, alone = (Rows(make(dtype, block, PT), dtype, block) for _ in range(2))     # alone: the same cache, never forked
        for x in (r, alone):
            fill(x, lens, PT, 100)
        free = r.c.pages_free
        r.c.fork(0, 2, tokens=L if L != 130 else None)               # (None: the length is read back)
        r.reordered([0, 1, 0, 3])
        assert r.c.pages_free == free - (L % PT != 0) and r.c.pages_shared == L // PT
        assert r.c.page_table.tolist() == r.c._table_host.tolist()
        assert same(r.c.keys(2), r.c.keys(0)) and same(r.c.values(2), r.c.values(0)), "right after the fork"
        q = _rand((B, H, 2, D), dtype, 5)
        q[2] = q[0]
        ctx = r.c.attend(q, SCALE, causal=True)
        assert same(ctx[2], ctx[0]), "right after the fork: attend"
        r.check("right after the fork")
        want = [L + 21, 33, L + 21, 70]
        r.c.reserve(want)
        alone.c.reserve([L + 21, 33, 0, 70])
        for i, t in enumerate((1, 20)):                               # one token, then a chunk that crosses a block (of 16)
            new = new_tokens((0, 2), t, dtype, 200 + 10 * i)
            r.append(new)
            alone.append({0: new[0]})
            r.check(f"after {t} more tokens")
            # copy on write: the source is what it is without the fork, byte for byte
            own, its = (torch.tensor(x.c._owned[0], device=DEV) for x in (r, alone))
            for name in BUFFERS:
                assert torch.equal(getattr(r.c, name)[own], getattr(alone.c, name)[its]), f"{name} of the source after {t} more tokens"
            assert same(r.c.v_tail[0], alone.c.v_tail[0]) and same(r.c.keys(0), alone.c.keys(0)) and same(r.c.values(0), alone.c.values(0))
        assert r.c.lengths.tolist() == want and r.c.overflow.item() == 0


# ---- 2. reorder: a cycle, a duplicate and an untouched row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block", FORMATS, ids=FIDS)
def test_reorder_with_a_cycle_a_duplicate_and_an_untouched_row(dtype, block):
    lens, index = [70, 129, 5, 64], [1, 0, 0, 3]
    with torch.no_grad():
        r = Rows(make(dtype, block, 64), dtype, block)
        fill(r, lens, 64, 300)
        r.check("before")
        before, row3, plan = pool_bytes(r.c), list(r.c._owned[3]), r.c._plan_reorder(index, lens)
        written = [j[3] for j in plan[3] if j[3] >= 0]
        assert len(plan[3]) == 3 and len(written) == 1 and all(j[1] != 3 for j in plan[3])
        r.c.reorder(torch.tensor(index, device=DEV))                 # an index on the device, the lengths read back with it
        r.reordered(index)
        assert r.c._owned[3] == row3 and r.c.page_table[3].tolist()[:1] == row3 and r.c.pages_shared == 1
        keep = torch.tensor([p for p in range(16) if p not in written], device=DEV)
        for was, now in zip(before, pool_bytes(r.c)):                  # nothing of the pool moved but the page the job names
            assert torch.equal(was[keep], now[keep])
        r.check("after the reorder")
        r.c.reserve([n + 21 for n in r.lens()])
        for i, t in enumerate((1, 20)):
            r.append(new_tokens(range(B), t, dtype, 400 + 10 * i))
            r.check(f"after the reorder and {t} more tokens")


# ---- 3. lifetime: a fork outlives its source ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block", FORMATS, ids=FIDS)
def test_shared_pages_outlive_the_source(dtype, block):
    with torch.no_grad():
        r = Rows(make(dtype, block, 64, pages=8), dtype, block)
        r.c.assign(0, [7, 3, 5])
        r.append(new_tokens([0], 130, dtype, 500))
        r.c.fork(0, 2, 130)
        r.reordered([0, 1, 0, 3])
        r.c.release(0)
        r.hist[0] = r.hist[1]                                         # (empty)
        assert r.c.pages_free == 5 and r.c.pages_shared == 0 and r.c.page_refs[7] == 1 and r.c.page_refs[5] == 0
        free = list(r.c._free)
        for name in BUFFERS:
            getattr(r.c, name)[torch.tensor(free, device=DEV)] = 0x7f
        r.c.reserve([0, 256, 0, 64])                                  # every free page, the source's open page among them
        assert r.c.pages_free == 0
        other = new_tokens([1, 3], 256, dtype, 510)
        other[3] = (other[3][0][:, :64], other[3][1][:, :64])
        r.append(other)
        r.check("the fork after its source was released and every free page rewritten")
        for b in (1, 3):
            r.c.release(b)
        assert r.c.pages_free == 5
        r.c.release(2)
        assert r.c.pages_free == 8 and r.c.page_refs == [0] * 8


# ---- 4. the prompt route ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block", FORMATS, ids=FIDS)
def test_prompt_panels_read_shared_pages(dtype, block):
    with torch.no_grad():
        r = Rows(make(dtype, block, 64, prompt_rows=64), dtype, block, prompt_rows=64)
        fill(r, [70, 0, 0, 0], 64, 600)
        r.c.fork(0, [1, 2, 3], 70)
        r.reordered([0, 0, 0, 0])
        assert r.c.pages_shared == 1 and r.c.page_refs[15] == 4
        r.c.reserve(90)
        r.append(new_tokens(range(B), 20, dtype, 610))
        t = r.twin()
        q = _rand((B, H, 20, D), dtype, 620)
        ctx, p = r.c.attend(q, SCALE, causal=True, return_probs=True)
        want, pw = t.attend(q, SCALE, causal=True, return_probs=True)
        assert same(ctx, want) and same(p, pw)
        assert r.c.lengths.tolist() == [90] * 4 and r.c.overflow.item() == 0


# ---- 5. a captured step follows a fork made between two replays ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block", FORMATS[:1], ids=FIDS[:1])
def test_captured_step_follows_a_fork(dtype, block):
    lens = [70, 33, 5, 64]
    sk, sv, ik, iv = (torch.zeros(B, KVH, 1, D, dtype=dtype, device=DEV) for _ in range(4))
    sq, iq = (torch.zeros(B, H, 1, D, dtype=dtype, device=DEV) for _ in range(2))
    r = Rows(make(dtype, block, 64), dtype, block)

    def step():
        sk.copy_(ik); sv.copy_(iv); sq.copy_(iq)
        r.c.append(sk, sv)
        return r.c.attend(sq, SCALE, causal=True)

    def replay_equal(i, what):
        new = new_tokens(range(B), 1, dtype, 710 + 10 * i)
        ik.copy_(torch.stack([new[b][0] for b in range(B)])); iv.copy_(torch.stack([new[b][1] for b in range(B)]))
        iq.copy_(_rand((B, H, 1, D), dtype, 720 + i))
        graph.replay()
        for b in range(B):
            r.hist[b] = (torch.cat([r.hist[b][0], new[b][0]], 1), torch.cat([r.hist[b][1], new[b][1]], 1))
        assert same(ctx, r.twin().attend(iq, SCALE, causal=True)), what
        r.check(what)

    with torch.no_grad():
        r.c.reserve(1)
        step()                                                        # warm-up: code objects, the exponent window table, attend's workspace
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx = step()
        r.c.reset()                                                   # undo the warm-up and capture-time appends
        for name in BUFFERS:
            getattr(r.c, name).fill_(0x7f)
        fill(r, lens, 64, 700)
        r.c.reserve([n + 1 for n in lens])
        replay_equal(0, "replay before the fork")
        r.c.fork(1, [0, 2])                                           # rows 0 and 2 become row 1: the captured step reads the new table
        r.reordered([1, 1, 1, 3])
        r.c.reserve([n + 2 for n in r.lens()])
        for i in (1, 2):
            replay_equal(i, f"replay {i}, after the fork")
    assert r.c.lengths.tolist() == [36, 36, 36, 67] and r.c.overflow.item() == 0


# ---- 6. the guard: a wrong count gives an empty row, never one over pages it was not given --------------------------------------------------------
@pytest.mark.parametrize("dtype,block", FORMATS, ids=FIDS)
@pytest.mark.parametrize("wrong", [69, 64, 71, 5])
def test_a_wrong_count_leaves_the_destination_empty(dtype, block, wrong):
    with torch.no_grad():
        r = Rows(make(dtype, block, 64), dtype, block)
        fill(r, [70, 33, 40, 0], 64, 800)
        own = torch.tensor(r.c._owned[0], device=DEV)
        before = [getattr(r.c, name)[own].clone() for name in BUFFERS] + [r.c.v_tail[0].clone()]
        k0, v0 = r.c.keys(0), r.c.values(0)
        r.c.fork(0, 2, tokens=wrong)
        assert r.c.lengths.tolist() == [70, 33, 0, 0] and r.c.overflow.item() == 1
        assert all(torch.equal(a, b) for a, b in zip(before, [getattr(r.c, name)[own] for name in BUFFERS] + [r.c.v_tail[0]]))
        assert same(r.c.keys(0), k0) and same(r.c.values(0), v0)
        r.c.release(2)                                                # the way to reuse such a row
        r.c.overflow.zero_()
        r.c.fork(0, 2, tokens=70)
        r.reordered([0, 1, 0, 3])
        r.check("the fork with the right count")


# ---- 7. a beam search: reorder, reserve, append, step after step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,block", FORMATS, ids=FIDS)
def test_a_beam_search_of_ten_steps(dtype, block):
    """more reorders than the cache has upload buffers, across a page boundary (60 -> 70 tokens), sources shared from earlier steps"""
    steps = ([0, 0, 1, 3], [1, 0, 0, 3], [2, 2, 2, 2], [0, 1, 2, 3], [3, 0, 0, 1], [1, 1, 0, 0], [0, 2, 2, 3], [3, 2, 1, 0], [0, 0, 0, 1], [2, 3, 0, 1])
    with torch.no_grad():
        r = Rows(make(dtype, block, 64), dtype, block)
        fill(r, [60, 60, 60, 60], 64, 900)
        for i, index in enumerate(steps):
            n = 60 + i
            r.c.reorder(index, [n] * B)
            r.reordered(index)
            r.c.reserve(n + 1)
            r.append(new_tokens(range(B), 1, dtype, 910 + 10 * i))
            if i in (3, 5, 9):
                r.check(f"step {i}")
                refs, owned = r.c.page_refs, [p for o in r.c._owned for p in o]
                assert refs == [owned.count(p) for p in range(16)] and r.c.pages_free == refs.count(0)
        assert r.c.lengths.tolist() == [70] * B
