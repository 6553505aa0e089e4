"""GPU tests of the 4-bit HBFP KV cache (bfp_ops.HBFPKVCache(code_bits=4), csrc/bfpq_kvcache.hip).  The law needs no tolerance:
the codes are the same integers in a narrower store, so a code_bits=4 cache and an int8 twin with the same other arguments, fed the same
calls on the same data, give the same raw bits from scores, context, attend (with and without p, both routes), keys, values, lengths and
overflow (tests/util.assert_bits_equal: any NaN equals any NaN).

Shapes: batch 3, block 64, capacity 320; D 64 (one block per key row) with 2 heads, D 128 (two) with 4 heads over 2 kv heads; fp32 /
bf16 / fp16 against mant_bits 3 / 2 / 1 as a Latin square over the two head shapes (SQUARE: every dtype with every width).  The layout
of the code buffers is checked against tests/kvcache_c4_layout.py, the torch restatement."""
import pytest
import torch

from quantization_sparsity_interplay_amd.bfp import bfp_ops
import kvcache_c4_layout as layout
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, CAP, BLK = 3, 320, 64
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SHAPES = ((64, 2, 2), (128, 4, 2), (64, 4, 2))                        # D, heads, kv_heads
# row j: dtype i with mant_bits 3, 2, 1 rotated by j, on shape j
SQUARE = tuple((DTYPES[i], (3, 2, 1)[(i + j) % 3]) + SHAPES[j] for j in range(3) for i in range(3))
DIAG = SQUARE[0::4]                                                    # one case per dtype, per width and per shape
BUFFERS = ("k_codes", "k_exps", "v_codes", "v_exps")


def _id(case):
    dt, m, D, H, kvh = case
    return f"{str(dt).split('.')[-1]}-m{m}-d{D}-h{H}kv{kvh}"


def cfg(mant_bits):
    return dict(mant_bits=mant_bits, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=BLK, num_format='bfp', weight_mant_bits=15,
                in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s',
                sparsity_mode='structured')


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _rand(shape, dtype, seed):
    """magnitudes over many binades along the tokens (tests/test_kvcache_device_gpu.py)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-6, 4, shape[:-1] + (1,), generator=g).float())).to(dtype).to(DEV)


def eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert_bits_equal(bits(a), bits(b), a.dtype, what)


def mk(case, code_bits, capacity=CAP, **mode):
    dt, m, D, H, kvh = case
    return bfp_ops.HBFPKVCache(B, H, D, capacity, dtype=dt, device_lengths=True, kv_heads=kvh, code_bits=code_bits, **mode, **cfg(m))


def pair(case, **mode):
    """(the 4-bit cache, its int8 twin)"""
    return mk(case, 4, **mode), mk(case, None, **mode)


def held_equal(c, twin, what):
    assert c.lengths.tolist() == twin.lengths.tolist(), what
    assert c.overflow.item() == twin.overflow.item(), what
    for name in ("k_exps", "v_exps", "v_tail"):
        if c.pages is None or name == "v_tail":
            assert torch.equal(getattr(c, name), getattr(twin, name)), f"{what}: {name}"
    for b in range(c.batch):
        eq(c.keys(b), twin.keys(b), f"{what}: keys of sequence {b}")
        eq(c.values(b), twin.values(b), f"{what}: values of sequence {b}")


def codes_equal(c, twin, what):
    """the code buffers of a contiguous pair, below each length (K) and over whole token blocks (V): the twin's int8 codes, packed"""
    for b, n in enumerate(c.lengths.tolist()):
        assert torch.equal(c.k_codes[b, :, :n], layout.pack(twin.k_codes[b, :, :n])), f"{what}: k_codes of sequence {b}"
        nb = (n + BLK - 1) // BLK * BLK
        assert torch.equal(c.v_codes[b, :, :, :nb // 2], layout.pack(twin.v_codes[b, :, :, :nb])), f"{what}: v_codes of sequence {b}"
        assert torch.equal(layout.unpack(c.v_codes[b, :, :, :nb // 2]), twin.v_codes[b, :, :, :nb]), f"{what}: v_codes of sequence {b}, unpacked"


def routes_equal(c, twin, seed, what, Tqs=(3,), max_lens=(None,), causal=(True,)):
    """scores, context and attend (with and without p) of both caches on the same q"""
    dt, D, H = c.dtype, c.head_dim, c.heads
    for Tq in Tqs:
        q = _rand((c.batch, H, Tq, D), dt, seed + Tq)
        for ml in max_lens:
            for cz in causal:
                ctx, p = c.attend(q, D ** -0.5, max_len=ml, causal=cz, return_probs=True)
                want, pw = twin.attend(q, D ** -0.5, max_len=ml, causal=cz, return_probs=True)
                eq(ctx, want, f"{what}: attend Tq {Tq} max_len {ml} causal {cz}")
                eq(p, pw, f"{what}: p of attend Tq {Tq} max_len {ml} causal {cz}")
                eq(c.attend(q, D ** -0.5, max_len=ml, causal=cz), want, f"{what}: attend without p, Tq {Tq} max_len {ml} causal {cz}")
                if Tq <= 16:
                    eq(c.context(pw), twin.context(pw), f"{what}: context Tq {Tq} L {pw.shape[-1]}")
            if Tq <= 16:
                eq(c.scores(q, ml), twin.scores(q, ml), f"{what}: scores Tq {Tq} max_len {ml}")


# ---- 1. append -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SQUARE, ids=[_id(c) for c in SQUARE])
def test_append_stores_the_twins_codes_packed(case):
    dt, m, D, H, kvh = case
    steps = (63, 1, 1, 65, 70)                                          # 63, 64, 65, 130, 200: two hand-overs of the open block, odd and even positions
    k, v = _rand((B, kvh, sum(steps), D), dt, 100 + m), _rand((B, kvh, sum(steps), D), dt, 101 + m)
    with torch.no_grad():
        c, twin = pair(case)
        s0 = 0
        for i, t in enumerate(steps):
            for x in (c, twin):
                x.append(k[:, :, s0:s0 + t].contiguous(), v[:, :, s0:s0 + t].contiguous())
            s0 += t
            held_equal(c, twin, f"append {i}")
            codes_equal(c, twin, f"append {i}")
            routes_equal(c, twin, 110 + i, f"append {i}")
        assert c.lengths.tolist() == [200] * 3 and c.overflow.item() == 0
        # a chunk that would pass the capacity: refused, the bytes as they were, overflow raised as the twin raises it
        before = [getattr(c, n).clone() for n in BUFFERS + ("v_tail",)]
        for x in (c, twin):
            x.append(k[:, :, :130].contiguous(), v[:, :, :130].contiguous(), _i32(121, 0, 120))
        assert c.lengths.tolist() == [200, 200, 320] and c.overflow.item() == 1 and twin.overflow.item() == 1
        for n, was in zip(BUFFERS + ("v_tail",), before):
            assert torch.equal(getattr(c, n)[:2], was[:2]), f"the refused sequence's {n} changed"
        held_equal(c, twin, "after the refused chunk")
        codes_equal(c, twin, "after the refused chunk")
        # ragged counts on a fresh pair
        c, twin = pair(case)
        for x in (c, twin):
            x.append(k, v, _i32(200, 70, 1))
        assert c.lengths.tolist() == [200, 70, 1]
        held_equal(c, twin, "ragged")
        codes_equal(c, twin, "ragged")
        routes_equal(c, twin, 120, "ragged", causal=(False,))


# ---- 2. every code value -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split('.')[-1] for d in DTYPES])
def test_every_code_value_is_held_and_read_back(dtype):
    """mant_bits 3: a block whose largest magnitude is 7 s (s a power of two) has the step s, so j s is the code j exactly.  Key row 5 holds
    j = -7..7 at d = 0..14 (odd and even nibbles of both signs side by side), and column 9 of V holds them at tokens 0..14.  Every other
    block holds one 7 s, outside what q and p touch: an all-zero block has no scale where the dtype rounds epsilon to zero (fp16)"""
    case = (dtype, 3, 64, 2, 2)
    D, s = 64, 0.25
    js = torch.arange(-7, 8, dtype=torch.float32)
    k = torch.zeros(B, 2, 16, D)
    v = torch.zeros(B, 2, 16, D)
    k[:, :, :, 63] = 7 * s
    v[:, :, 0, :] = 7 * s
    k[:, :, 5:7, 63] = 0
    v[:, :, 0, 9:11] = 0
    k[:, :, 5, :15] = js * s
    k[:, :, 6, 1:16] = js.flip(0) * s                                   # the same codes in the other nibble
    v[:, :, :15, 9] = js * s
    v[:, :, 1:16, 10] = js.flip(0) * s
    k, v = k.to(dtype).to(DEV), v.to(dtype).to(DEV)
    with torch.no_grad():
        c, twin = pair(case)
        for x in (c, twin):
            x.append(k, v)
        held_equal(c, twin, "codes")
        codes_equal(c, twin, "codes")
        want = js.to(torch.int8).to(DEV)
        assert torch.equal(twin.k_codes[0, 0, 5, :15], want) and torch.equal(twin.v_codes[0, 0, 9, :15], want)   # the test's premise
        assert torch.equal(layout.unpack(c.k_codes)[0, 0, 5, :15], want) and torch.equal(layout.unpack(c.k_codes)[0, 0, 6, 1:16], want.flip(0))
        assert torch.equal(layout.unpack(c.v_codes)[0, 0, 9, :15], want) and torch.equal(layout.unpack(c.v_codes)[0, 0, 10, 1:16], want.flip(0))
        for b in range(B):
            eq(c.keys(b), k[b:b + 1], "keys() are the values")
            eq(c.values(b), v[b:b + 1], "values() are the values")
        # q row t = 1.5 e_t (1.5: the code 6 under the step 0.25; a power of two would be the largest of its block and saturate at 7):
        # scores[t][n] = 1.5 k[n][t], exact in every dtype; p row t = 1.5 e_t: context[t][d] = 1.5 v[t][d]
        q = (1.5 * torch.eye(16, D)).to(dtype).to(DEV).expand(B, 2, 16, D).contiguous()
        sc = c.scores(q, 16)
        eq(sc, twin.scores(q, 16), "scores of single elements")
        eq(sc, (1.5 * k[..., :16].float()).to(dtype).transpose(-1, -2).contiguous(), "scores of single elements read the codes back")
        p = (1.5 * torch.eye(16, 16)).to(dtype).to(DEV).expand(B, 2, 16, 16).contiguous()
        ctx = c.context(p)
        eq(ctx, twin.context(p), "context of single elements")
        eq(ctx, (1.5 * v.float()).to(dtype), "context of single elements reads the codes back")


# ---- 3. the ends of the exponent range -----------------------------------------------------------------------------------------------------
# (largest, smallest) power of two the blocks are scaled to: both ends of the int8 block exponent in fp32 and bf16, of the dtype in fp16
ENDS = {torch.float32: (125, -140), torch.bfloat16: (125, -130), torch.float16: (13, -22)}


@pytest.mark.parametrize("case", DIAG, ids=[_id(c) for c in DIAG])
def test_exponent_range_ends_give_the_twins_bits(case):
    dt, m, D, H, kvh = case
    hi, lo = ENDS[dt]
    g = torch.Generator().manual_seed(300 + m)
    base_k, base_v = torch.randn(B, kvh, 130, D, generator=g), torch.randn(B, kvh, 130, D, generator=g)
    base_q = torch.randn(B, H, 2, D, generator=g)
    base_p = torch.rand(B, H, 2, 130, generator=g)
    inf_or_zero = 0
    with torch.no_grad():
        for ekv in (hi, lo):
            c, twin = pair(case)
            # sequence 0 at the end itself, sequence 1 a few binades inside it, sequence 2 mixing both ends block by block
            scale = torch.full((B, 1, 130, 1), float(ekv))
            scale[1] += 3.0 if ekv == lo else -3.0
            scale[2, :, 64:] = float(hi if ekv == lo else lo)
            k, v = ((x.double() * torch.exp2(scale.double())).to(dt).to(DEV) for x in (base_k, base_v))
            for x in (c, twin):
                x.append(k, v)
            held_equal(c, twin, f"K, V at 2^{ekv}")
            codes_equal(c, twin, f"K, V at 2^{ekv}")
            for eq_ in (hi, lo, 0):
                q = (base_q.double() * 2.0 ** eq_).to(dt).to(DEV)
                p = (base_p.double() * 2.0 ** min(eq_, 0)).to(dt).to(DEV)
                what = f"K, V at 2^{ekv}, q at 2^{eq_}"
                sc, sw = c.scores(q), twin.scores(q)
                eq(sc, sw, what + ": scores")
                cx, cw = c.context(p), twin.context(p)
                eq(cx, cw, what + ": context")
                inf_or_zero += int(torch.isinf(sw[..., :130]).any()) + int((sw[..., :130] == 0).any()) + int((cw == 0).any())
                for scale_a in (1.0, 2.0 ** -100 if dt != torch.float16 else 2.0 ** -14):
                    got, pg = c.attend(q, scale_a, return_probs=True)
                    want, pw = twin.attend(q, scale_a, return_probs=True)
                    eq(got, want, what + f": attend, scale {scale_a}")
                    eq(pg, pw, what + f": p of attend, scale {scale_a}")
    assert inf_or_zero > 0                                              # the ends were reached: some result overflowed or flushed


# ---- 4. NaN ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DIAG, ids=[_id(c) for c in DIAG])
def test_nan_blocks_reach_the_twins_outputs(case):
    dt, m, D, H, kvh = case
    k, v = _rand((B, kvh, 130, D), dt, 400 + m), _rand((B, kvh, 130, D), dt, 401 + m)
    k[0, 0, 17, 3] = float('nan')                                       # one key row
    v[1, kvh - 1, 40, D - 2] = float('nan')                             # one closed token block of V
    v[2, 0, 129, 1] = float('inf')                                      # and an infinity in the open one
    with torch.no_grad():
        c, twin = pair(case)
        for x in (c, twin):
            x.append(k, v)
        assert (twin.k_exps == -128).any() and (twin.v_exps == -128).any()   # the marker is an exponent byte, not a code
        held_equal(c, twin, "NaN")
        routes_equal(c, twin, 410, "NaN", Tqs=(1, 16), causal=(True, False))
        q = _rand((B, H, 3, D), dt, 420)
        assert torch.isnan(c.scores(q)[0, 0, :, 17]).all() and torch.isnan(c.attend(q, 0.125)[1, H - 1]).any()


# ---- 5. routes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SQUARE, ids=[_id(c) for c in SQUARE])
def test_decode_routes_equal_the_twin(case):
    dt, m, D, H, kvh = case
    k, v = _rand((B, kvh, 300, D), dt, 500 + m), _rand((B, kvh, 300, D), dt, 501 + m)
    with torch.no_grad():
        for cps in (0, 1, 2):
            c, twin = pair(case, chunks_per_split=cps)
            for x in (c, twin):
                x.append(k, v, _i32(300, 129, 64))
            routes_equal(c, twin, 510 + cps, f"chunks_per_split {cps}", Tqs=(1, 3, 16) if cps == 0 else (3,), max_lens=(None, 256, 128),
                         causal=(True, False))


@pytest.mark.parametrize("case", DIAG, ids=[_id(c) for c in DIAG])
@pytest.mark.parametrize("prompt_rows", (16, 32))
def test_prompt_panels_equal_the_twin(case, prompt_rows):
    dt, m, D, H, kvh = case
    k, v, q = (_rand((B, n, 80, D), dt, 600 + m + i) for i, n in enumerate((kvh, kvh, H)))
    with torch.no_grad():
        for Tq in (17, 48, 80):                                          # whole: the Tq tokens appended, then attended at once
            c, twin = pair(case, prompt_rows=prompt_rows)
            for x in (c, twin):
                x.append(k[:, :, :Tq].contiguous(), v[:, :, :Tq].contiguous(), _i32(Tq, Tq - 5, 1))
            for ml, cz in ((None, True), (256, False), (128, True)):
                got, p = c.attend(q[:, :, :Tq].contiguous(), D ** -0.5, max_len=ml, causal=cz, return_probs=True)
                want, pw = twin.attend(q[:, :, :Tq].contiguous(), D ** -0.5, max_len=ml, causal=cz, return_probs=True)
                eq(got, want, f"Tq {Tq} max_len {ml} causal {cz}")
                eq(p, pw, f"p, Tq {Tq} max_len {ml} causal {cz}")
                eq(c.attend(q[:, :, :Tq].contiguous(), D ** -0.5, max_len=ml, causal=cz), want, f"without p, Tq {Tq} max_len {ml} causal {cz}")
        c, twin = pair(case, prompt_rows=prompt_rows)                    # in chunks of 17, 48 and the 15 left
        for s0, s1 in ((0, 17), (17, 65), (65, 80)):
            for x in (c, twin):
                x.append(k[:, :, s0:s1].contiguous(), v[:, :, s0:s1].contiguous())
            got, p = c.attend(q[:, :, s0:s1].contiguous(), D ** -0.5, causal=True, return_probs=True)
            want, pw = twin.attend(q[:, :, s0:s1].contiguous(), D ** -0.5, causal=True, return_probs=True)
            eq(got, want, f"the chunk from {s0}")
            eq(p, pw, f"p of the chunk from {s0}")
        held_equal(c, twin, "the prompt in chunks")


@pytest.mark.parametrize("case", [c for c in DIAG if c[3] != c[4]], ids=[_id(c) for c in DIAG if c[3] != c[4]])
def test_grouped_cache_equals_its_repeated_twin(case):
    dt, m, D, H, kvh = case
    g = H // kvh
    k, v = _rand((B, kvh, 131, D), dt, 700 + m), _rand((B, kvh, 131, D), dt, 701 + m)
    with torch.no_grad():
        c = mk(case, 4, prompt_rows=16)
        rep = mk((dt, m, D, H, H), 4, prompt_rows=16)                    # code_bits=4 too: H kv heads fed the repeated K and V
        c.append(k, v, _i32(131, 64, 17))
        rep.append(k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), _i32(131, 64, 17))
        routes_equal(c, rep, 710, "grouped", Tqs=(1, 16, 40), max_lens=(None, 128), causal=(True, False))
        for b in range(B):
            eq(c.keys(b).repeat_interleave(g, 1), rep.keys(b), "keys")
            eq(c.values(b).repeat_interleave(g, 1), rep.values(b), "values")


# ---- 6. windows and starts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DIAG, ids=[_id(c) for c in DIAG])
@pytest.mark.parametrize("window", (None, 50, 64))
def test_first_keys_equal_the_twin(case, window):
    dt, m, D, H, kvh = case
    k, v = _rand((B, kvh, 200, D), dt, 800 + m), _rand((B, kvh, 200, D), dt, 801 + m)
    with torch.no_grad():
        c, twin = pair(case, starts=True, window=window, prompt_rows=32)
        for x in (c, twin):
            x.append(k, v, _i32(200, 150, 131))
            x.starts.copy_(_i32(0, 37, 130))
        routes_equal(c, twin, 810, f"window {window}", Tqs=(1, 16, 48), max_lens=(None, 128), causal=(True, False))
        held_equal(c, twin, f"window {window}")


# ---- 7. paged --------------------------------------------------------------------------------------------------------------------------------
def scattered(b, W):
    """sequence b's pages in token order: scattered and decreasing"""
    return [W * B - 1 - b - B * i for i in range(W)]


def stale(c):
    for name in BUFFERS:
        getattr(c, name).fill_(0x7f)


def paged_pair(case, PT, give=None, capacity=CAP, **mode):
    """(the paged 4-bit cache, the paged int8 twin), pools pre-filled with 0x7f bytes, the same scattered table"""
    W = capacity // PT
    out = []
    for cb in (4, None):
        x = mk(case, cb, capacity=capacity, page_tokens=PT, pages=W * B + 2, **mode)
        stale(x)
        for b in range(B):
            x.assign(b, scattered(b, W)[:W if give is None else give[b]])
        out.append(x)
    return out


@pytest.mark.parametrize("case,PT", [(c, 64) for c in DIAG] + [(DIAG[1], 128)], ids=[_id(c) + "-p64" for c in DIAG] + [_id(DIAG[1]) + "-p128"])
def test_paged_cache_equals_the_contiguous_one_and_the_paged_twin(case, PT):
    dt, m, D, H, kvh = case
    cap = 320 if PT == 64 else 384                                       # (a multiple of the page)
    k, v = _rand((B, kvh, 201, D), dt, 900 + m), _rand((B, kvh, 201, D), dt, 901 + m)
    q48 = _rand((B, H, 48, D), dt, 902 + m)
    with torch.no_grad():
        c, twin = paged_pair(case, PT, capacity=cap, prompt_rows=16)
        flat = mk(case, 4, capacity=cap, prompt_rows=16)                 # the contiguous 4-bit cache
        s0 = 0
        for t, counts in ((63, (63, 60, 17)), (1, (1, 1, 0)), (1, (1, 0, 1)), (65, (65, 65, 3)), (70, (70, 1, 0))):
            for x in (c, twin, flat):
                x.append(k[:, :, s0:s0 + t].contiguous(), v[:, :, s0:s0 + t].contiguous(), _i32(*counts))
            s0 += t
            held_equal(c, twin, f"append at {s0}")
            held_equal(c, flat, f"append at {s0}, against the contiguous cache")
        assert c.lengths.tolist() == [200, 127, 21] and c.overflow.item() == 0
        for other, name in ((twin, "the paged int8 twin"), (flat, "the contiguous 4-bit cache")):
            routes_equal(c, other, 910, name, Tqs=(1, 16), max_lens=(None, 128), causal=(True, False))
            eq(c.attend(q48, D ** -0.5, causal=True), other.attend(q48, D ** -0.5, causal=True), name + ": the prompt route")
        # the pool holds the twin's codes packed, page for page, and 0x7f wherever no token was written
        for b, n in enumerate(c.lengths.tolist()):
            for i, pg in enumerate(c._owned[b]):
                rows = max(0, min(PT, n - i * PT))
                assert torch.equal(c.k_codes[pg, :, :rows], layout.pack(twin.k_codes[pg, :, :rows])), (b, i)
                assert (c.k_codes[pg, :, rows:] == 0x7f).all() and (twin.k_codes[pg, :, rows:] == 0x7f).all(), (b, i)
                nb = (rows + BLK - 1) // BLK * BLK
                assert torch.equal(c.v_codes[pg, :, :, :nb // 2], layout.pack(twin.v_codes[pg, :, :, :nb])), (b, i)
                assert (c.v_codes[pg, :, :, nb // 2:] == 0x7f).all(), (b, i)
        for pg in c._free:
            assert all((getattr(c, name)[pg] == 0x7f).all() for name in BUFFERS), pg


@pytest.mark.parametrize("case", DIAG[:2], ids=[_id(c) for c in DIAG[:2]])
def test_a_missing_page_refuses_the_sequence(case):
    dt, m, D, H, kvh = case
    k, v = _rand((B, kvh, 70, D), dt, 950 + m), _rand((B, kvh, 70, D), dt, 951 + m)
    with torch.no_grad():
        c, twin = paged_pair(case, 64, give=(1, 2, 2))
        for x in (c, twin):
            x.append(k[:, :, :60].contiguous(), v[:, :, :60].contiguous(), _i32(60, 60, 3))
        before = [getattr(c, n)[c._owned[0][0]].clone() for n in BUFFERS] + [c.v_tail[0].clone()]
        for x in (c, twin):
            x.append(k[:, :, 60:70].contiguous(), v[:, :, 60:70].contiguous())       # tokens 60 .. 69 of sequence 0: the last six have no page
        assert c.lengths.tolist() == [60, 70, 13] and c.overflow.item() == 1 and twin.overflow.item() == 1
        after = [getattr(c, n)[c._owned[0][0]] for n in BUFFERS] + [c.v_tail[0]]
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "the refused sequence's page or tail changed"
        held_equal(c, twin, "after the refusal")
        routes_equal(c, twin, 960, "after the refusal")


@pytest.mark.parametrize("case", DIAG[:2], ids=[_id(c) for c in DIAG[:2]])
def test_fork_and_reorder_share_pages_as_the_twin(case):
    dt, m, D, H, kvh = case
    k, v = _rand((B, kvh, 140, D), dt, 970 + m), _rand((B, kvh, 140, D), dt, 971 + m)
    with torch.no_grad():
        # fork at L 70: one full page shared, the open one copied
        c, twin = paged_pair(case, 64, give=(2, 0, 0))
        for x in (c, twin):
            x.append(k[:, :, :70].contiguous(), v[:, :, :70].contiguous(), _i32(70, 0, 0))
        pool = {n: getattr(c, n).clone() for n in BUFFERS}
        for x in (c, twin):
            x.fork(0, [1, 2], tokens=70)
        assert c._owned == twin._owned and c.pages_shared == 1 and c.lengths.tolist() == [70, 70, 70]
        fresh = [c._owned[1][1], c._owned[2][1]]
        for n in BUFFERS:                                                # outside the copied pages the pool is untouched, byte for byte
            now = getattr(c, n)
            keep = torch.ones(now.shape[0], dtype=torch.bool, device=DEV)
            keep[torch.tensor(fresh, device=DEV)] = False
            assert torch.equal(now[keep], pool[n][keep]), n
            for pg in fresh:
                assert torch.equal(now[pg], now[c._owned[0][1]]), (n, pg)
        held_equal(c, twin, "fork")
        for x in (c, twin):
            x.reserve(140)
        for i, (a, b_) in enumerate(((70, 100), (100, 140))):             # diverging appends: each sequence takes other tokens
            for x in (c, twin):
                x.append(k[:, :, a:b_].roll(i + 1, 0).contiguous(), v[:, :, a:b_].roll(i + 1, 0).contiguous(), _i32(b_ - a, b_ - a - 7, 1))
            held_equal(c, twin, f"fork, append {i}")
        routes_equal(c, twin, 980, "fork", Tqs=(1, 16), causal=(True, False))
        # reorder([1, 0, 0]) on ragged lengths
        c, twin = paged_pair(case, 64, give=(3, 2, 1))
        for x in (c, twin):
            x.append(k, v, _i32(140, 70, 5))
            x.reorder([1, 0, 0], tokens=[140, 70, 5])
        assert c._owned == twin._owned and c.lengths.tolist() == [70, 140, 140] and c.overflow.item() == 0
        held_equal(c, twin, "reorder")
        for x in (c, twin):
            x.reserve(200)
            x.append(k[:, :, :40].roll(1, 0).contiguous(), v[:, :, :40].roll(1, 0).contiguous(), _i32(40, 1, 33))
        held_equal(c, twin, "reorder, then append")
        routes_equal(c, twin, 990, "reorder", Tqs=(1, 16), causal=(True, False))


# ---- 8. graph replay -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("case", DIAG[:2], ids=[_id(c) for c in DIAG[:2]])
def test_captured_step_replays_across_the_block_and_page_boundary(case, paged):
    dt, m, D, H, kvh = case
    start, steps, scale = (62, 5, 127), 5, D ** -0.5
    k, v = _rand((B, kvh, max(start) + steps, D), dt, 1000 + m), _rand((B, kvh, max(start) + steps, D), dt, 1001 + m)
    qs = [_rand((B, H, 1, D), dt, 1010 + i) for i in range(steps)]
    c, twin = paged_pair(case, 64, give=(2, 1, 3)) if paged else pair(case)
    sk, sv, ik, iv = (torch.zeros(B, kvh, 1, D, dtype=dt, device=DEV) for _ in range(4))
    sq, iq = (torch.zeros(B, H, 1, D, dtype=dt, device=DEV) for _ in range(2))

    def step():
        sk.copy_(ik); sv.copy_(iv); sq.copy_(iq)
        c.append(sk, sv)
        return c.attend(sq, scale, causal=True)

    def restart(x):
        x.lengths.zero_()
        x.overflow.zero_()
        x.append(k[:, :, :max(start)].contiguous(), v[:, :, :max(start)].contiguous(), _i32(*start))

    with torch.no_grad():
        c.prepare_attend()
        twin.prepare_attend()                                            # (the twin's workspace is not the replays' allocation)
        ws = (c._att_ws, c._ws)
        step()                                                           # warm-up: code objects, the exponent window table
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx = step()
        restart(c)
        restart(twin)
        held = torch.cuda.memory_allocated()
        for i in range(steps):                                           # sequence 0: 62 -> 67, over the block and the page boundary
            n = max(start) + i
            ik.copy_(k[:, :, n:n + 1]); iv.copy_(v[:, :, n:n + 1]); iq.copy_(qs[i])
            graph.replay()
            twin.append(ik, iv)
            want = twin.attend(iq, scale, causal=True)
            eq(ctx, want, f"replay {i}")
            del want
            assert torch.cuda.memory_allocated() == held, f"replay {i} allocated"
        held_equal(c, twin, "after the replays")
        assert c.lengths.tolist() == [s + steps for s in start] and c.overflow.item() == 0
        assert c._att_ws is ws[0] and c._ws is ws[1]                      # nothing was made after prepare_attend()
