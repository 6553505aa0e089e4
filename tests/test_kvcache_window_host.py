"""Host-side checks of the first visible key per row on the HBFP KV cache (HBFPKVCache(window=W, starts=True)): the two new C
entries (exported, declared with the signatures native.py binds -- the entries they extend with `starts` and `window` in front of the
stream -- every refusal before a launch), the Python refusals on device='meta', a cache with neither being today's cache, and att_first
of csrc/bfpq_kvcache.hip restated in Python against a brute-force mask.  No GPU needed: the pointers are not memory."""
import ctypes
import os
import re

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_kv_attend_gqa_win", "bfpq_kv_attend_rows_win")
P = ctypes.c_void_p(16)
Z = None
S = ctypes.c_void_p(0)
BLOCKS = (16, 32, 64)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bfpq.h")


def L():
    return native.load_library()


def _args(**kw):
    base = dict(num_format='bfp', sparsity_num_format='bfp', rounding_mode='determ', block_size=64, mant_bits=7, epsilon=1e-8)
    base.update(kw)
    return dict(bfp_ops.unpack_bfp_args(base), device='meta')


def _ctype(param):
    if '*' in param:
        return ctypes.c_void_p
    for word, t in (('int64_t', ctypes.c_int64), ('double', ctypes.c_double), ('int', ctypes.c_int)):
        if re.search(rf"\b{word}\b", param):
            return t
    raise AssertionError(param)


def test_new_entries_are_exported_and_declared_as_bound():
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW) <= set(native.EXPORTED_SYMBOLS)
    declared = {}
    for name in NEW + ("bfpq_kv_attend_gqa", "bfpq_kv_attend_rows"):
        assert hasattr(L(), name), name
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/bfpq.h"
        restype, argtypes = native.PROTOTYPES[name]
        assert restype is ctypes.c_int, name
        declared[name] = [a.strip() for a in m.group(1).split(',')]
        assert [_ctype(a) for a in declared[name]] == list(argtypes), name
    for name in NEW:
        old, new = declared[name[:-4]], declared[name]
        assert new[:-3] == old[:-1] and new[-1] == old[-1], name                       # the entry it extends, and two more in front of the stream
        assert re.fullmatch(r"const int32_t\s*\*\s*starts\w*", new[-3]) and re.fullmatch(r"int64_t\s+window", new[-2]), name
        assert list(native.PROTOTYPES[name][1]) == list(native.PROTOTYPES[name[:-4]][1][:-1]) + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    comment = text[:text.index("int bfpq_kv_attend_gqa_win")].rsplit("/*", 1)[1]
    assert "modeling_gpt2.py:228-230" in comment and "modeling_llama.py:402-404" in comment and "sliding_window" in comment


# the arguments of bfpq_kv_attend_gqa_win; rows_win has row0 and rows in front of starts
def gqa(*, q=P, kc=P, ke=P, vc=P, ve=P, out=P, p=Z, ln=P, BH=4, heads=2, Tq=3, g=4, D=64, ml=100, cap=128, ldd=64, ldo=64, ldp=100,
        scale=0.125, causal=0, dt=2, blk=64, xm=7, wm=7, win=P, sws=P, swb=1 << 40, pws=P, pwb=1 << 40, cps=0, st=P, W=50):
    return L().bfpq_kv_attend_gqa_win(q, kc, ke, vc, ve, out, p, ln, BH, heads, Tq, g, D, ml, cap, ldd, ldo, ldp, scale, causal, dt, blk, xm, wm, 1e-8,
                                      win, sws, swb, pws, pwb, cps, st, W, S)


def rows(*, q=P, kc=P, ke=P, vc=P, ve=P, out=P, p=Z, ln=P, BH=4, heads=2, Tq=100, g=4, D=64, ml=100, cap=128, ldd=64, ldo=64, ldp=100,
         scale=0.125, causal=0, dt=2, blk=64, xm=7, wm=7, win=P, sws=P, swb=1 << 40, pws=Z, pwb=0, cps=0, row0=32, n=48, st=P, W=50):
    return L().bfpq_kv_attend_rows_win(q, kc, ke, vc, ve, out, p, ln, BH, heads, Tq, g, D, ml, cap, ldd, ldo, ldp, scale, causal, dt, blk, xm, wm, 1e-8,
                                       win, sws, swb, pws, pwb, cps, row0, n, st, W, S)


@pytest.mark.parametrize("blk", BLOCKS)
@pytest.mark.parametrize("entry", (gqa, rows), ids=("gqa_win", "rows_win"))
def test_win_entries_refuse_before_any_launch(entry, blk):
    """window < 0 and a misaligned starts: BFPQ_E_ARG; everything else as the entry each extends, with every (starts, window) form"""
    for kw in (dict(W=-1), dict(W=-(1 << 40)), dict(st=ctypes.c_void_p(18)), dict(st=ctypes.c_void_p(17), W=0)):
        assert entry(blk=blk, **kw) == E_ARG, kw
        assert entry(blk=blk, q=Z, ml=0, **kw) == E_ARG, kw                            # (a value: before the shapes)
    forms = (dict(), dict(st=Z), dict(W=0), dict(st=Z, W=0), dict(W=1 << 40))
    for form in forms:
        for kw in (dict(dt=3), dict(xm=0), dict(wm=8), dict(blk=48), dict(BH=-2), dict(Tq=-1), dict(heads=0), dict(heads=3), dict(g=0),
                   dict(cps=-1), dict(causal=2), dict(scale=float('nan')), dict(scale=float('inf')), dict(scale=1e300)):
            assert entry(**dict(dict(blk=blk), **kw, **form)) == E_ARG, (kw, form)
        for kw in (dict(g=1 << 31), dict(ml=0), dict(ml=129), dict(cap=100), dict(D=8), dict(ldd=32), dict(ldo=62), dict(p=P, ldp=99), dict(cps=17),
                   dict(swb=15)):
            assert entry(blk=blk, **kw, **form) == E_UNSUPPORTED, (kw, form)
        assert entry(blk=blk, BH=0, **form) == 0 and entry(blk=blk, Tq=0, **(dict(row0=0, n=0) if entry is rows else {}), **form) == 0
        for name in ("q", "kc", "ke", "vc", "ve", "out", "ln", "win", "sws"):
            assert entry(blk=blk, **{name: Z}, **form) == E_ARG, (name, form)          # taken up to the null: nothing was launched
        assert entry(blk=blk, p=ctypes.c_void_p(17), **form) == E_ARG
    assert gqa(blk=blk, Tq=17) == E_UNSUPPORTED and gqa(blk=blk, pwb=15) == E_UNSUPPORTED and gqa(blk=blk, pws=Z) == E_ARG
    for kw in (dict(row0=-1), dict(n=-1), dict(row0=60, n=41)):
        assert rows(blk=blk, **kw) == E_ARG, kw
    assert rows(blk=blk, n=0) == 0 and rows(blk=blk, D=320, ldd=320, ldo=320) == E_UNSUPPORTED


def test_python_refusals_come_before_any_launch():
    a = _args()
    mk = lambda **kw: bfp_ops.HBFPKVCache(2, 4, 64, 320, dtype=torch.bfloat16, **dict(a, **kw))
    for bad in (True, False, 16.0, "32", (4,)):
        with pytest.raises(TypeError, match="window"):
            mk(device_lengths=True, window=bad)
    for bad in (0, -1, -64):
        with pytest.raises(ValueError, match="window"):
            mk(device_lengths=True, window=bad)
    for bad in (1, 0, None, "yes", torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(TypeError, match="starts"):
            mk(device_lengths=True, starts=bad)
    with pytest.raises(ValueError, match="window needs device_lengths"):
        mk(window=16)
    with pytest.raises(ValueError, match="starts needs device_lengths"):
        mk(starts=True)
    mk(starts=False)                                                                   # the host-length cache, as today
    q = torch.zeros(2, 4, 17, 64, dtype=torch.bfloat16, device='meta')
    cache = mk(device_lengths=True, window=16, starts=True)
    long = mk(device_lengths=True, window=16, starts=True, prompt_rows=32, kv_heads=2, chunks_per_split=2, max_query_rows=4)
    assert cache.window == long.window == 16 and cache.starts.shape == (2,) and cache.starts.dtype == torch.int32
    with torch.no_grad():
        with pytest.raises(ValueError, match="up to 16 query rows"):
            cache.attend(q, 0.125)                                                     # every refusal of attend() stays
        with pytest.raises(ValueError, match="max_query_rows"):
            long.attend(q[:, :, :5], 0.125)
        with pytest.raises(ValueError, match="scale"):
            long.attend(q, float('nan'))
        with pytest.raises(ValueError, match="max_len"):
            long.attend(q, 0.125, max_len=321)
        for f in (long.scores, lambda x: long.context(torch.zeros(2, 4, 17, 320, dtype=torch.bfloat16, device='meta'))):
            with pytest.raises(ValueError, match="up to 16 query rows"):
                f(q)
    with pytest.raises(ValueError, match="inference only"):
        long.attend(q, 0.125)
    for bad in (True, 2.0, 0, -3):                                                     # the binding refuses what the class does
        with pytest.raises(ValueError, match="window"):
            native._kv_window("kv_attend", 8, 4, None, bad, torch.device('meta'))
    for bad in (torch.zeros(3, dtype=torch.int32, device='meta'), torch.zeros(2, dtype=torch.int64, device='meta'), [0, 0]):
        with pytest.raises(ValueError, match="starts"):
            native._kv_window("kv_attend", 8, 4, bad, None, torch.device('meta'))
    assert native._kv_window("kv_attend", 8, 4, None, None, torch.device('meta')) == (None, 0)


@pytest.mark.parametrize("kv_heads", (None, 2))
def test_neither_is_todays_cache(kv_heads):
    a = _args()
    mk = lambda **kw: bfp_ops.HBFPKVCache(2, 4, 64, 320, dtype=torch.bfloat16, device_lengths=True, kv_heads=kv_heads, prompt_rows=32, **dict(a, **kw))
    plain, none, both = mk(), mk(window=None, starts=False), mk(window=100, starts=True)
    today = {'args', 'act', 'device_lengths', 'chunks_per_split', 'max_query_rows', 'prompt_rows', 'batch', 'heads', 'head_dim', 'capacity', 'dtype',
             'kv_heads', 'group', 'block', 'mant_bits', 'epsilon', 'cap', 'stats', '_length', 'buffers', 'k_codes', 'k_exps', 'v_codes', 'v_exps',
             'v_tail', 'lengths', 'overflow', '_ws', '_att_ws', '_rows_ws'}
    assert set(vars(plain)) == set(vars(none)) == today                                # the attributes of the cache before window / starts
    assert set(vars(both)) == today | {'window', 'starts'}
    assert plain.window is None and plain.starts is None and none.window is None and none.starts is None
    g = 4 // (kv_heads or 4)
    want = 2 * (4 // g) * (320 * 64 + 320 + 64 * 320 + 64 * 5 + 64 * 64 * 2)           # k codes and exps, v codes and exps, the bf16 tail
    assert plain.nbytes() == none.nbytes() == both.nbytes() == want                    # starts is no buffer of the cache
    for name, value in vars(plain).items():
        other = vars(none)[name]
        if isinstance(value, torch.Tensor):
            assert (value.shape, value.dtype, value.device) == (other.shape, other.dtype, other.device), name
        elif name not in ('buffers', 'stats', 'act'):
            assert value == other, name
    for c in (plain, both):
        c.prepare_attend()                                                             # the same workspaces: no new one
    assert plain._att_ws.numel() == both._att_ws.numel() and plain._rows_ws.numel() == both._rows_ws.numel()
    assert plain._ws.numel() == both._ws.numel()
    op = bfp_ops.F_matmul_bfp(matrix_unit='int8', **{k: v for k, v in a.items() if k != 'device'}, device='meta')
    via = op.kv_cache(2, 4, 64, 320, device='meta', device_lengths=True, window=7, starts=True)
    assert via.window == 7 and via.starts is not None and via.stats is op.matmul_stats
    with pytest.raises(TypeError):
        op.kv_cache(2, 4, 64, 320, device='meta', device_lengths=True, window=7.5)


# ---- att_first and att_visible of csrc/bfpq_kvcache.hip, restated ----------------------------------------------------------------------------
def att_visible(ln, Kx, Tq, t, causal):
    v = ln - Tq + t + 1 if causal else ln
    return min(max(v, 0), Kx)


def att_first(ln, Tq, t, causal, start, window):
    lo = max(start, 0)
    if window <= 0:
        return lo
    v = ln - Tq + t + 1 if causal else ln
    return max(lo, v - window if v > window else 0)


def range_first(a, e, rows, row0, ln, Tq, causal, start, window):
    t = row0 if a // rows != e // rows else row0 + a % rows
    return att_first(ln, Tq, t, causal, start, window)


def test_att_first_against_a_brute_force_mask():
    """the mask the reference builds: key n is seen by the token at position i = len - Tq + t (causal: n <= i; window: n > i - W, the
    last W up to its own) unless n is a pad token (n < start) or past max_len.  This checks the definition, not the kernel: what ties
    the HIP att_first to it is _bounds() of tests/test_kvcache_window_gpu.py, the same formula, which every GPU test there compares p
    against.  The restatement is also held to the text of the .hip file's helper and to a cache that takes window / starts"""
    src = open(os.path.join(os.path.dirname(HEADER), "..", "quantization-sparsity-interplay_amd", "csrc", "bfpq_kvcache.hip")).read()
    body = src[src.index("int att_first(int len, int Tq, int t, int causal, int start, int window)"):]
    body = body[:body.index("\n}\n")]
    for line in ("const int lo = start > 0 ? start : 0;", "if (window <= 0) return lo;", "const int v = causal ? len - Tq + t + 1 : len;",
                 "const int w = v > window ? v - window : 0;", "return w > lo ? w : lo;"):
        assert line in body, line
    cache = bfp_ops.HBFPKVCache(2, 4, 64, 320, dtype=torch.bfloat16, device_lengths=True, window=5, starts=True, **_args())
    assert cache.window == 5 and cache.starts.shape == (2,)
    for ln in range(0, 12):
        for Tq in range(1, 8):
            for causal in (0, 1):
                for start in (-2, 0, 1, 5, ln, ln + 3):
                    for W in (0, 1, 2, 5, 20):
                        for max_len in (4, 16):
                            Kx = min(ln, max_len)
                            los = []
                            for t in range(Tq):
                                i = ln - Tq + t if causal else ln - 1                  # the last key the row may see
                                mask = [n <= i and n < Kx and n >= start and (W == 0 or n > i - W) for n in range(16)]
                                lo, hi = att_first(ln, Tq, t, causal, start, W), att_visible(ln, Kx, Tq, t, causal)
                                assert mask == [lo <= n < hi for n in range(16)], (ln, Tq, causal, start, W, max_len, t)
                                los.append(lo)
                            assert los == sorted(los)                                  # lo does not decrease with the token
                            for rows_ in (1, 2, Tq):                                   # range_first: the least lo of a range of panel rows
                                for row0 in range(0, Tq - rows_ + 1):
                                    for a in range(2 * rows_):
                                        for e in range(a, 2 * rows_):
                                            least = min(los[row0 + p % rows_] for p in range(a, e + 1))
                                            got = range_first(a, e, rows_, row0, ln, Tq, causal, start, W)
                                            assert got <= least and (a // rows_ != e // rows_ or got == least)
