"""Host-side checks of grouped-query attention on the HBFP KV cache (HBFPKVCache(kv_heads=...)): the two C entries (exported,
declared with the signatures native.py binds, the old entries their group = 1 case, every refusal before a launch), the sizes -- the
buffers a g-th of the twin's, the workspaces the twin's -- and the Python refusals.  No GPU needed: the pointers are not memory."""
import ctypes
import os
import re

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_kv_bmm_dec_gqa", "bfpq_kv_attend_gqa")
P = ctypes.c_void_p(16)
Z = None
S = ctypes.c_void_p(0)
BLOCKS = (16, 32, 64)
QK, PV = native.KV_QK, native.KV_PV
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
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert set(NEW) <= set(native.EXPORTED_SYMBOLS)
    for name in NEW:
        assert hasattr(L(), name), name
        m = re.search(rf"\b(int64_t|int)\s+{name}\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/bfpq.h"
        restype, argtypes = native.PROTOTYPES[name]
        assert restype is ctypes.c_int and m.group(1) == 'int', name
        assert [_ctype(a) for a in m.group(2).split(',')] == list(argtypes), name
        old = native.PROTOTYPES[name.replace("_gqa", "_dev" if "bmm" in name else "")][1]
        assert len(argtypes) == len(old) + 1                                           # the old entry's arguments and `group`
    assert "modeling_llama.py:397-409" in open(HEADER).read()                          # the reference lines the entries replace


# bmm(x, wcodes, wexp, out, lens, B, heads, Tq, group, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, family, dtype, block, xm, wm, epsilon, exp_win,
#     ws, ws_bytes, chunks_per_split, stream)
def bmm(*, x=P, wc=P, we=P, out=P, ln=P, B=4, heads=2, Tq=1, g=4, Kx=64, Nout=100, ldx=64, ldw=64, ldwe=4, wbs=128, ldo=100, fam=QK, dt=2,
        blk=64, xm=7, wm=7, win=P, ws=P, wsb=1 << 40, cps=0):
    return L().bfpq_kv_bmm_dec_gqa(x, wc, we, out, ln, B, heads, Tq, g, Kx, Nout, ldx, ldw, ldwe, wbs, ldo, fam, dt, blk, xm, wm, 1e-8, win, ws,
                                   wsb, cps, S)


def pv(**kw):
    return bmm(**dict(dict(fam=PV, Kx=100, Nout=64, ldx=100, ldw=128, ldwe=8, wbs=64, ldo=64), **kw))


@pytest.mark.parametrize("blk", BLOCKS)
def test_bmm_dec_gqa_arguments(blk):
    """every refusal returns before anything is launched"""
    for f in (bmm, pv):
        for kw in (dict(dt=3), dict(xm=0), dict(wm=8), dict(blk=48), dict(B=-2), dict(Tq=-1), dict(heads=0), dict(heads=3), dict(g=0), dict(g=-4),
                   dict(cps=-1), dict(fam=2)):
            assert f(**dict(dict(blk=blk), **kw)) == E_ARG, kw
        for kw in (dict(Tq=17), dict(g=1 << 31), dict(ldo=62), dict(cps=17), dict(ldx=1 << 29, g=8)):   # (R ldx = 2^32: past the pitch limit)
            assert f(blk=blk, **kw) == E_UNSUPPORTED, kw
        for kw in (dict(B=0), dict(Tq=0)):
            assert f(blk=blk, **kw) == 0, kw
        for name in ("x", "wc", "we", "out", "ln", "win"):
            assert f(blk=blk, **{name: Z}) == E_ARG, name
    assert bmm(blk=blk, B=1 << 28, heads=1, g=256, Tq=16) == E_UNSUPPORTED             # 2^36 (kv head, row tile) pairs
    # p v: the workspace of B * group heads, a workgroup per (kv head, tile of 16 rows) on a grid dimension of 65535
    need = L().bfpq_kv_dec_ws_bytes(4 * 4, 3, 64, 100, blk)
    assert pv(blk=blk, Tq=3, wsb=need - 1) == E_UNSUPPORTED and pv(blk=blk, Tq=3, wsb=need, ws=Z) == E_ARG
    assert pv(blk=blk, Tq=3, wsb=need, ws=ctypes.c_void_p(8)) == E_ARG
    assert pv(blk=blk, B=65535, heads=1, Tq=16, g=2) == E_UNSUPPORTED                  # two tiles per kv head
    assert pv(blk=blk, B=65535, heads=1, Tq=8, g=2, ws=Z) == E_ARG                     # one tile: taken (and refused for its null ws)
    assert pv(blk=blk, B=8192, heads=1, Tq=16, g=8, ws=Z) == E_UNSUPPORTED and pv(blk=blk, B=8191, heads=1, Tq=16, g=8, ws=Z) == E_ARG


# attend(q, k_codes, k_exps, v_codes, v_exps, out, p, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype, block,
#        xm, wm, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split, stream)
def attend(*, q=P, kc=P, ke=P, vc=P, ve=P, out=P, p=Z, ln=P, BH=4, heads=2, Tq=1, g=4, D=64, ml=100, cap=128, ldd=64, ldo=64, ldp=100,
           scale=0.125, causal=0, dt=2, blk=64, xm=7, wm=7, win=P, sws=P, swb=1 << 40, pws=P, pwb=1 << 40, cps=0):
    return L().bfpq_kv_attend_gqa(q, kc, ke, vc, ve, out, p, ln, BH, heads, Tq, g, D, ml, cap, ldd, ldo, ldp, scale, causal, dt, blk, xm, wm, 1e-8,
                                  win, sws, swb, pws, pwb, cps, S)


@pytest.mark.parametrize("blk", BLOCKS)
def test_attend_gqa_arguments(blk):
    for kw in (dict(dt=3), dict(xm=0), dict(wm=8), dict(blk=48), dict(BH=-2), dict(Tq=-1), dict(heads=0), dict(heads=3), dict(g=0), dict(g=-1),
               dict(cps=-1), dict(causal=2), dict(scale=float('nan')), dict(scale=float('inf')), dict(scale=1e300)):
        assert attend(**dict(dict(blk=blk), **kw)) == E_ARG, kw
    need_s, need_p = L().bfpq_kv_attend_ws_bytes(4 * 4, 3, 100), L().bfpq_kv_dec_ws_bytes(4 * 4, 3, 64, 100, blk)
    assert need_s > 0 and need_p > 0
    for kw in (dict(Tq=17), dict(g=1 << 31), dict(ml=0), dict(ml=129), dict(cap=100), dict(D=8), dict(ldd=32), dict(ldo=62), dict(p=P, ldp=99),
               dict(cps=17), dict(Tq=3, swb=need_s - 1), dict(Tq=3, pwb=need_p - 1), dict(BH=65536, heads=1, g=1), dict(BH=65535, heads=1, Tq=9, g=2),
               dict(BH=8192, heads=1, Tq=16, g=8)):
        assert attend(blk=blk, **kw) == E_UNSUPPORTED, kw
    for kw in (dict(BH=0), dict(Tq=0)):
        assert attend(blk=blk, **kw) == 0, kw
    for name in ("q", "kc", "ke", "vc", "ve", "out", "ln", "win", "sws", "pws"):
        assert attend(blk=blk, **{name: Z}) == E_ARG, name
        assert attend(blk=blk, Tq=3, swb=need_s, pwb=need_p, **{name: Z}) == E_ARG, name   # (the twin's workspaces are enough)
    for kw in (dict(BH=65535, heads=1, Tq=8, g=2), dict(BH=8191, heads=1, Tq=16, g=8)):
        assert attend(blk=blk, q=Z, **kw) == E_ARG, kw                                  # within the grid: taken up to the null q


def test_old_entries_are_the_group_1_case():
    """the same answers from the old entry and from the new one with group = 1, on refusals of every kind"""
    for kw in (dict(), dict(Tq=17), dict(heads=3), dict(ldo=62), dict(x=Z), dict(B=0)):
        a = dict(dict(x=P, B=4, heads=2, Tq=1, ldo=100), **kw)
        old = L().bfpq_kv_bmm_dec_dev(a['x'], P, P, Z, P, a['B'], a['heads'], a['Tq'], 64, 100, 64, 64, 4, 128, a['ldo'], QK, 2, 64, 7, 7, 1e-8, P, P,
                                      0, 0, S)
        assert old == bmm(g=1, out=Z, wsb=0, **kw), kw                                 # (out is null: nothing is launched)
    for kw in (dict(), dict(Tq=17), dict(heads=3), dict(BH=65536, heads=1), dict(ml=129), dict(BH=0)):
        a = dict(dict(BH=4, heads=2, Tq=1, ml=100), **kw)
        old = L().bfpq_kv_attend(Z, P, P, P, P, P, Z, P, a['BH'], a['heads'], a['Tq'], 64, a['ml'], 128, 64, 64, 100, 0.125, 0, 2, 64, 7, 7, 1e-8, P,
                                 P, 1 << 40, P, 1 << 40, 0, S)
        assert old == attend(g=1, q=Z, **kw), kw


@pytest.mark.parametrize("device_lengths", (False, True))
@pytest.mark.parametrize("heads,kv_heads", ((8, 8), (8, 2), (8, 1), (12, 4), (6, 6), (32, 8)))
def test_sizes_against_the_twin(heads, kv_heads, device_lengths):
    g = heads // kv_heads
    mode = dict(device_lengths=True, max_query_rows=3) if device_lengths else {}
    twin = bfp_ops.HBFPKVCache(2, heads, 64, 100, dtype=torch.bfloat16, **mode, **_args())
    c = bfp_ops.HBFPKVCache(2, heads, 64, 100, dtype=torch.bfloat16, kv_heads=kv_heads, **mode, **_args())
    assert (c.kv_heads, c.group, c.heads) == (kv_heads, g, heads)
    assert c.nbytes() * g == twin.nbytes()                                             # exactly the twin's divided by g
    for name, t in twin.buffers.items():
        assert c.buffers[name].shape == t.shape[:1] + (kv_heads,) + t.shape[2:], name
    if device_lengths:
        assert c.lengths.shape == (2,) and c.overflow.shape == (1,)
        assert c._ws.numel() == twin._ws.numel() == native.kv_dec_ws_bytes(2 * kv_heads * g, 3, 64, 128, 64)   # g * 3 rows per kv head
        c.prepare_attend(); twin.prepare_attend()
        assert c._att_ws.numel() == twin._att_ws.numel() == native.kv_attend_ws_bytes(2 * kv_heads * g, 3, 128)
    none = bfp_ops.HBFPKVCache(2, heads, 64, 100, dtype=torch.bfloat16, kv_heads=None, **mode, **_args())
    assert (none.kv_heads, none.group) == (heads, 1) and none.nbytes() == twin.nbytes() == 2 * heads * (128 * 64 * 2 + 128 + 2 * 64 + 64 * 64 * 2)


def test_kv_cache_passes_kv_heads_through():
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **{k: v for k, v in _args().items() if k != 'device'})
    c = mm.kv_cache(2, 8, 64, 100, dtype=torch.bfloat16, device='meta', kv_heads=2, device_lengths=True)
    assert (c.kv_heads, c.group) == (2, 4) and c.stats is mm.matmul_stats and c.k_codes.shape == (2, 2, 128, 64)


def test_python_refusals_allocate_and_launch_nothing():
    for bad in (3, 5, 0, -2, 16):
        with pytest.raises(ValueError, match="kv_heads"):
            bfp_ops.HBFPKVCache(2, 8, 64, 100, kv_heads=bad, **_args())
    for bad in (2.0, '2', True):
        with pytest.raises(TypeError, match="kv_heads"):
            bfp_ops.HBFPKVCache(2, 8, 64, 100, kv_heads=bad, **_args())
    dt = torch.bfloat16
    z = lambda *s: torch.zeros(s, dtype=dt, device='meta')
    for mode in (dict(), dict(device_lengths=True, max_query_rows=2)):
        c = bfp_ops.HBFPKVCache(2, 8, 64, 100, dtype=dt, kv_heads=2, **mode, **_args())
        with torch.no_grad():
            with pytest.raises(ValueError, match=r"append takes \[2, 2, t >= 1, 64\]"):
                c.append(z(2, 8, 1, 64), z(2, 8, 1, 64))                              # k_new with `heads` heads
            with pytest.raises(ValueError, match=r"scores takes \[2, 8, t >= 1, 64\]"):
                c.scores(z(2, 2, 1, 64))                                               # q with kv_heads heads
            if mode:
                with pytest.raises(ValueError, match=r"context takes \[2, 8, t >= 1, 100\]"):
                    c.context(z(2, 2, 1, 100))
                with pytest.raises(ValueError, match=r"attend takes \[2, 8, t >= 1, 64\]"):
                    c.attend(z(2, 2, 1, 64), 0.125)
                with pytest.raises(ValueError, match="query rows"):
                    c.scores(z(2, 8, 17, 64))                                          # the limits stay limits per query head
                with pytest.raises(ValueError, match="max_query_rows"):
                    c.attend(z(2, 8, 3, 64), 0.125)
                with pytest.raises(ValueError, match="max_query_rows"):
                    c.context(z(2, 8, 3, 100))
                assert c._att_ws is None
        with pytest.raises(ValueError, match="gradients"):
            c.scores(z(2, 8, 1, 64))
        assert c.stats.cache_calls == 0
    # a grid past the launch limit: 4096 x 8 kv heads with two row tiles each, where the tile is on the grid (the split p v kernel)
    big = bfp_ops.HBFPKVCache(4096, 32, 16, 64, dtype=dt, kv_heads=8, device_lengths=True, **_args(block_size=16))
    with torch.no_grad():
        with pytest.raises(ValueError, match="65535"):
            big.attend(z(4096, 32, 8, 16), 0.25)
        with pytest.raises(ValueError, match="65535"):
            big.context(z(4096, 32, 8, 64))
        with pytest.raises(native.NativeUnavailable):                                  # the qk kernel strides over the pairs: scores() is
            big.scores(z(4096, 32, 8, 16))                                             # taken, up to the operand that is on no GPU
    assert bmm(blk=16, B=4096 * 8, heads=8, g=4, Tq=8, Kx=16, ldx=16, x=Z) == E_ARG    # and by the entry, up to the null x
    # a cache without groups keeps its refusals where they were: none here, the entry's own after the operand checks
    wide = bfp_ops.HBFPKVCache(2048, 33, 16, 64, dtype=dt, device_lengths=True, **_args(block_size=16))
    with torch.no_grad():
        for call in (lambda: wide.scores(z(2048, 33, 1, 16)), lambda: wide.context(z(2048, 33, 1, 64)),
                     lambda: wide.attend(z(2048, 33, 1, 16), 0.25)):
            with pytest.raises(native.NativeUnavailable):
                call()


def test_native_wrappers_take_a_group(monkeypatch):
    zt = lambda *s, dt=torch.int8: torch.zeros(s, dtype=dt)
    bufs = lambda: [zt(4, 128, 64), zt(4, 128, 1), zt(4, 64, 128), zt(4, 64, 2)]
    u8 = lambda n: zt(n, dt=torch.uint8)
    q = zt(4, 6, 64, dt=torch.bfloat16)
    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **kw: None)
    for bad in (4, 0, -1, 2.0, True):                                                  # 6 rows per kv head are no 4 query heads
        with pytest.raises(ValueError, match="group"):
            native.kv_attend(q, *bufs(), zt(2, dt=torch.int32), 2, 100, 0.125, False, 64, 7, 1e-8, u8(1 << 20), u8(1 << 20), group=bad)
        with pytest.raises(ValueError, match="group"):
            native.kv_bmm_dec_dev(q, bufs()[0], bufs()[1], QK, 100, 128, zt(2, dt=torch.int32), 2, 64, 7, 1e-8, group=bad)
    small = native.kv_dec_ws_bytes(4 * 3, 2, 64, 100, 64) - 1                          # the workspaces are those of BH * group heads
    with pytest.raises(ValueError, match="sum_ws"):
        native.kv_attend(q, *bufs(), zt(2, dt=torch.int32), 2, 100, 0.125, False, 64, 7, 1e-8, u8(1 << 20), u8(small), group=3)
    with pytest.raises(ValueError, match="score_ws"):
        native.kv_attend(q, *bufs(), zt(2, dt=torch.int32), 2, 100, 0.125, False, 64, 7, 1e-8, u8(native.kv_attend_ws_bytes(12, 2, 100) - 1),
                         u8(1 << 20), group=3)
