"""Host-side checks of prompt attention on the HBFP KV cache (HBFPKVCache(prompt_rows=P)): the new C entry and its size
function (exported, declared with the signatures native.py binds, bfpq_kv_attend_gqa's arguments and two more, every refusal before a
launch), the workspace bytes, and the Python refusals; prompt_rows=0 is today's cache.  No GPU needed: the pointers are not memory."""
import ctypes
import os
import re

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_kv_attend_rows", "bfpq_kv_attend_rows_ws_bytes")
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
    for name, rtype in zip(NEW, ('int', 'int64_t')):
        assert hasattr(L(), name), name
        m = re.search(rf"\b(int64_t|int)\s+{name}\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/bfpq.h"
        restype, argtypes = native.PROTOTYPES[name]
        assert m.group(1) == rtype and restype is (ctypes.c_int if rtype == 'int' else ctypes.c_int64), name
        assert [_ctype(a) for a in m.group(2).split(',')] == list(argtypes), name
    rows, gqa = native.PROTOTYPES["bfpq_kv_attend_rows"][1], native.PROTOTYPES["bfpq_kv_attend_gqa"][1]
    assert list(rows) == list(gqa[:-1]) + [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]      # row0 and rows in front of the stream
    comment = text[:text.index("int64_t bfpq_kv_attend_rows_ws_bytes")].rsplit("/*", 1)[1]
    assert "modeling_gpt2.py:207-243" in comment and "modeling_llama.py:397-409" in comment      # the reference lines the entry replaces


def test_workspace_bytes():
    f = L().bfpq_kv_attend_rows_ws_bytes
    for BH, Pr, ml in ((8, 16, 320), (32, 512, 4096), (3, 48, 257), (1, 16, 1)):
        want = (4 * BH * Pr * ((ml + 3) // 4 * 4) + 15) // 16 * 16
        assert f(BH, Pr, ml) == want == native.kv_attend_rows_ws_bytes(BH, Pr, ml)
    assert f(8, 16, 320) == L().bfpq_kv_attend_ws_bytes(8, 16, 320)                   # a panel of 16 rows is attend()'s score rows
    assert f(0, 16, 320) == 0 and f(-1, 16, 320) == E_ARG and f(8, -16, 320) == E_ARG and f(8, 16, -1) == E_ARG
    assert f(32, 4096, 4096) == E_UNSUPPORTED and f(32, 4080, 4096) > 0               # 2^31 bytes and just below
    assert f(1 << 31, 16, 320) == E_UNSUPPORTED and f(8, 1 << 31, 320) == E_UNSUPPORTED and f(8, 16, 1 << 31) == E_UNSUPPORTED
    with pytest.raises(Exception):
        native.kv_attend_rows_ws_bytes(32, 4096, 4096)
    # the bound the class states: the largest multiple of 16 whose workspace stays below 2^31 bytes
    for B, H, cap in ((1, 32, 4096), (8, 12, 1024), (2, 4, 320), (64, 64, 8192)):
        pm = bfp_ops.HBFPKVCache.prompt_rows_max(B, H, cap)
        assert pm % 16 == 0
        assert pm == 0 or 0 < f(B * H, pm, native.code_pitch(cap)) < 1 << 31
        assert f(B * H, pm + 16, native.code_pitch(cap)) == E_UNSUPPORTED


# rows(q, k_codes, k_exps, v_codes, v_exps, out, p, lens, BH, heads, Tq, group, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype, block,
#      xm, wm, epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split, row0, rows, stream)
def rows(*, q=P, kc=P, ke=P, vc=P, ve=P, out=P, p=Z, ln=P, BH=4, heads=2, Tq=100, g=4, D=64, ml=100, cap=128, ldd=64, ldo=64, ldp=100,
         scale=0.125, causal=0, dt=2, blk=64, xm=7, wm=7, win=P, sws=P, swb=1 << 40, pws=Z, pwb=0, cps=0, row0=32, n=48):
    return L().bfpq_kv_attend_rows(q, kc, ke, vc, ve, out, p, ln, BH, heads, Tq, g, D, ml, cap, ldd, ldo, ldp, scale, causal, dt, blk, xm, wm, 1e-8,
                                   win, sws, swb, pws, pwb, cps, row0, n, S)


@pytest.mark.parametrize("blk", BLOCKS)
def test_attend_rows_arguments(blk):
    """every refusal returns before anything is launched: bfpq_kv_attend_gqa's conventions, and the panel's"""
    for kw in (dict(dt=3), dict(xm=0), dict(wm=8), dict(blk=48), dict(BH=-2), dict(Tq=-1), dict(heads=0), dict(heads=3), dict(g=0), dict(g=-1),
               dict(cps=-1), dict(causal=2), dict(scale=float('nan')), dict(scale=float('inf')), dict(scale=1e300), dict(row0=-1), dict(n=-1),
               dict(row0=101, n=0), dict(row0=60, n=41), dict(row0=0, n=101)):
        assert rows(**dict(dict(blk=blk), **kw)) == E_ARG, kw
    need = L().bfpq_kv_attend_rows_ws_bytes(4 * 4, 48, 100)
    assert need == 4 * 16 * 48 * 100
    for kw in (dict(g=1 << 31), dict(ml=0), dict(ml=129), dict(cap=100), dict(D=8), dict(D=320, ldd=320, ldo=320), dict(ldd=32), dict(ldo=62),
               dict(p=P, ldp=99), dict(cps=17), dict(swb=need - 1), dict(Tq=1 << 31, row0=0, n=16)):
        assert rows(blk=blk, **kw) == E_UNSUPPORTED, kw
    for kw in (dict(BH=0), dict(Tq=0, row0=0, n=0), dict(n=0), dict(row0=100, n=0)):
        assert rows(blk=blk, **kw) == 0, kw
    for name in ("q", "kc", "ke", "vc", "ve", "out", "ln", "win", "sws"):
        assert rows(blk=blk, **{name: Z}) == E_ARG, name
        assert rows(blk=blk, swb=need, **{name: Z}) == E_ARG, name                     # (the panel's bytes are enough: taken up to the null)
    assert rows(blk=blk, q=ctypes.c_void_p(8)) == E_ARG and rows(blk=blk, sws=ctypes.c_void_p(8)) == E_ARG
    assert rows(blk=blk, p=ctypes.c_void_p(17)) == E_ARG
    # any Tq, a whole prompt in one panel, D up to 256: taken up to the null q
    for kw in (dict(Tq=17, row0=0, n=17), dict(Tq=1 << 20, row0=(1 << 20) - 16, n=16), dict(D=256, ldd=256, ldo=256), dict(pws=P, pwb=16, cps=16)):
        assert rows(blk=blk, q=Z, **kw) == E_ARG, kw


def test_python_refusals_come_before_any_launch():
    a = _args()
    mk = lambda **kw: bfp_ops.HBFPKVCache(2, 4, 64, 320, dtype=torch.bfloat16, **dict(a, **kw))
    for bad in (8, 24, 17, -16):
        with pytest.raises(ValueError, match="multiple of 16"):
            mk(device_lengths=True, prompt_rows=bad)
    for bad in (True, False, 16.0, "32", None):
        with pytest.raises(TypeError, match="prompt_rows"):
            mk(device_lengths=True, prompt_rows=bad)
    with pytest.raises(ValueError, match="device_lengths"):
        mk(prompt_rows=32)
    with pytest.raises(ValueError, match="2\\^31"):
        bfp_ops.HBFPKVCache(1, 32, 128, 4096, dtype=torch.bfloat16, device_lengths=True, prompt_rows=4096, **a)
    with pytest.raises(ValueError, match="head_dim"):
        bfp_ops.HBFPKVCache(1, 2, 512, 320, dtype=torch.bfloat16, device_lengths=True, prompt_rows=32, **a)
    assert bfp_ops.HBFPKVCache.prompt_rows_max(1, 32, 4096) == 4080
    cache = mk(device_lengths=True, prompt_rows=0)
    q = torch.zeros(2, 4, 17, 64, dtype=torch.bfloat16, device='meta')
    with torch.no_grad():
        with pytest.raises(ValueError, match="up to 16 query rows"):
            cache.attend(q, 0.125)                                                     # Tq > 16 with prompt_rows=0: as today
        long = mk(device_lengths=True, prompt_rows=32)
        for f in (long.scores, lambda x: long.context(torch.zeros(2, 4, 17, 320, dtype=torch.bfloat16, device='meta'))):
            with pytest.raises(ValueError, match="up to 16 query rows"):
                f(q)                                                                   # scores() and context() keep their limit
        with pytest.raises(ValueError, match="scale"):
            long.attend(q, float('nan'))
        with pytest.raises(ValueError, match="max_len"):
            long.attend(q, 0.125, max_len=321)
    with pytest.raises(ValueError, match="inference only"):
        long.attend(q, 0.125)


@pytest.mark.parametrize("kv_heads", (None, 2))
def test_prompt_rows_0_is_todays_cache(kv_heads):
    a = _args()
    mk = lambda **kw: bfp_ops.HBFPKVCache(2, 4, 64, 320, dtype=torch.bfloat16, device_lengths=True, kv_heads=kv_heads, **dict(a, **kw))
    plain, zero, long = mk(), mk(prompt_rows=0), mk(prompt_rows=96)
    assert plain.prompt_rows == zero.prompt_rows == 0 and long.prompt_rows == 96
    assert plain.nbytes() == zero.nbytes() == long.nbytes()                            # the panel workspace is no buffer of the cache
    for c in (plain, zero, long):
        assert c._att_ws is None and c._rows_ws is None                                # nothing is made before prepare_attend()
    assert set(vars(plain)) == set(vars(zero))
    for name, value in vars(plain).items():
        other = vars(zero)[name]
        if isinstance(value, torch.Tensor):
            assert (value.shape, value.dtype, value.device) == (other.shape, other.dtype, other.device), name
        elif name not in ('buffers', 'stats', 'act'):
            assert value == other, name
    assert {k: (t.shape, t.dtype) for k, t in plain.buffers.items()} == {k: (t.shape, t.dtype) for k, t in zero.buffers.items()}
    zero.prepare_attend()
    long.prepare_attend()
    assert zero._rows_ws is None and zero._att_ws.numel() == long._att_ws.numel() == 2 * 4 * 16 * 320 * 4
    assert long._rows_ws.numel() == native.kv_attend_rows_ws_bytes(2 * 4, 96, 320) == 2 * 4 * 96 * 320 * 4
    op = bfp_ops.F_matmul_bfp(matrix_unit='int8', **{k: v for k, v in a.items() if k != 'device'}, device='meta')
    via = op.kv_cache(2, 4, 64, 320, device='meta', device_lengths=True, prompt_rows=32)
    assert via.prompt_rows == 32 and via.stats is op.matmul_stats
