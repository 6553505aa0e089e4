"""Host-side checks of HBFPKVCache.attend: the two C entries (exported, declared with the signatures native.py binds, the
workspace size without a device, every refusal before a launch) and the Python refusals, which allocate nothing.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_kv_attend_ws_bytes", "bfpq_kv_attend")
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
    return dict(bfp_ops.unpack_bfp_args(base), device='cpu')


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
        assert restype is (ctypes.c_int64 if m.group(1) == 'int64_t' else ctypes.c_int), name
        assert [_ctype(a) for a in m.group(2).split(',')] == list(argtypes), name
    assert "modeling_gpt2.py:207-243" in open(HEADER).read()                       # the reference lines the entry replaces


def test_workspace_bytes_without_a_device():
    ws = L().bfpq_kv_attend_ws_bytes
    assert ws(12, 1, 4096) == 12 * 4096 * 4                                        # fp32 score rows [BH, Tq, max_len]
    assert ws(12, 16, 4096) == 16 * ws(12, 1, 4096)
    assert ws(1, 1, 1) == 16 and ws(1, 1, 5) == 32 and ws(3, 1, 6) == 96           # the pitch rounded up to 4 elements, the whole to 16 bytes
    assert ws(0, 1, 64) == 0 and ws(1, 0, 64) == 0
    assert native.kv_attend_ws_bytes(6, 3, 250) == ws(6, 3, 250) == 6 * 3 * 252 * 4
    for bad in ((-1, 1, 64), (1, -1, 64), (1, 1, -1)):
        assert ws(*bad) == E_ARG, bad
    for bad in ((1, 17, 64), (1, 1, 1 << 31), (1 << 31, 1, 64)):
        assert ws(*bad) == E_UNSUPPORTED, bad
    with pytest.raises(RuntimeError):
        native.kv_attend_ws_bytes(1, 17, 64)


# attend(q, k_codes, k_exps, v_codes, v_exps, out, p, lens, BH, heads, Tq, D, max_len, cap, ldd, ldo, ldp, scale, causal, dtype, block, xm, wm,
#        epsilon, exp_win, score_ws, score_ws_bytes, sum_ws, sum_ws_bytes, chunks_per_split, stream)
def attend(*, q=P, kc=P, ke=P, vc=P, ve=P, out=P, p=Z, ln=P, BH=4, heads=2, Tq=1, D=64, ml=100, cap=128, ldd=64, ldo=64, ldp=100, scale=0.125,
           causal=0, dt=2, blk=64, xm=7, wm=7, win=P, sws=P, swb=1 << 30, pws=P, pwb=1 << 30, cps=0):
    return L().bfpq_kv_attend(q, kc, ke, vc, ve, out, p, ln, BH, heads, Tq, D, ml, cap, ldd, ldo, ldp, scale, causal, dt, blk, xm, wm, 1e-8, win,
                              sws, swb, pws, pwb, cps, S)


@pytest.mark.parametrize("blk", BLOCKS)
def test_attend_arguments(blk):
    """every refusal returns before anything is launched (the pointers are not memory)"""
    for kw in (dict(dt=3), dict(dt=-1), dict(xm=0), dict(wm=8), dict(blk=48), dict(BH=-2), dict(Tq=-1), dict(heads=0), dict(heads=3), dict(cps=-1),
               dict(causal=2), dict(causal=-1), dict(scale=float('nan')), dict(scale=float('inf')), dict(scale=-float('inf')), dict(scale=1e300)):
        assert attend(**dict(dict(blk=blk), **kw)) == E_ARG, kw
    need_s, need_p = L().bfpq_kv_attend_ws_bytes(4, 1, 100), L().bfpq_kv_dec_ws_bytes(4, 1, 64, 100, blk)
    for kw in (dict(Tq=17), dict(ml=0), dict(ml=129), dict(cap=100), dict(D=8), dict(D=blk + 8), dict(D=2048, ldd=2048, ldo=2048), dict(ldd=32),
               dict(ldd=96), dict(ldo=62), dict(ldo=60), dict(p=P, ldp=99), dict(BH=65536, heads=1), dict(cps=17), dict(swb=need_s - 1),
               dict(pwb=need_p - 1), dict(swb=0)):
        assert attend(blk=blk, **kw) == E_UNSUPPORTED, kw
    for kw in (dict(BH=0), dict(Tq=0)):
        assert attend(blk=blk, **kw) == 0, kw
    for name in ("q", "kc", "ke", "vc", "ve", "out", "ln", "win", "sws", "pws"):
        assert attend(blk=blk, **{name: Z}) == E_ARG, name                         # (p may be null: no probabilities returned)
    for name in ("kc", "vc", "out", "sws", "pws"):
        assert attend(blk=blk, **{name: ctypes.c_void_p(8)}) == E_ARG, name
    assert attend(blk=blk, ln=ctypes.c_void_p(18)) == E_ARG and attend(blk=blk, q=ctypes.c_void_p(17)) == E_ARG
    assert attend(blk=blk, p=ctypes.c_void_p(17)) == E_ARG


def test_python_refusals_allocate_nothing():
    c = bfp_ops.HBFPKVCache(2, 3, 64, 100, dtype=torch.bfloat16, device_lengths=True, max_query_rows=2, **_args())
    h = bfp_ops.HBFPKVCache(2, 3, 64, 100, dtype=torch.bfloat16, **_args())
    assert c._att_ws is None and c.nbytes() == h.nbytes()                          # construction and nbytes() are as before
    q = torch.zeros(2, 3, 2, 64, dtype=torch.bfloat16)
    with torch.no_grad():
        with pytest.raises(ValueError, match="attend needs device_lengths=True"):
            h.attend(q, 0.125)
        with pytest.raises(ValueError, match="attend needs device_lengths=True"):
            h.prepare_attend()
        with pytest.raises(ValueError, match="max_query_rows"):
            c.attend(torch.zeros(2, 3, 3, 64, dtype=torch.bfloat16), 0.125)
        with pytest.raises(ValueError, match="query rows"):
            c.attend(torch.zeros(2, 3, 17, 64, dtype=torch.bfloat16), 0.125)
        for bad in (float('nan'), float('inf'), None, '0.125', True, 1j):
            with pytest.raises(ValueError, match="scale"):
                c.attend(q, bad)
        for bad in (0, 101, -1, 64.0, True):
            with pytest.raises(ValueError, match="max_len"):
                c.attend(q, 0.125, max_len=bad)
        for bad in (q.float(), q[:, :2], q[..., :32], q[0]):
            with pytest.raises(ValueError):
                c.attend(bad, 0.125)
    with pytest.raises(ValueError, match="gradients"):
        c.attend(q, 0.125)
    assert c._att_ws is None and c.stats.cache_calls == 0
    c.prepare_attend()                                                             # the explicit preparation: once, sized by the capacity
    ws = c._att_ws
    assert ws.numel() == native.kv_attend_ws_bytes(6, 2, 128) and ws.dtype == torch.uint8
    c.prepare_attend()
    assert c._att_ws is ws and c.nbytes() == h.nbytes()


def test_native_wrapper_checks_every_tensor(monkeypatch):
    z = lambda *s, dt=torch.int8: torch.zeros(s, dtype=dt)
    bufs = lambda: [z(4, 128, 64), z(4, 128, 1), z(4, 64, 128), z(4, 64, 2)]
    i32 = lambda n: z(n, dt=torch.int32)
    q = z(4, 1, 64, dt=torch.bfloat16)
    u8 = lambda n: z(n, dt=torch.uint8)
    big = 1 << 20
    with pytest.raises(native.NativeUnavailable):
        native.kv_attend(q, *bufs(), i32(2), 2, 100, 0.125, False, 64, 7, 1e-8, u8(big), u8(big))
    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **kw: None)
    for kw in (dict(ln=i32(3)), dict(ln=i32(2).long()), dict(heads=3), dict(heads=0), dict(i=0, b=z(4, 100, 64)), dict(i=1, b=z(4, 128, 2)),
               dict(i=2, b=z(4, 64, 128, dt=torch.uint8)), dict(i=3, b=z(4, 64, 1)), dict(scale=float('inf')), dict(sws=u8(10)), dict(pws=u8(10)),
               dict(sws=None), dict(pws=z(big))):
        b = bufs()
        if 'i' in kw:
            b[kw['i']] = kw['b']
        with pytest.raises(ValueError):
            native.kv_attend(q, *b, kw.get('ln', i32(2)), kw.get('heads', 2), 100, kw.get('scale', 0.125), False, 64, 7, 1e-8,
                             kw.get('sws', u8(big)), kw.get('pws', u8(big)))
    with pytest.raises(ValueError):
        native.kv_attend(q[0], *bufs(), i32(2), 2, 100, 0.125, False, 64, 7, 1e-8, u8(big), u8(big))
