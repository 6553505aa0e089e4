"""Host-side checks of the HBFP KV cache (csrc/bfpq_kvcache.hip, bfp_ops.HBFPKVCache): kv_cache_config_check, the new C entries (exported,
declared, every refusal before a launch) and the dense batched entry as a call of the strided one.  No GPU needed."""
import ctypes
import os

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_kv_ok", "bfpq_kv_append", "bfpq_kv_bmm_dec", "bfpq_hbfp_bmm_i8_strided")
P = ctypes.c_void_p(16)
Z = None
S = ctypes.c_void_p(0)
BLOCKS = (16, 32, 64)


def L():
    return native.load_library()


def _args(**kw):
    base = dict(num_format='bfp', sparsity_num_format='bfp', rounding_mode='determ', block_size=64, mant_bits=7, epsilon=1e-8)
    base.update(kw)
    return bfp_ops.unpack_bfp_args(base)


# ---- the configuration check --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", BLOCKS)
def test_config_check_accepts(blk):
    for m in range(1, 8):
        for D in (64, 128, 192):
            assert bfp_ops.kv_cache_config_check(_args(block_size=blk, mant_bits=m), D) is None
    if blk < 64:
        bfp_ops.kv_cache_config_check(_args(block_size=blk), 32 if blk == 32 else 48)
    # pruning of q / p (in_sparsity) is the product's business, not the cache's
    bfp_ops.kv_cache_config_check(_args(block_size=blk, in_sparsity=True, sparsity_mode='structured', N=2, M=4), 64)
    bfp_ops.kv_cache_config_check(_args(block_size=blk, in_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5), 64)
    bfp_ops.kv_cache_config_check(_args(block_size=blk, grad_sparsity=True), 64)


@pytest.mark.parametrize("kw,D,reason", [
    (dict(w_sparsity=True, sparsity_mode='structured', N=2, M=4), 64, "pruned K / V"),
    (dict(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5), 64, "pruned K / V"),
    (dict(rounding_mode='stoc'), 64, "stochastic rounding"),
    (dict(num_format='fp32'), 64, "num_format"),
    (dict(sparsity_num_format='fp32'), 64, "sparsity_num_format"),
    (dict(block_size=8), 64, "block_size"),
    (dict(block_size=128), 128, "block_size"),
    (dict(mant_bits=0), 64, "mant_bits"),
    (dict(mant_bits=8), 64, "mant_bits"),
    (dict(), 96, "head_dim"),                                   # D % block
    (dict(block_size=16), 40, "head_dim"),
    (dict(block_size=16), 8, "head_dim"),
    (dict(in_sparsity=True, sparsity_mode='structured', N=5, M=4), 64, "in_sparsity"),
])
def test_config_check_refuses(kw, D, reason):
    with pytest.raises(ValueError, match=reason):
        bfp_ops.kv_cache_config_check(_args(**kw), D)
    with pytest.raises(ValueError, match=reason):                # ... at construction, before any buffer is made
        bfp_ops.HBFPKVCache(1, 1, D, 64, dtype=torch.float32, **dict(_args(**kw), device='cpu'))


def test_the_op_offers_the_cache_and_counts_it():
    mm = bfp_ops.F_matmul_bfp(matrix_unit='int8', **_args())
    assert mm.matmul_stats.cache_calls == 0 and callable(mm.kv_cache)
    assert not hasattr(bfp_ops.F_matmul_bfp(**_args()), 'kv_cache')
    with pytest.raises(ValueError, match="pruned K / V"):
        bfp_ops.F_matmul_bfp(matrix_unit='int8', **_args(w_sparsity=True, sparsity_mode='structured', N=2, M=4)).kv_cache(1, 2, 64, 128)
    with pytest.raises(TypeError):
        bfp_ops.HBFPKVCache(1, 1, 64, 64, dtype=torch.float64, **dict(_args(), device='cpu'))
    with pytest.raises(TypeError):
        bfp_ops.HBFPKVCache(1, 1, 64, 64, dtype=torch.float32, no_such_argument=1, **dict(_args(), device='cpu'))


def test_buffers_and_host_refusals_on_cpu_buffers():
    """shape, dtype, capacity and gradient refusals come before any launch: they show on a cache whose buffers live on the CPU"""
    c = bfp_ops.HBFPKVCache(2, 3, 64, 100, dtype=torch.bfloat16, **dict(_args(block_size=16, mant_bits=3), device='cpu'))
    assert c.cap == 128 and c.capacity == 100 and c.length == 0
    assert c.k_codes.shape == (2, 3, 128, 64) and c.k_exps.shape == (2, 3, 128, 4) and c.v_codes.shape == (2, 3, 64, 128)
    assert c.v_exps.shape == (2, 3, 64, 8) and c.v_tail.shape == (2, 3, 16, 64) and c.v_tail.dtype == torch.bfloat16
    assert not bool(c.v_codes.any())
    assert c.nbytes() == 6 * (128 * 64 + 128 * 4 + 64 * 128 + 64 * 8 + 2 * 16 * 64)
    big = bfp_ops.HBFPKVCache(1, 2, 64, 4096, dtype=torch.bfloat16, **dict(_args(), device='cpu'))
    assert 0.5 < big.nbytes() / (2 * 2 * 4096 * 64 * 2) < 0.52                   # codes + exponents + the open block against bf16 K and V
    k = torch.zeros(2, 3, 4, 64, dtype=torch.bfloat16)
    with torch.no_grad():
        for bad in (k.float(), k[:, :2], k[..., :32], k[0]):
            with pytest.raises(ValueError):
                c.append(bad, bad)
        with pytest.raises(ValueError, match="capacity"):
            c.append(k.expand(2, 3, 4, 64).repeat(1, 1, 26, 1), k.repeat(1, 1, 26, 1))      # 104 > 100
        with pytest.raises(ValueError, match="empty"):
            c.scores(k)
        with pytest.raises(ValueError):
            c.context(torch.zeros(2, 3, 1, 5, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="gradients"):
        c.append(k, k)
    assert c.length == 0 and c.stats.cache_calls == 0


# ---- the C entries ------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    assert set(NEW) <= set(native.EXPORTED_SYMBOLS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bfpq.h")).read()
    for name in NEW:
        assert hasattr(L(), name), name
        assert f"int {name}(" in header, name
    assert native.KV_DEC_MAX_TOKENS == 16 and "#define BFPQ_KV_DEC_MAX_TOKENS 16" in header


def test_kv_ok():
    ok = L().bfpq_kv_ok
    for blk in BLOCKS:
        assert ok(64, 64, blk) == 1 and ok(128, 4096, blk) == 1 and ok(1024, 64, blk) == 1
        assert ok(64, 100, blk) == 0 and ok(64, 0, blk) == 0 and ok(8, 64, blk) == 0 and ok(0, 64, blk) == 0 and ok(2048, 64, blk) == 0
        assert ok(1024, 1 << 21, blk) == 0
    assert ok(96, 64, 64) == 0 and ok(96, 64, 32) == 1 and ok(48, 64, 32) == 0 and ok(48, 64, 16) == 1
    for blk in (8, 48, 128, 0, -16):
        assert ok(64, 64, blk) == 0 and not native.kv_ok(64, 64, blk)


# append(k_new, v_new, k_codes, k_exps, v_codes, v_exps, v_tail, BH, D, pos, t, cap, ldd, dtype, block, mant_bits, epsilon, exp_win, stream)
def append(*, kn=P, vn=P, kc=P, ke=P, vc=P, ve=P, vt=P, BH=2, D=64, pos=0, t=1, cap=128, ldd=64, dt=2, blk=64, m=7, win=P):
    return L().bfpq_kv_append(kn, vn, kc, ke, vc, ve, vt, BH, D, pos, t, cap, ldd, dt, blk, m, 1e-8, win, S)


@pytest.mark.parametrize("blk", BLOCKS)
def test_append_arguments(blk):
    for kw in (dict(dt=3), dict(dt=-1), dict(m=0), dict(m=8), dict(BH=-1), dict(t=-1), dict(pos=-1), dict(blk=8), dict(blk=128)):
        assert append(**dict(dict(blk=blk), **kw)) == E_ARG, kw
    for kw in (dict(cap=100), dict(cap=0), dict(D=8), dict(D=blk + 8), dict(ldd=32), dict(ldd=96), dict(D=128, ldd=64), dict(pos=128),
               dict(pos=100, t=29), dict(D=2048, ldd=2048)):
        assert append(blk=blk, **kw) == E_UNSUPPORTED, kw
    for kw in (dict(BH=0), dict(t=0)):
        assert append(blk=blk, **kw) == 0, kw
    for name in ("kn", "vn", "kc", "ke", "vc", "ve", "vt", "win"):
        assert append(blk=blk, **{name: Z}) == E_ARG, name
    for name in ("kn", "vn", "kc", "vc", "vt"):
        assert append(blk=blk, **{name: ctypes.c_void_p(8)}) == E_ARG, name


# dec(x, wcodes, wexp, out, B, Tq, Kx, Nout, ldx, ldw, ldwe, w_bstride, ldo, family, dtype, block, xm, wm, epsilon, exp_win, stream)
def dec(*, x=P, wc=P, we=P, out=P, B=2, Tq=1, Kx=64, Nout=100, ldx=64, ldw=64, ldwe=4, wbs=128, ldo=100, fam=0, dt=2, blk=64, xm=7, wm=7, win=P):
    return L().bfpq_kv_bmm_dec(x, wc, we, out, B, Tq, Kx, Nout, ldx, ldw, ldwe, wbs, ldo, fam, dt, blk, xm, wm, 1e-8, win, S)


PV = dict(fam=1, Kx=100, Nout=64, ldx=100, ldw=128, ldwe=8, wbs=64, ldo=64)


@pytest.mark.parametrize("blk", BLOCKS)
def test_decode_product_arguments(blk):
    for kw in (dict(dt=3), dict(xm=0), dict(wm=8), dict(fam=2), dict(fam=-1), dict(B=-1), dict(Tq=-1), dict(Nout=-1), dict(Kx=-1), dict(blk=48)):
        assert dec(**dict(dict(blk=blk), **kw)) == E_ARG, kw
    for kw in (dict(Tq=17), dict(Kx=0), dict(Kx=blk + 8, ldx=128, ldw=128), dict(ldx=32), dict(ldw=96), dict(Kx=128, ldx=128), dict(ldwe=0),
               dict(wbs=99), dict(ldo=102), dict(ldo=96), dict(wbs=1 << 26), dict(Tq=16, ldx=1 << 28)):
        assert dec(blk=blk, **kw) == E_UNSUPPORTED, kw
    for kw in (dict(Nout=72), dict(ldw=64), dict(ldwe=100 // blk), dict(ldx=99), dict(wbs=63), dict(ldo=62)):
        assert dec(blk=blk, **dict(PV, **kw)) == E_UNSUPPORTED, kw
    for kw in (dict(B=0), dict(Tq=0), dict(Nout=0, ldo=0)):
        assert dec(blk=blk, **kw) == 0, kw
    for name in ("x", "wc", "we", "out", "win"):
        assert dec(blk=blk, **{name: Z}) == E_ARG, name
        assert dec(blk=blk, **dict(PV, **{name: Z})) == E_ARG, name
    for name in ("wc", "out"):
        assert dec(blk=blk, **{name: ctypes.c_void_p(8)}) == E_ARG, name
    assert dec(blk=blk, x=ctypes.c_void_p(17)) == E_ARG                           # x: aligned to its element, rows may start anywhere


# strided(xc, xe, wc, we, out, B, T, N, K, ldk, w_ld, w_exp_ld, w_bstride, w_rows, block, dtype, wm, xm, stream)
def strided(*, xc=P, xe=P, wc=P, we=P, out=P, B=2, T=40, N=80, K=64, ldk=64, wld=64, weld=4, wbs=128, rows=70, blk=64, dt=2, wm=7, xm=7):
    return L().bfpq_hbfp_bmm_i8_strided(xc, xe, wc, we, out, B, T, N, K, ldk, wld, weld, wbs, rows, blk, dt, wm, xm, S)


@pytest.mark.parametrize("blk", BLOCKS)
def test_strided_arguments(blk):
    for kw in (dict(dt=3), dict(wm=0), dict(xm=8), dict(B=-1), dict(T=-1), dict(N=-16), dict(blk=48)):
        assert strided(**dict(dict(blk=blk), **kw)) == E_ARG, kw
    for kw in (dict(N=72), dict(K=blk // 2), dict(ldk=96), dict(wld=96), dict(wld=0), dict(K=128, ldk=128), dict(weld=64 // blk - 1),
               dict(rows=0), dict(rows=81), dict(wbs=69), dict(wbs=1 << 26)):
        assert strided(blk=blk, **kw) == E_UNSUPPORTED, kw
    for kw in (dict(B=0), dict(T=0), dict(N=0)):
        assert strided(blk=blk, **kw) == 0, kw
    for name in ("xc", "xe", "wc", "we", "out"):
        assert strided(blk=blk, **{name: Z}) == E_ARG, name
    for name in ("xc", "wc", "out"):
        assert strided(blk=blk, **{name: ctypes.c_void_p(8)}) == E_ARG, name


def test_wrapper_shapes_are_checked(monkeypatch):
    monkeypatch.setattr(native, 'require_device_tensor_any', lambda *a, **k: None)
    z = lambda *s: torch.zeros(s, dtype=torch.int8)
    with pytest.raises(ValueError, match="exponents"):
        native.hbfp_bmm_i8_strided((z(32, 64), z(32, 4)), z(2, 128, 64), z(2, 128, 1), 2, 16, 16, 64, 128, 16, 7, 7)
    with pytest.raises(ValueError, match="rows"):
        native.hbfp_bmm_i8_strided((z(32, 64), z(32, 1)), z(2, 100, 64), z(2, 100, 1), 2, 16, 16, 64, 128, 16, 7, 7)
    with pytest.raises(ValueError, match="contiguous"):
        native.hbfp_bmm_i8_strided((z(32, 64), z(32, 1)), z(2, 128, 128)[..., :64], z(2, 128, 1), 2, 16, 16, 64, 128, 16, 7, 7)


def test_native_wrappers_check_every_tensor(monkeypatch):
    """kv_append / kv_bmm_dec take nothing on trust: a CPU tensor raises, and so do a strided v_new, a buffer of the wrong size or dtype"""
    z = lambda *s, dt=torch.int8: torch.zeros(s, dtype=dt)
    bufs = lambda: [z(2, 128, 64), z(2, 128, 1), z(2, 64, 128), z(2, 64, 2), z(2, 64, 64, dt=torch.bfloat16)]
    k = z(2, 3, 64, dt=torch.bfloat16)
    with pytest.raises(native.NativeUnavailable):
        native.kv_append(k, k, *bufs(), 0, 64, 7, 1e-8)
    with pytest.raises(native.NativeUnavailable):
        native.kv_bmm_dec(k, z(2, 128, 64), z(2, 128, 1), native.KV_QK, 100, 128, 64, 7, 1e-8)
    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **kw: None)
    for bad in (dict(v=z(2, 3, 128, dt=torch.bfloat16)[..., ::2]), dict(v=k.float()), dict(v=k[:, :2]), dict(i=0, b=z(2, 100, 64)),
                dict(i=1, b=z(2, 128, 1, dt=torch.uint8)), dict(i=2, b=z(2, 128, 64).transpose(-1, -2)), dict(i=3, b=z(2, 64, 1)),
                dict(i=4, b=z(2, 64, 64, dt=torch.float32)), dict(blk=48)):
        b = bufs()
        if 'i' in bad:
            b[bad['i']] = bad['b']
        with pytest.raises(ValueError):
            native.kv_append(k, bad.get('v', k), *b, 0, bad.get('blk', 64), 7, 1e-8)
    for wc, we in ((z(2, 100, 64), z(2, 128, 1)), (z(2, 128, 64), z(2, 100, 1)), (z(2, 128, 64).float(), z(2, 128, 1)),
                   (z(2, 128, 128)[..., :64], z(2, 128, 1))):
        with pytest.raises(ValueError):
            native.kv_bmm_dec(k, wc, we, native.KV_QK, 100, 128, 64, 7, 1e-8)
