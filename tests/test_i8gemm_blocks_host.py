"""Host-side checks of the int8 matrix-unit GEMM at HBFP blocks 16 and 32: argument validation of the new entry points, the route table
rows of these blocks, the packer and the extra state of a block-16 module.  No GPU needed: every C call here is refused before it launches,
and the route checks replace every launch by a recorder (as tests/test_linear_routes_host.py does)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_hbfp_linear_i8b_ok", "bfpq_hbfp_linear_i8b_parts", "bfpq_hbfp_linear_i8b", "bfpq_hbfp_linear_i8b_splitk",
       "bfpq_hbfp_linear_decode8b_ws", "bfpq_hbfp_linear_decode8b")
P = ctypes.c_void_p(16)
Z = None
S = ctypes.c_void_p(0)
BAD_BLOCKS = (8, 48, 128, 64, 0, -16)


def L():
    return native.load_library()


def test_new_entries_are_exported():
    assert set(NEW) <= set(native.EXPORTED_SYMBOLS)
    for name in NEW:
        assert hasattr(L(), name), name


@pytest.mark.parametrize("blk", BAD_BLOCKS)
def test_b_entries_refuse_other_blocks(blk):
    assert L().bfpq_hbfp_linear_i8b_ok(128, 64, 512, blk) == 0
    assert L().bfpq_hbfp_linear_i8b_parts(128, 64, 512, blk) == E_ARG
    assert L().bfpq_hbfp_linear_decode8b_ws(1, 64, 512, blk) == E_ARG
    assert L().bfpq_hbfp_linear_i8b(P, P, P, P, Z, P, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert L().bfpq_hbfp_linear_i8b_splitk(P, P, P, P, Z, P, P, 2, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert L().bfpq_hbfp_linear_decode8b(P, P, P, P, Z, P, P, 1, 16, 256, blk, 2, 7, 7, S) == E_ARG
    if blk != 64:                                                       # (the Python predicate takes block 64 too)
        assert not native.hbfp_linear_i8_ok(16, 16, 256, 7, 7, block_size=blk)


@pytest.mark.parametrize("blk", (16, 32))
def test_ok_parts_ws_and_merged_predicate(blk):
    ok = L().bfpq_hbfp_linear_i8b_ok
    assert ok(1, 16, 256, blk) == 1 and ok(2048, 4096, 1024, blk) == 1 and ok(197, 768, 3072, blk) == 1
    assert ok(0, 16, 256, blk) == 0 and ok(1, 24, 256, blk) == 0 and ok(1, 16, 192, blk) == 0
    parts = L().bfpq_hbfp_linear_i8b_parts
    assert parts(2048, 4096, 4096, blk) == 1 and 2 <= parts(128, 1024, 4096, blk) <= 8 and parts(1, 16, 192, blk) == 1
    ws = L().bfpq_hbfp_linear_decode8b_ws
    assert ws(1, 16, 64, blk) == 16 * 16                                # the slices of the block-64 plan, one token group of 16 rows
    assert ws(17, 1024, 4096, blk) > 0 and ws(17, 1024, 4096, blk) % (32 * 1024) == 0
    assert ws(0, 16, 64, blk) == E_UNSUPPORTED and ws(1, 24, 64, blk) == E_UNSUPPORTED and ws(1, 16, 96, blk) == E_UNSUPPORTED
    # the Python predicate takes blocks 16, 32 and 64 alike and refuses 8-bit mantissas
    assert all(native.hbfp_linear_i8_ok(16, 16, 256, 7, 7, block_size=b) for b in (16, 32, 64))
    assert not native.hbfp_linear_i8_ok(16, 16, 256, 8, 7, block_size=blk) and not native.hbfp_linear_i8_ok(16, 16, 256, 7, 8, block_size=blk)


@pytest.mark.parametrize("blk", (16, 32))
@pytest.mark.parametrize("dt,wm,xm", [(3, 7, 7), (-1, 7, 7), (2, 0, 7), (2, 8, 7), (2, 7, 0), (2, 7, 8)])
def test_bad_enums(blk, dt, wm, xm):
    assert L().bfpq_hbfp_linear_i8b(P, P, P, P, Z, P, 16, 16, 256, blk, dt, wm, xm, S) == E_ARG
    assert L().bfpq_hbfp_linear_i8b_splitk(P, P, P, P, Z, P, P, 2, 16, 16, 256, blk, dt, wm, xm, S) == E_ARG
    assert L().bfpq_hbfp_linear_decode8b(P, P, P, P, Z, P, P, 16, 16, 256, blk, dt, wm, xm, S) == E_ARG


@pytest.mark.parametrize("blk", (16, 32))
def test_shapes_and_pointers(blk):
    i8, sk, d8 = L().bfpq_hbfp_linear_i8b, L().bfpq_hbfp_linear_i8b_splitk, L().bfpq_hbfp_linear_decode8b
    assert i8(P, P, P, P, Z, P, 16, 16, 192, blk, 2, 7, 7, S) == E_UNSUPPORTED
    assert i8(P, P, P, P, Z, P, 16, 24, 256, blk, 2, 7, 7, S) == E_UNSUPPORTED
    assert i8(Z, P, P, P, Z, P, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert i8(ctypes.c_void_p(8), P, P, P, Z, P, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert i8(P, ctypes.c_void_p(18), P, P, Z, P, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    if blk == 16:
        assert i8(P, ctypes.c_void_p(20), P, P, Z, P, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG     # two exponent dwords per stage
    assert i8(P, P, P, P, Z, P, 0, 16, 256, blk, 2, 7, 7, S) == 0
    assert i8(P, P, P, P, Z, P, -1, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert sk(P, P, P, P, Z, P, P, 0, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert sk(P, P, P, P, Z, P, P, 65, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert sk(P, P, P, P, Z, P, Z, 2, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert sk(P, P, P, P, Z, P, ctypes.c_void_p(20), 2, 16, 16, 256, blk, 2, 7, 7, S) == E_ARG
    assert d8(P, P, P, P, Z, P, P, 1, 16, 96, blk, 2, 7, 7, S) == E_UNSUPPORTED
    assert d8(P, P, P, P, Z, P, P, 0, 16, 64, blk, 2, 7, 7, S) == E_ARG
    assert d8(P, P, P, P, Z, P, Z, 1, 16, 64, blk, 2, 7, 7, S) == E_ARG


# ---- the route table at blocks 16 and 32 --------------------------------------------------------------------------------------------
TOKENS = (0, 1, 16, 17, 64, 65, 197, 512, 513, 1576, 2048)
SHAPES = ((768, 768), (3072, 768), (768, 3072), (1024, 1024), (4096, 1024), (1024, 4096), (24, 512), (32, 96))
GEMMS = ('decode4', 'mx8', 'int8', 'fake')


DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def want_small(T, N, K, cb, wm, xm, blk, dtype=None, any_tokens=False):
    """blocks 16 / 32: the int8 unit (4- and 8-bit codes) up to the measured limit of the block and the activation dtype (any number of tokens
    for the cached forward), else the fake route"""
    if T == 0:
        return 'empty'
    lim = None if any_tokens else bfp_ops.I8_SMALL_BLOCK_MAX_TOKENS.get((blk, dtype), bfp_ops.I8_SMALL_BLOCK_MAX_TOKENS[(blk, torch.bfloat16)])
    if cb in (4, 8) and (lim is None or T <= lim) and N % 16 == 0 and K % 64 == 0 and wm <= 7 and xm <= 7:
        return 'int8'
    return 'fake'


def _zeros(shape, dtype=torch.bfloat16):
    return torch.zeros((), dtype=dtype).expand(*shape)


class _OnDevice(torch.Tensor):
    @property
    def device(self):
        return torch.device('cuda', 0)


@pytest.fixture
def calls(monkeypatch):
    log = []

    def gemm(name, n_of):
        def f(x, *args, **kwargs):
            log.append((name, kwargs.get('block_size')))
            return _zeros(tuple(x.shape[:-1]) + (n_of(args),), x.dtype)
        return f

    def quantize_nm(t, block_size, mant_bits, epsilon, *args, code_bits=0, **kwargs):
        return None, _zeros((t.numel() * code_bits // 8,), torch.uint8 if code_bits == 4 else torch.int8), \
            _zeros((t.shape[0], max(t.shape[-1] // block_size, 1)), torch.int8)

    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **k: None)
    monkeypatch.setattr(native, 'hbfp_linear_decode_tiled', gemm('decode4', lambda a: a[2]))
    monkeypatch.setattr(native, 'hbfp_linear_mx8', gemm('mx8', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'hbfp_linear_i8', gemm('int8', lambda a: a[1].shape[0]))
    monkeypatch.setattr(F, 'linear', gemm('fake', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'codes4_to_i8', lambda codes4, n: _zeros((n,), torch.int8))
    monkeypatch.setattr(native, 'dequantize', lambda codes, exps, cols, dtype, *a, **k: _zeros((exps.shape[0], cols), dtype))
    monkeypatch.setattr(native, 'quantize_nm', quantize_nm)
    monkeypatch.setattr(native.FastQuant, '__call__', lambda self, t, out=None: t)
    return log


def _route(log, blk):
    gemms = [c for c in log if c[0] in GEMMS]
    assert len(gemms) <= 1, log
    del log[:]
    if not gemms:
        return 'empty'
    name, b = gemms[0]
    if name == 'int8':
        assert b == blk, (b, blk)                        # the int8 unit is told the block
    return name


def _packed(N, K, cb, wm, blk):
    return bfp_ops.PackedBFP(_zeros((N, K * cb // 8), torch.uint8 if cb == 4 else torch.int8), _zeros((N, max(K // blk, 1)), torch.int8),
                             (N, K), torch.float32, wm, blk, cb)


def test_limits_table():
    """fp32 activations (BASELINE configs 1 and 5) take the int8 unit at every token count; 16-bit ones up to the few-token kernel"""
    for blk in (16, 32):
        assert bfp_ops.i8_small_block_max_tokens(blk, torch.float32) is None
        assert bfp_ops.i8_small_block_max_tokens(blk, torch.bfloat16) == bfp_ops.i8_small_block_max_tokens(blk, None)
        for dt in DTYPES:
            assert (blk, dt) in bfp_ops.I8_SMALL_BLOCK_MAX_TOKENS
    assert bfp_ops.linear_route(2048, 4096, 1024, 8, 7, 7, i8_max_tokens=bfp_ops.I8_MAX_TOKENS, block_size=16, dtype=torch.float32) == 'int8'
    assert bfp_ops.linear_route(197, 3072, 768, 8, 7, 7, block_size=32, dtype=torch.float32) == 'int8'


@pytest.mark.parametrize("blk", (16, 32))
@pytest.mark.parametrize("dt", DTYPES + (None,), ids=['fp32', 'bf16', 'fp16', 'none'])
def test_linear_route_table(blk, dt):
    R = bfp_ops.linear_route
    for N, K in SHAPES:
        for cb in (4, 8):
            for m in (1, 3, 4, 7):
                for T in TOKENS:
                    want = want_small(T, N, K, cb, m, m, blk, dt)
                    assert R(T, N, K, cb, m, m, block_size=blk, dtype=dt) == want, (T, N, K, cb, m)
                    assert R(T, N, K, cb, m, m, i8_max_tokens=bfp_ops.I8_MAX_TOKENS, block_size=blk, dtype=dt) == want
                    assert R(T, N, K, cb, m, m, decode_tokens=0, i8_max_tokens=None, mx8_min_tokens=None, block_size=blk, dtype=dt) == \
                        want_small(T, N, K, cb, m, m, blk, any_tokens=True)


@pytest.mark.parametrize("blk", (16, 32))
@pytest.mark.parametrize("dt", DTYPES, ids=['fp32', 'bf16', 'fp16'])
def test_packed_forwards_routes(calls, blk, dt):
    for N, K in SHAPES:
        for cb, wm in ((4, 3), (8, 7)):
            pk = _packed(N, K, cb, wm, blk)
            mod = PackedBFPLinear(pk, None, 7, 1e-8, native.ActSparsity('structured', 1, 4, 0.0, 's'))
            for T in TOKENS:
                want = want_small(T, N, K, cb, wm, 7, blk, dt)
                assert pk.linear(_zeros((T, K), dt), None, 7).shape == (T, N)
                assert _route(calls, blk) == want, (T, N, K, cb)
                with torch.no_grad():
                    assert mod(_zeros((T, K), dt)).shape == (T, N)
                assert _route(calls, blk) == want, (T, N, K, cb)


@pytest.mark.parametrize("blk", (16, 32))
@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16), ids=['fp32', 'bf16'])
def test_cached_bfplinear_routes(calls, blk, dt):
    """the cached matrix_unit='int8' forward: the int8 unit at any token count, as at block 64"""
    for N, K in SHAPES:
        w = _zeros((N, K), dt).as_subclass(_OnDevice)
        for m in (4, 7):
            cfg = dict(num_format='bfp', sparsity_num_format='bfp', block_size=blk, mant_bits=m, rounding_mode='determ', epsilon=1e-8)
            lin = bfp_ops.BFPLinear(64, 16, **cfg).eval().enable_weight_cache(matrix_unit='int8')
            cache = lin._weight_cache
            for T in TOKENS:
                i8 = cache.i8_calls
                with torch.no_grad():
                    y = lin.linear_op(_zeros((T, K), dt).as_subclass(_OnDevice), w)
                assert y.shape == (T, N)
                want = 'fake' if T == 0 else want_small(T, N, K, 8, m, m, blk, any_tokens=True)
                got = _route(calls, blk)
                assert (got if T else 'fake') == want, (T, N, K, m)
                assert cache.i8_calls - i8 == (want == 'int8') * 1


def test_block64_cached_route_unchanged_and_mx8_stays_block_64():
    """matrix_unit=True (the block-scaled route) keeps refusing blocks 16 and 32"""
    w = _zeros((256, 512), torch.float32).as_subclass(_OnDevice)
    x = _zeros((64, 512), torch.float32).as_subclass(_OnDevice)
    for blk in (16, 32):
        cfg = dict(num_format='bfp', sparsity_num_format='bfp', block_size=blk, mant_bits=3, rounding_mode='determ', epsilon=1e-8)
        lin = bfp_ops.BFPLinear(512, 256, **cfg).eval().enable_weight_cache(matrix_unit=True)
        assert bfp_ops._cached_route(x, w, lin.bfp_args, lin._weight_cache) == 'fake'


# ---- the packer and the module's extra state -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", (16, 32))
def test_from_bfp_args_accepts_blocks_16_and_32(monkeypatch, blk):
    seen = []

    def quantize_nm(t, block_size, mant_bits, epsilon, N=0, M=0, sparsify_first=True, want_deq=True, code_bits=0, want_exp=False, **kw):
        seen.append((block_size, mant_bits, code_bits, N, M))
        return None, torch.zeros((t.shape[0], t.shape[1] * code_bits // 8), dtype=torch.int8), \
            torch.zeros((t.shape[0], t.shape[1] // block_size), dtype=torch.int8)

    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **k: None)
    monkeypatch.setattr(native, 'quantize_nm', quantize_nm)
    w = torch.zeros(64, 256)
    for m in (1, 3, 4, 7):
        a = bfp_ops.unpack_bfp_args(dict(num_format='bfp', sparsity_num_format='bfp', block_size=blk, mant_bits=m, rounding_mode='determ',
                                         w_sparsity=True, sparsity_mode='structured', N=1, M=4))
        pk = bfp_ops.PackedBFP.from_bfp_args(w, a)
        assert pk.block_size == blk and pk.code_bits == bfp_ops.code_bits_for(m) and pk.exps.shape == (64, 256 // blk)
        assert seen[-1] == (blk, m, bfp_ops.code_bits_for(m), 1, 4)
    # the refusals stay
    base = dict(num_format='bfp', sparsity_num_format='bfp', block_size=blk, rounding_mode='determ')
    with pytest.raises(AssertionError):
        bfp_ops.PackedBFP.from_bfp_args(w, bfp_ops.unpack_bfp_args(dict(base, mant_bits=8)))
    with pytest.raises(ValueError):
        bfp_ops.PackedBFP.from_bfp_args(w, bfp_ops.unpack_bfp_args(dict(base, mant_bits=7, rounding_mode='stoc')))
    with pytest.raises(ValueError):
        bfp_ops.PackedBFP.from_bfp_args(w, bfp_ops.unpack_bfp_args(dict(base, mant_bits=7, w_sparsity=True, sparsity_mode='unstructured',
                                                                         sparsity_frac=0.5, first='q')))
    for bad in (8, 48, 128):
        with pytest.raises(AssertionError):
            bfp_ops.PackedBFP.from_bfp_args(w, bfp_ops.unpack_bfp_args(dict(base, mant_bits=7, block_size=bad)))


def test_block16_module_extra_state_round_trip():
    N, K = 64, 256
    pk = bfp_ops.PackedBFP(torch.arange(N * K, dtype=torch.int32).remainder(255).sub(127).to(torch.int8).view(N, K),
                           torch.arange(N * K // 16, dtype=torch.int32).remainder(7).sub(3).to(torch.int8).view(N, K // 16),
                           (N, K), torch.float32, 7, 16, 8)
    act = native.ActSparsity('structured', 1, 4, 0.0, 's')
    mod = PackedBFPLinear(pk, torch.ones(N), 7, 1e-8, act)
    sd = mod.state_dict()
    # a module of other metadata (the buffers must match in shape for load_state_dict): the block comes back from the extra state
    empty = bfp_ops.PackedBFP(torch.zeros((N, K), dtype=torch.int8), torch.zeros((N, K // 16), dtype=torch.int8), (N, K), torch.bfloat16, 3, 64, 8)
    other = PackedBFPLinear(empty, torch.zeros(N), 3, 1e-3, None)
    other.load_state_dict(sd)
    p = other.packed
    assert (p.block_size, p.mant_bits, p.code_bits, p.dtype, p.shape) == (16, 7, 8, torch.float32, (N, K))
    assert other.x_sparsity == act and other.x_mant_bits == 7
    assert torch.equal(p.codes, pk.codes) and torch.equal(p.exps, pk.exps)
    moved = other.to(torch.float64)                        # (.to() keeps the buffers' meaning: int8 codes stay int8)
    assert moved.packed.block_size == 16 and moved.packed.codes.dtype == torch.int8


def test_exponent_shapes_are_checked_against_the_block(monkeypatch):
    """block-64 exponents with block_size=16 (the kernels would read past them), or block-16 exponents at block 64, are refused before
    anything runs"""
    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **k: None)
    T, N, K = 4, 64, 256
    x = torch.zeros((T, K))
    wc = torch.zeros((N, K), dtype=torch.int8)
    for blk, wrong in ((16, 64), (32, 64), (64, 16), (16, 32)):
        with pytest.raises(ValueError, match="exponents"):
            native.hbfp_linear_i8(x, wc, torch.zeros((N, K // wrong), dtype=torch.int8), 7, 7, block_size=blk)
        xq = (torch.zeros((T, K), dtype=torch.int8), torch.zeros((T, K // wrong), dtype=torch.int8))
        with pytest.raises(ValueError, match="exponents"):
            native.hbfp_linear_i8(x, wc, torch.zeros((N, K // blk), dtype=torch.int8), 7, 7, xq=xq, block_size=blk)
