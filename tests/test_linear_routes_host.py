"""The route table of the packed Linear forwards, row by row: which kernel PackedBFP.linear, PackedBFPLinear and the cached
BFPLinear(matrix_unit=...) run for T tokens of an [N, K] weight.  No GPU needed: the native predicates (hbfp_linear_mx8_ok / _i8_ok)
answer on the host, and every launch is replaced by a recorder.  The expected route comes from the table written out below; the forwards
must take it, and bfp_ops.linear_route must name it."""
import pytest
import torch
import torch.nn.functional as F

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear

TOKENS = (0, 1, 16, 32, 64, 65, 512, 513, 2048)
WIDTHS = (3, 4, 5, 7)
# LLaMA-7B q/k/v/o, gate/up and down projections; N % 16 != 0; K % 64 != 0
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008), (24, 512), (32, 96))
GEMMS = ('decode4', 'mx8', 'int8', 'fake')
mx8_ok, i8_ok = native.hbfp_linear_mx8_ok, native.hbfp_linear_i8_ok


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def want_packed(T, N, K, cb, wm, xm, decode_tokens=64):
    """PackedBFP.linear, and PackedBFPLinear with 4-bit codes"""
    if T == 0:
        return 'empty'
    if cb == 4 and T <= decode_tokens and N % 16 == 0 and K % 256 == 0:
        return 'decode4'
    if cb in (4, 8) and mx8_ok(T, N, K, wm, xm):
        return 'mx8'
    return 'fake'


def want_module(T, N, K, cb, wm, xm):
    """PackedBFPLinear: 8-bit codes take the int8 unit up to 512 tokens, unless past 64 tokens the block-scaled route runs"""
    if cb == 8 and 1 <= T <= 512 and not (T > 64 and mx8_ok(T, N, K, wm, xm)) and i8_ok(T, N, K, wm, xm):
        return 'int8'
    return want_packed(T, N, K, cb, wm, xm)


def want_cached(T, N, K, m, matrix_unit):
    """the cached BFPLinear under no_grad, on a configuration the matrix-unit routes cover ('fake': the fake-quantize path)"""
    if matrix_unit == 'int8' and m <= 7 and T >= 1 and i8_ok(T, N, K, m, m):
        return 'int8'
    if matrix_unit is True and m <= 4 and T >= 32 and mx8_ok(T, N, K, m, m):
        return 'mx8'
    return 'fake'


# ---- recorders ------------------------------------------------------------------------------------------------------------------------
def _zeros(shape, dtype=torch.bfloat16):
    """a stand-in tensor of any size that takes no memory"""
    return torch.zeros((), dtype=dtype).expand(*shape)


class _OnDevice(torch.Tensor):
    """a host tensor that reports a ROCm device: the cached forward checks x.device before it picks a matrix-unit route"""

    @property
    def device(self):
        return torch.device('cuda', 0)


@pytest.fixture
def calls(monkeypatch):
    """every launch of the packed forwards replaced by a recorder; returns the list of recorded names"""
    log = []

    def gemm(name, n_of):
        def f(x, *args, **kwargs):
            log.append(name)
            return _zeros(tuple(x.shape[:-1]) + (n_of(args),), x.dtype)
        return f

    def quantize_nm(t, block_size, mant_bits, epsilon, *args, code_bits=0, **kwargs):
        log.append('pack')
        return None, _zeros((t.numel() * code_bits // 8,), torch.uint8 if code_bits == 4 else torch.int8), \
            _zeros((t.shape[0], max(t.shape[-1] // 64, 1)), torch.int8)

    def fast_quant(self, t, out=None):
        log.append('quant')
        return t

    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **k: None)
    monkeypatch.setattr(native, 'hbfp_linear_decode_tiled', gemm('decode4', lambda a: a[2]))
    monkeypatch.setattr(native, 'hbfp_linear_mx8', gemm('mx8', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'hbfp_linear_i8', gemm('int8', lambda a: a[1].shape[0]))
    monkeypatch.setattr(F, 'linear', gemm('fake', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'mfma_tiles', lambda codes, exps: (codes, exps))
    monkeypatch.setattr(native, 'mx8_from_hbfp', lambda codes, exps, cols, mb, cb: (_zeros((exps.shape[0], cols), torch.uint8), exps))
    monkeypatch.setattr(native, 'codes4_to_i8', lambda codes4, n: _zeros((n,), torch.int8))
    monkeypatch.setattr(native, 'dequantize', lambda codes, exps, cols, dtype, *a, **k: _zeros((exps.shape[0], cols), dtype))
    monkeypatch.setattr(native, 'act_codes', lambda x, *a, **k: (_zeros(x.shape, torch.int8), _zeros((x.shape[0], 1), torch.int8)))
    monkeypatch.setattr(native, 'quantize_nm', quantize_nm)
    monkeypatch.setattr(native.FastQuant, '__call__', fast_quant)
    return log


def _route(log):
    """the route one forward took: its one GEMM launch, or 'empty' for none"""
    gemms = [c for c in log if c in GEMMS]
    assert len(gemms) <= 1, log
    del log[:]
    return gemms[0] if gemms else 'empty'


def _packed(N, K, cb, wm):
    return bfp_ops.PackedBFP(_zeros((N, K * cb // 8), torch.uint8 if cb == 4 else torch.int8), _zeros((N, max(K // 64, 1)), torch.int8),
                             (N, K), torch.bfloat16, wm, 64, cb)


def _sweep():
    for N, K in SHAPES:
        for cb in (4, 8):
            for wm in WIDTHS:
                for xm in WIDTHS:
                    yield N, K, cb, wm, xm


# ---- the forwards ---------------------------------------------------------------------------------------------------------------------
def test_packed_linear_routes(calls):
    for N, K, cb, wm, xm in _sweep():
        pk = _packed(N, K, cb, wm)
        for T in TOKENS:
            assert pk.linear(_zeros((T, K)), None, xm).shape == (T, N)
            assert _route(calls) == want_packed(T, N, K, cb, wm, xm), (T, N, K, cb, wm, xm)
        pk.linear(_zeros((16, K)), None, xm, decode_tokens=0)
        assert _route(calls) == want_packed(16, N, K, cb, wm, xm, decode_tokens=0), (N, K, cb, wm, xm)


@pytest.mark.parametrize("act", [None, native.ActSparsity('structured', 2, 4, 0.0, 's')], ids=['dense', '2:4'])
def test_packed_module_routes(calls, act):
    for N, K, cb, wm, xm in _sweep():
        mod = PackedBFPLinear(_packed(N, K, cb, wm), None, xm, 1e-8, act)
        for T in TOKENS:
            with torch.no_grad():
                y = mod(_zeros((T, K)))
            assert y.shape == (T, N)
            assert _route(calls) == want_module(T, N, K, cb, wm, xm), (T, N, K, cb, wm, xm)


@pytest.mark.parametrize("matrix_unit", [True, 'int8'])
def test_cached_bfplinear_routes(calls, matrix_unit):
    for N, K in SHAPES:
        w = _zeros((N, K)).as_subclass(_OnDevice)
        for m in WIDTHS:
            cfg = dict(num_format='bfp', sparsity_num_format='bfp', block_size=64, mant_bits=m, rounding_mode='determ', epsilon=1e-8)
            lin = bfp_ops.BFPLinear(64, 16, **cfg).eval().enable_weight_cache(matrix_unit=matrix_unit)
            cache = lin._weight_cache
            for T in TOKENS:
                mx, i8 = cache.mx_calls, cache.i8_calls
                with torch.no_grad():
                    y = lin.linear_op(_zeros((T, K)).as_subclass(_OnDevice), w)
                assert y.shape == (T, N)
                want = want_cached(T, N, K, m, matrix_unit)
                assert _route(calls) == want, (T, N, K, m)
                assert (cache.mx_calls - mx, cache.i8_calls - i8) == ((want == 'mx8') * 1, (want == 'int8') * 1)


def test_item4_shapes_leave_the_int8_unit():
    """an 8-bit-code module whose shape the int8 unit refuses (out_features % 16 != 0, in_features % 64 != 0) runs PackedBFP.linear's
    routes at every token count instead of raising from hbfp_linear_i8"""
    for N, K in ((24, 512), (32, 96)):
        for T in (1, 7, 200, 512, 513):
            assert want_module(T, N, K, 8, 7, 7) == 'fake'
            assert bfp_ops.linear_route(T, N, K, 8, 7, 7, i8_max_tokens=bfp_ops.I8_MAX_TOKENS) == 'fake'


# ---- the pure function ----------------------------------------------------------------------------------------------------------------
def test_linear_route_table():
    R = bfp_ops.linear_route
    for N, K, cb, wm, xm in _sweep():
        for T in TOKENS:
            where = (T, N, K, cb, wm, xm)
            assert R(T, N, K, cb, wm, xm) == want_packed(T, N, K, cb, wm, xm), where
            assert R(T, N, K, cb, wm, xm, decode_tokens=0) == want_packed(T, N, K, cb, wm, xm, decode_tokens=0), where
            assert R(T, N, K, cb, wm, xm, i8_max_tokens=bfp_ops.I8_MAX_TOKENS) == want_module(T, N, K, cb, wm, xm), where
    for N, K in SHAPES:
        for m in WIDTHS:
            for T in TOKENS:
                i8 = R(T, N, K, 8, m, m, decode_tokens=0, i8_max_tokens=None, mx8_min_tokens=None)
                mx = R(T, N, K, bfp_ops.code_bits_for(m), m, m, decode_tokens=0, mx8_min_tokens=bfp_ops.CACHED_MX8_MIN_TOKENS)
                assert (i8 if T else 'fake') == want_cached(T, N, K, m, 'int8'), (T, N, K, m)
                assert (mx if T else 'fake') == want_cached(T, N, K, m, True), (T, N, K, m)


def test_linear_route_asks_each_predicate_once(monkeypatch):
    asked = []
    monkeypatch.setattr(native, 'hbfp_linear_mx8_ok', lambda *a, **k: asked.append('mx8') or False)
    monkeypatch.setattr(native, 'hbfp_linear_i8_ok', lambda *a, **k: asked.append('i8') or False)
    for T in TOKENS:
        for cb in (4, 8):
            for opts in (dict(), dict(i8_max_tokens=bfp_ops.I8_MAX_TOKENS), dict(decode_tokens=0, i8_max_tokens=None, mx8_min_tokens=None)):
                asked.clear()
                bfp_ops.linear_route(T, 24, 512, cb, 4, 4, **opts)
                assert sorted(set(asked)) == sorted(asked), (T, cb, opts, asked)


def test_code_bits_rule():
    assert [bfp_ops.code_bits_for(m) for m in range(1, 11)] == [4, 4, 4, 8, 8, 8, 8, 16, 16, 16]
