"""The codes-operand form of the prefill GEMM (bfpq_hbfp_linear_mx4w, hold_image=False) without a GPU: the exported entries and the
nibble -> e4m3 table the kernel uses, argument validation before any launch, the hold_image switch through extra state, and the routes
a hold_image=False module takes with every launch replaced by a recorder."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import quantization_sparsity_interplay_amd as pkg
import test_linear_routes_host as R
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, pack_linear_layers

MX4W = ("bfpq_hbfp_linear_mx4w_ok", "bfpq_hbfp_linear_mx4w", "bfpq_hbfp_linear_mx4w_parts", "bfpq_hbfp_linear_mx4w_splitk")


def e4m3_value(b):
    """OCP e4m3: sign, 4 exponent bits with bias 7, 3 mantissa bits (exponent 0: subnormal; 0x7f / 0xff: NaN)"""
    sign, e, m = -1.0 if b & 0x80 else 1.0, (b >> 3) & 15, b & 7
    assert (b & 0x7f) != 0x7f
    return sign * (m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7))


def test_exports_and_the_code_table():
    L = pkg.load_library()
    raw = ctypes.CDLL(native.lib_path())
    for name in MX4W + ("bfpq_e4m3_of_code4_host",):
        assert hasattr(raw, name) and name in native.EXPORTED_SYMBOLS, name
    assert L.bfpq_version() == 4
    table = (ctypes.c_uint8 * 16)()
    assert L.bfpq_e4m3_of_code4_host(table) == 0 and L.bfpq_e4m3_of_code4_host(None) == -1
    want = [n if n < 8 else n - 16 for n in range(16)]                      # two's-complement nibbles
    assert [e4m3_value(b) for b in table] == [float(v) for v in want]
    assert table[0] == 0                                                    # +0, not -0: a pruned code adds nothing, with no sign


def test_ok_agrees_with_the_image_form_and_arguments_are_checked_without_gpu():
    L = pkg.load_library()
    for T in (0, 1, 31, 64, 65, 128, 2048, 1 << 20):
        for N in (0, 1, 8, 24, 100, 129, 4096, 11008):
            for K in (0, 64, 192, 200, 256, 320, 768, 4096, 4160, 11008):
                assert L.bfpq_hbfp_linear_mx4w_ok(T, N, K) == L.bfpq_hbfp_linear_mx8_ok(T, N, K), (T, N, K)
                assert L.bfpq_hbfp_linear_mx4w_parts(T, N, K) == L.bfpq_hbfp_linear_mx8_parts(T, N, K), (T, N, K)
    assert L.bfpq_hbfp_linear_mx4w_ok(2048, 11008, 4096) == 1 and L.bfpq_hbfp_linear_mx4w_ok(2048, 11008, 4160) == 0
    assert L.bfpq_hbfp_linear_mx4w_ok(7, 24, 512) == 1                      # N % 16 != 0 is taken, as by the image form
    assert L.bfpq_hbfp_linear_mx4w_parts(128, 4096, 11008) == 8
    n, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(8)
    BF16, E_ARG, E_UNSUPPORTED = native.BF16, -1, -2
    f = L.bfpq_hbfp_linear_mx4w
    assert f(one, one, one, one, n, one, 8, 8, 256, BF16, 0, n) == E_ARG                     # w_mant_bits outside 1..3
    assert f(one, one, one, one, n, one, 8, 8, 256, BF16, 4, n) == E_ARG
    assert f(one, one, one, one, n, one, 8, 8, 256, 7, 3, n) == E_ARG                        # bad output dtype
    assert f(one, one, one, one, n, one, 8, 8, 200, BF16, 3, n) == E_UNSUPPORTED             # K % 256 != 0
    assert f(one, one, one, one, n, one, 8, 8, 64, BF16, 3, n) == E_UNSUPPORTED
    for k in (0, 1, 2, 3, 5):                                                                # every operand but the bias must be given
        ops = [one, one, one, one, n, one]
        ops[k] = n
        assert f(*ops, 8, 8, 256, BF16, 3, n) == E_ARG, k
    assert f(n, one, one, one, n, one, 8, 8, 256, BF16, 3, n) == E_ARG
    assert f(one, one, n, one, n, one, 8, 8, 256, BF16, 3, n) == E_ARG                       # no codes
    assert f(one, one, one, n, n, one, 8, 8, 256, BF16, 3, n) == E_ARG                       # no exponents
    assert f(one, one, odd, one, n, one, 8, 8, 256, BF16, 3, n) == E_ARG                     # codes not 16-byte aligned
    assert f(one, one, one, ctypes.c_void_p(18), n, one, 8, 8, 256, BF16, 3, n) == E_ARG     # exponents not 4-byte aligned
    assert f(one, one, one, one, n, one, 0, 8, 256, BF16, 3, n) == 0                         # no tokens: ok, no launch
    g = L.bfpq_hbfp_linear_mx4w_splitk
    assert g(one, one, one, one, n, one, n, 4, 8, 8, 256, BF16, 3, n) == E_ARG               # no slabs
    assert g(one, one, one, one, n, one, odd, 4, 8, 8, 256, BF16, 3, n) == E_ARG             # slabs not aligned
    assert g(one, one, one, one, n, one, one, 0, 8, 8, 256, BF16, 3, n) == E_ARG             # parts < 1
    assert g(one, one, one, one, n, one, one, 4, 8, 8, 256, BF16, 5, n) == E_ARG             # w_mant_bits outside 1..3
    assert g(one, one, one, one, n, one, one, 4, 8, 8, 256, 9, 3, n) == E_ARG                # bad dtype
    assert g(one, one, one, one, n, one, one, 4, 8, 8, 320, BF16, 3, n) == E_UNSUPPORTED     # refused shape
    assert g(one, one, n, one, n, one, one, 4, 8, 8, 256, BF16, 3, n) == E_ARG               # no codes
    assert g(one, one, one, one, n, one, one, 4, 0, 8, 256, BF16, 3, n) == 0                 # no tokens: ok
    assert native.hbfp_linear_mx4w_ok(2048, 4096, 4096, 3, 4) and not native.hbfp_linear_mx4w_ok(2048, 4096, 4096, 4, 3)
    assert not native.hbfp_linear_mx4w_ok(2048, 4096, 4096, 3, 5) and not native.hbfp_linear_mx4w_ok(2048, 4096, 4096, 3, 3, block_size=32)


def test_hold_image_travels_as_extra_state():
    mod = PackedBFPLinear(R._packed(32, 256, 4, 3), None, 3, 1e-8, hold_image=False)
    assert mod.hold_image is False and mod.get_extra_state()['hold_image'] is False and "hold_image=False" in repr(mod)
    dflt = PackedBFPLinear(R._packed(32, 256, 4, 3), None, 3, 1e-8)
    assert dflt.hold_image is True and dflt.get_extra_state()['hold_image'] is True and "hold_image" not in repr(dflt)
    dflt.set_extra_state(mod.get_extra_state())
    assert dflt.hold_image is False
    old = {k: v for k, v in mod.get_extra_state().items() if k != 'hold_image'}             # a state saved before the switch existed
    mod.set_extra_state(old)
    assert mod.hold_image is True
    a = PackedBFPLinear(bfp_ops.PackedBFP(torch.zeros(32, 128, dtype=torch.uint8), torch.zeros(32, 4, dtype=torch.int8), (32, 256),
                                          torch.bfloat16, 3, 64, 4), None, 3, 1e-8, hold_image=False)
    b = PackedBFPLinear(bfp_ops.PackedBFP(torch.ones(32, 128, dtype=torch.uint8), torch.ones(32, 4, dtype=torch.int8), (32, 256),
                                          torch.bfloat16, 3, 64, 4), None, 3, 1e-8)
    b.load_state_dict(a.state_dict())
    assert b.hold_image is False and torch.equal(b.codes, a.codes)
    assert a.packed.resident_bytes() == a.packed.nbytes() == 32 * 128 + 32 * 4
    a.packed._mx8 = (torch.zeros(32, 256, dtype=torch.uint8), torch.zeros(32, 4, dtype=torch.uint8))
    a.packed._tiles = (torch.zeros(32 * 128, dtype=torch.uint8), torch.zeros(32 * 4, dtype=torch.int8))
    assert a.packed.resident_bytes() == 2 * (32 * 128 + 32 * 4) + 32 * 256 + 32 * 4
    assert f"resident_bytes={a.packed.resident_bytes()}" in repr(a)


@pytest.fixture
def calls(monkeypatch):
    """the recorders of tests/test_linear_routes_host.py, plus one for the codes-operand GEMM; the weight's image builder is recorded too"""
    log = []

    def gemm(name, n_of):
        def f(x, *args, **kwargs):
            log.append(name)
            return R._zeros(tuple(x.shape[:-1]) + (n_of(args),), x.dtype)
        return f

    def mx8_from_hbfp(codes, exps, cols, mb, cb):
        log.append('image')
        return R._zeros((exps.shape[0], cols), torch.uint8), exps

    monkeypatch.setattr(native, 'require_device_tensor', lambda *a, **k: None)
    monkeypatch.setattr(native, 'hbfp_linear_decode_tiled', gemm('decode4', lambda a: a[2]))
    monkeypatch.setattr(native, 'hbfp_linear_mx8', gemm('mx8', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'hbfp_linear_mx4w', gemm('mx4w', lambda a: a[1].shape[0]))
    monkeypatch.setattr(native, 'hbfp_linear_i8', gemm('int8', lambda a: a[1].shape[0]))
    monkeypatch.setattr(F, 'linear', gemm('fake', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'mfma_tiles', lambda codes, exps: (codes, exps))
    monkeypatch.setattr(native, 'mx8_from_hbfp', mx8_from_hbfp)
    monkeypatch.setattr(native, 'codes4_to_i8', lambda codes4, n: R._zeros((n,), torch.int8))
    monkeypatch.setattr(native, 'dequantize', lambda codes, exps, cols, dtype, *a, **k: R._zeros((exps.shape[0], cols), dtype))
    monkeypatch.setattr(native, 'act_codes', lambda x, *a, **k: (R._zeros(x.shape, torch.int8), R._zeros((x.shape[0], 1), torch.int8)))
    monkeypatch.setattr(native.FastQuant, '__call__', lambda self, t, out=None: t)
    return log


def _taken(log):
    gemms = [c for c in log if c in R.GEMMS + ('mx4w',)]
    assert len(gemms) <= 1, log
    image = 'image' in log
    del log[:]
    return (gemms[0] if gemms else 'empty'), image


@pytest.mark.parametrize("act", [None, native.ActSparsity('structured', 2, 4, 0.0, 's')], ids=['dense', '2:4'])
def test_lean_module_routes(calls, act):
    """a hold_image=False module runs hbfp_linear_mx4w exactly where the table says 'mx8' for 4-bit block-64 codes, never asks for the
    weight's image there, and takes every other route (8-bit codes included) as the default module does"""
    for N, K, cb, wm, xm in R._sweep():
        lean = PackedBFPLinear(R._packed(N, K, cb, wm), None, xm, 1e-8, act, hold_image=False)
        held = PackedBFPLinear(R._packed(N, K, cb, wm), None, xm, 1e-8, act)
        for T in R.TOKENS:
            want = R.want_module(T, N, K, cb, wm, xm)
            with torch.no_grad():
                y = lean(R._zeros((T, K)))
            assert y.shape == (T, N)
            route, image = _taken(calls)
            if want == 'mx8' and cb == 4:
                assert (route, image) == ('mx4w', False), (T, N, K, cb, wm, xm)
            else:
                assert route == want and (not image or want == 'mx8'), (T, N, K, cb, wm, xm)    # (8-bit codes keep their image)
            with torch.no_grad():
                held(R._zeros((T, K)))
            route, _ = _taken(calls)
            assert route == want, (T, N, K, cb, wm, xm)
        assert getattr(lean.packed, '_mx8', None) is None or cb == 8
        assert bfp_ops.linear_route(2048, N, K, cb, wm, xm) == R.want_packed(2048, N, K, cb, wm, xm)       # the route's name is unchanged


def test_lean_packed_linear_and_small_blocks(calls):
    """PackedBFP.linear(hold_image=False); blocks 16 / 32 have no block-scaled route and are untouched"""
    pk = R._packed(4096, 4096, 4, 3)
    pk.linear(R._zeros((2048, 4096)), None, 3, hold_image=False)
    assert _taken(calls) == ('mx4w', False) and getattr(pk, '_mx8', None) is None
    pk.linear(R._zeros((2048, 4096)), None, 3)
    assert _taken(calls) == ('mx8', True) and pk._mx8 is not None
    pk.linear(R._zeros((16, 4096)), None, 3, hold_image=False)
    assert _taken(calls) == ('decode4', False)
    small = bfp_ops.PackedBFP(R._zeros((4096, 2048), torch.uint8), R._zeros((4096, 128), torch.int8), (4096, 4096), torch.bfloat16, 3, 32, 4)
    small.linear(R._zeros((8, 4096)), None, 3, hold_image=False)
    assert _taken(calls)[0] == 'int8'


def test_measured_fallback_of_the_codes_route(calls):
    """where the codes route did not beat the dequantize + library GEMM route by more than the spread (profiles/r10_prefill_codes.json:
    q_proj at 8192 tokens), hold_image=False takes that route; it holds no image either"""
    assert (bfp_ops.CODES_FAKE_MIN_TOKENS, bfp_ops.CODES_FAKE_MAX_WEIGHT) == (8192, 4096 * 4096)
    for (N, K, T), want in (((4096, 4096, 8192), 'fake'), ((4096, 4096, 8191), 'mx4w'), ((4096, 4096, 2048), 'mx4w'),
                            ((11008, 4096, 8192), 'mx4w'), ((4096, 11008, 8192), 'mx4w'), ((2048, 4096, 16384), 'fake')):
        assert bfp_ops.codes_route(T, N, K) == want
        pk = R._packed(N, K, 4, 3)
        pk.linear(R._zeros((T, K)), None, 3, hold_image=False)
        assert _taken(calls) == (want, False) and getattr(pk, '_mx8', None) is None
        pk.linear(R._zeros((T, K)), None, 3)
        assert _taken(calls)[0] == 'mx8'


def test_pack_linear_layers_passes_the_switch(calls, monkeypatch):
    def quantize_nm(t, block_size, mant_bits, epsilon, *args, code_bits=0, **kwargs):
        return None, R._zeros((t.shape[0], t.shape[-1] * code_bits // 8), torch.uint8), R._zeros((t.shape[0], t.shape[-1] // 64), torch.int8)
    monkeypatch.setattr(native, 'quantize_nm', quantize_nm)
    monkeypatch.setattr(native, 'require_device_tensor_any', lambda *a, **k: None, raising=False)
    args = pkg.BFPConfig.hbfp(4, 64, w_sparsity=True, N=2, M=4, sparsity_mode='structured', first='s').to_kwargs()
    args['rounding_mode'] = 'determ'
    sizes = []
    for hold in (True, False):
        model = torch.nn.Sequential(torch.nn.Linear(256, 64), torch.nn.Linear(64, 32))       # (the second one's K is not packable)
        names, saved = pack_linear_layers(model, args, **({} if hold else {'hold_image': False}))
        assert names == ['0'] and isinstance(model[0], PackedBFPLinear) and model[0].hold_image is hold
        sizes.append(saved)
    assert sizes[0] == sizes[1] == 64 * 256 * 4 - (64 * 128 + 64 * 4)                        # "bytes saved" keeps its meaning
