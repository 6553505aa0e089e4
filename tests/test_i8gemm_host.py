"""Host-side checks of the HBFP5-HBFP8 int8 matrix-unit GEMM (bfpq_i8gemm.hip): exports, argument validation, the matrix_unit switch
and the 8-bit-code PackedBFPLinear extra state.  No GPU needed: every call here fails its checks before launching anything."""
import ctypes

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear, patch_linear_layers

E_ARG, E_UNSUPPORTED = -1, -2
NEW = ("bfpq_hbfp_linear_i8_ok", "bfpq_hbfp_linear_i8_parts", "bfpq_hbfp_linear_i8", "bfpq_hbfp_linear_i8_splitk",
       "bfpq_hbfp_linear_decode8_ws", "bfpq_hbfp_linear_decode8", "bfpq_codes4_to_i8")
P = ctypes.c_void_p(16)          # a non-null, 16-byte aligned dummy (never dereferenced: every call below is refused first)
Z = None


def L():
    return native.load_library()


def test_new_entries_are_exported():
    assert set(NEW) <= set(native.EXPORTED_SYMBOLS)
    for name in NEW:
        assert hasattr(L(), name), name
    assert L().bfpq_version() == 4


def test_i8_ok_and_parts():
    ok = L().bfpq_hbfp_linear_i8_ok
    assert ok(1, 16, 256) == 1 and ok(2048, 11008, 4096) == 1 and ok(128, 4096, 11008) == 1
    assert ok(0, 16, 256) == 0 and ok(1, 8, 256) == 0 and ok(1, 24, 256) == 0 and ok(1, 16, 192) == 0 and ok(1, 16, 128) == 0
    parts = L().bfpq_hbfp_linear_i8_parts
    assert parts(2048, 11008, 4096) == 1                       # enough tiles
    assert 2 <= parts(128, 4096, 11008) <= 8                    # 128 tokens x down_proj: too few tiles
    assert parts(1, 16, 192) == 1                              # not a tile shape
    assert L().bfpq_tune(4, 3) == E_ARG and L().bfpq_tune(4, -2) == E_ARG and L().bfpq_tune(5, 65) == E_ARG and L().bfpq_tune(5, -1) == E_ARG
    try:
        assert L().bfpq_tune(5, 3) == 0 and parts(128, 4096, 11008) == 3 and parts(128, 4096, 512) == 2     # capped at K / 256
    finally:
        assert L().bfpq_tune(5, 0) == 0
    assert L().bfpq_tune(4, -1) == 0


def test_decode8_ws():
    ws = L().bfpq_hbfp_linear_decode8_ws
    assert ws(1, 16, 64) == 16 * 16                            # one slice, one token group of 16 rows
    assert ws(17, 4096, 4096) > 0 and ws(17, 4096, 4096) % (32 * 4096) == 0
    assert ws(0, 16, 64) == E_UNSUPPORTED and ws(1, 24, 64) == E_UNSUPPORTED and ws(1, 16, 96) == E_UNSUPPORTED


@pytest.mark.parametrize("dt,wm,xm", [(3, 7, 7), (-1, 7, 7), (2, 0, 7), (2, 8, 7), (2, 7, 0), (2, 7, 8)])
def test_bad_enums(dt, wm, xm):
    s = ctypes.c_void_p(0)
    assert L().bfpq_hbfp_linear_i8(P, P, P, P, Z, P, 16, 16, 256, dt, wm, xm, s) == E_ARG
    assert L().bfpq_hbfp_linear_i8_splitk(P, P, P, P, Z, P, P, 2, 16, 16, 256, dt, wm, xm, s) == E_ARG
    assert L().bfpq_hbfp_linear_decode8(P, P, P, P, Z, P, P, 16, 16, 256, dt, wm, xm, s) == E_ARG


def test_shapes_and_pointers():
    s = ctypes.c_void_p(0)
    i8, sk, d8 = L().bfpq_hbfp_linear_i8, L().bfpq_hbfp_linear_i8_splitk, L().bfpq_hbfp_linear_decode8
    assert i8(P, P, P, P, Z, P, 16, 16, 192, 2, 7, 7, s) == E_UNSUPPORTED          # K % 256
    assert i8(P, P, P, P, Z, P, 16, 24, 256, 2, 7, 7, s) == E_UNSUPPORTED          # N % 16
    assert i8(Z, P, P, P, Z, P, 16, 16, 256, 2, 7, 7, s) == E_ARG
    assert i8(ctypes.c_void_p(8), P, P, P, Z, P, 16, 16, 256, 2, 7, 7, s) == E_ARG  # codes not 16-byte aligned
    assert i8(P, ctypes.c_void_p(18), P, P, Z, P, 16, 16, 256, 2, 7, 7, s) == E_ARG  # exponents not 4-byte aligned
    assert i8(P, P, P, P, Z, P, 0, 16, 256, 2, 7, 7, s) == 0                        # nothing to do
    assert i8(P, P, P, P, Z, P, -1, 16, 256, 2, 7, 7, s) == E_ARG
    assert sk(P, P, P, P, Z, P, P, 0, 16, 16, 256, 2, 7, 7, s) == E_ARG              # parts
    assert sk(P, P, P, P, Z, P, P, 65, 16, 16, 256, 2, 7, 7, s) == E_ARG
    assert sk(P, P, P, P, Z, P, Z, 2, 16, 16, 256, 2, 7, 7, s) == E_ARG              # slabs
    assert sk(P, P, P, P, Z, P, ctypes.c_void_p(20), 2, 16, 16, 256, 2, 7, 7, s) == E_ARG
    assert d8(P, P, P, P, Z, P, P, 1, 16, 96, 2, 7, 7, s) == E_UNSUPPORTED           # K % 64
    assert d8(P, P, P, P, Z, P, P, 0, 16, 64, 2, 7, 7, s) == E_ARG
    assert d8(P, P, P, P, Z, P, Z, 1, 16, 64, 2, 7, 7, s) == E_ARG
    c4 = L().bfpq_codes4_to_i8
    assert c4(P, P, 12, s) == E_ARG and c4(P, P, -8, s) == E_ARG and c4(Z, P, 8, s) == E_ARG and c4(P, P, 0, s) == 0


def test_python_ok_every_block():
    ok = native.hbfp_linear_i8_ok
    assert ok(1, 4096, 11008, 7, 7) and ok(2048, 11008, 4096, 5, 5) and ok(3, 16, 64, 1, 1)
    assert ok(1, 4096, 4096, 7, 7, block_size=32) and ok(1, 4096, 4096, 7, 7, block_size=16)        # one predicate for every block
    assert not ok(1, 4096, 4096, 8, 7) and not ok(1, 4096, 4096, 7, 0) and not ok(1, 4096, 4096, 7, 7, block_size=48)
    assert not ok(1, 24, 256, 7, 7) and not ok(1, 16, 96, 7, 7)


def test_matrix_unit_values():
    for bad in ('int4', 'INT8', 2, None, 'true'):
        with pytest.raises(ValueError):
            bfp_ops.WeightCache(None, matrix_unit=bad)
        lin = bfp_ops.BFPLinear(256, 16, num_format='bfp', mant_bits=7, block_size=64, rounding_mode='determ')
        with pytest.raises(ValueError):
            lin.enable_weight_cache(matrix_unit=bad)
        with pytest.raises(ValueError):
            patch_linear_layers(torch.nn.Sequential(torch.nn.Linear(256, 16)), dict(num_format='bfp', mant_bits=7, block_size=64),
                                cache_weights=True, matrix_unit=bad)
    assert bfp_ops.WeightCache(None, matrix_unit='int8').matrix_unit == 'int8'
    assert bfp_ops.WeightCache(None, matrix_unit=True).matrix_unit is True
    assert bfp_ops.WeightCache(None, matrix_unit=False).matrix_unit is False
    c = bfp_ops.WeightCache(None, matrix_unit='int8')
    assert c.i8_calls == 0 and c.mx_calls == 0
    m = torch.nn.Sequential(torch.nn.Linear(256, 16))
    patch_linear_layers(m, dict(num_format='bfp', mant_bits=7, block_size=64, rounding_mode='determ'), cache_weights=True, matrix_unit='int8')
    assert m[0]._weight_cache.matrix_unit == 'int8'


def _module8(x_sparsity=None, mant_bits=7):
    pk = bfp_ops.PackedBFP(torch.zeros(32, 256, dtype=torch.int8), torch.zeros(32, 4, dtype=torch.int8), (32, 256), torch.bfloat16, mant_bits, 64, 8)
    return PackedBFPLinear(pk, None, mant_bits, 1e-8, x_sparsity)


def test_packed_linear_code8_extra_state_round_trip():
    spec = native.ActSparsity('structured', 2, 4, 0.0, 's')
    m = _module8(spec, 5)
    sd = m.state_dict()
    other = _module8(None, 7)
    other.load_state_dict(sd)
    st = other.get_extra_state()
    assert st['code_bits'] == 8 and st['mant_bits'] == 5 and other.x_mant_bits == 5 and other.x_sparsity == spec
    assert other.packed.code_bits == 8 and other.packed.mant_bits == 5 and other.codes.dtype == torch.int8


def test_packed_linear_older_state_still_loads():
    """a 4-bit state saved before this change (no x_sparsity key) loads and keeps its 4-bit form"""
    pk = bfp_ops.PackedBFP(torch.zeros(32, 128, dtype=torch.uint8), torch.zeros(32, 4, dtype=torch.int8), (32, 256), torch.bfloat16, 3, 64, 4)
    m = PackedBFPLinear(pk, None, 3, 1e-8, None)
    sd = m.state_dict()
    key = [k for k in sd if k.endswith("_extra_state")][0]
    old = dict(sd[key])
    del old["x_sparsity"]
    sd[key] = old
    fresh = PackedBFPLinear(pk, None, 3, 1e-8, native.ActSparsity('structured', 2, 4, 0.0, 's'))
    fresh.load_state_dict(sd)
    assert fresh.x_sparsity is None and fresh.packed.code_bits == 4 and fresh.packed.mant_bits == 3


def test_from_linear_refusals_stay():
    lin = torch.nn.Linear(256, 32)
    base = dict(num_format='bfp', sparsity_num_format='bfp', block_size=64, rounding_mode='determ')
    with pytest.raises(ValueError):
        PackedBFPLinear.from_linear(lin, dict(base, mant_bits=7, w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='q'))
    with pytest.raises(ValueError):
        PackedBFPLinear.from_linear(lin, dict(base, mant_bits=7, rounding_mode='stoc'))
    with pytest.raises(AssertionError):
        PackedBFPLinear.from_linear(lin, dict(base, mant_bits=8))
