"""Pruned activations on the packed / matrix-unit paths, host side: argument validation of the two image entry points (no launch
happens for a rejected call) and the activation spec's round trip through PackedBFPLinear's extra state."""
import ctypes

import pytest
import torch

import quantization_sparsity_interplay_amd as pkg
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import PackedBFPLinear


def test_quantize_mx8_nm_argument_validation():
    L = pkg.load_library()
    n = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)               # a non-null, never dereferenced pointer: rejected before any launch
    f = L.bfpq_quantize_mx8_nm
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 0, 4, 1, one, one, n) == -1       # N = 0
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 5, 4, 1, one, one, n) == -1       # N > M
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 2, 0, 1, one, one, n) == -1       # M = 0
    assert f(one, one, one, 4, 64, native.BF16, 0, 1e-8, 2, 4, 1, one, one, n) == -1       # mant_bits 0
    assert f(one, one, one, 4, 64, native.BF16, 5, 1e-8, 2, 4, 1, one, one, n) == -1       # 5 mantissa bits do not fit e4m3
    assert f(one, one, one, 4, 64, 9, 3, 1e-8, 2, 4, 1, one, one, n) == -1                 # bad dtype
    assert f(n, one, one, 4, 64, native.BF16, 3, 1e-8, 2, 4, 1, one, one, n) == -1         # null input
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 2, 4, 1, n, one, n) == -1         # no exponent table
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 2, 4, 1, one, n, n) == -1         # N:4 without its table
    assert f(one, one, one, 4, 100, native.BF16, 3, 1e-8, 2, 4, 1, one, one, n) == -2      # cols % 64: through the codes
    assert f(one, one, one, 4, 96, native.F32, 3, 1e-8, 1, 2, 0, one, n, n) == -2          # cols % 64, fp32
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 3, 16, 1, one, n, n) == -2        # an M the one-pass kernel does not take
    assert f(one, one, one, 4, 64, native.BF16, 3, 1e-8, 2, 65, 1, one, n, n) == -2        # M > 64
    assert f(ctypes.c_void_p(8), one, one, 4, 64, native.BF16, 3, 1e-8, 2, 4, 1, one, one, n) == -2   # input not 16-byte aligned
    assert f(one, one, one, 0, 64, native.BF16, 3, 1e-8, 2, 4, 1, one, one, n) == 0        # empty tensor: ok, no launch
    assert f(one, one, one, 4, 0, native.F16, 3, 1e-8, 1, 8, 0, one, n, n) == 0


def test_quantize_threshold_mx8_argument_validation():
    L = pkg.load_library()
    n = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    f = L.bfpq_quantize_threshold_mx8
    far, far2 = ctypes.c_void_p(1 << 40), ctypes.c_void_p((1 << 40) + (1 << 20))
    assert f(one, far, far2, 4, 64, native.BF16, 0, 1e-8, one, one, n) == -1                # mant_bits 0
    assert f(one, far, far2, 4, 64, native.BF16, 5, 1e-8, one, one, n) == -1                # mant_bits 5
    assert f(one, far, far2, 4, 64, 3, 3, 1e-8, one, one, n) == -1                          # bad dtype
    assert f(one, far, far2, 4, 64, native.BF16, 3, 1e-8, one, n, n) == -1                  # no workspace
    assert f(one, far, far2, 4, 64, native.BF16, 3, 1e-8, n, one, n) == -1                  # no exponent table
    assert f(n, far, far2, 4, 64, native.BF16, 3, 1e-8, one, one, n) == -1                  # null input
    # the cut-segment workgroups re-read the input: an output that overlaps it is refused
    assert f(one, one, far2, 4, 64, native.BF16, 3, 1e-8, one, one, n) == -1                # image == input
    assert f(one, far, one, 4, 64, native.BF16, 3, 1e-8, one, one, n) == -1                 # scales == input
    assert f(one, ctypes.c_void_p(16 + 256), far2, 4, 64, native.BF16, 3, 1e-8, one, one, n) == -1   # image inside the input
    assert f(one, far, far2, 4, 100, native.BF16, 3, 1e-8, one, one, n) == -2               # cols % 64: through the codes
    assert f(ctypes.c_void_p(24), far, far2, 4, 64, native.BF16, 3, 1e-8, one, one, n) == -2   # input not 16-byte aligned
    assert f(one, far, far2, 0, 64, native.BF16, 3, 1e-8, one, one, n) == 0                 # empty tensor: ok, no launch


def test_new_entries_are_exported():
    assert {"bfpq_quantize_mx8_nm", "bfpq_quantize_threshold_mx8"} <= set(native.EXPORTED_SYMBOLS)
    assert pkg.load_library().bfpq_version() == 4


def test_act_sparsity_spec():
    A = native.ActSparsity
    base = pkg.BFPConfig.hbfp(4, 64).to_kwargs()
    assert A.from_bfp_args(bfp_ops.unpack_bfp_args(dict(base))) is None
    s24 = A.from_bfp_args(dict(base, in_sparsity=True, sparsity_mode='structured', N=2, M=4, first='q'))
    assert s24 == A('structured', 2, 4, 0.0, 'q')
    assert A.from_bfp_args(dict(base, in_sparsity=True, sparsity_mode='structured', N=4, M=4)) is None      # N == M keeps everything
    u = A.from_bfp_args(dict(base, in_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='s'))
    assert u == A('unstructured', 0, 0, 0.5, 's')
    assert A.from_bfp_args(dict(base, in_sparsity=False, w_sparsity=True, sparsity_mode='structured', N=2, M=4)) is None
    with pytest.raises(ValueError):
        A.from_bfp_args(dict(base, in_sparsity=True, sparsity_mode='blocky'))
    assert len({s24, A('structured', 2, 4, 0.0, 'q'), u}) == 2                                              # hashable, by value
    assert A.from_dict(u.as_dict()) == u and A.from_dict(None) is None
    # the reference prunes first only for first == 's' (bfp_ops.py:141-149): any other value quantizes first
    for mode in ('structured', 'unstructured'):
        for first, want in (('s', 's'), ('q', 'q'), ('x', 'q'), ('', 'q')):
            got = A.from_bfp_args(dict(base, in_sparsity=True, sparsity_mode=mode, N=2, M=4, sparsity_frac=0.5, first=first))
            assert got.first == want, (mode, first)


def _module(x_sparsity):
    """a PackedBFPLinear made from CPU-side metadata (codes / exponents as CPU tensors: nothing is launched)"""
    pk = bfp_ops.PackedBFP(torch.zeros(32, 128, dtype=torch.uint8), torch.zeros(32, 4, dtype=torch.int8), (32, 256), torch.bfloat16, 3, 64, 4)
    return PackedBFPLinear(pk, None, 3, 1e-8, x_sparsity)


def test_packed_linear_extra_state_round_trip():
    spec = native.ActSparsity('unstructured', 0, 0, 0.5, 'q')
    m = _module(spec)
    sd = m.state_dict()
    other = _module(None)
    other.load_state_dict(sd)
    assert other.x_sparsity == spec
    assert "x_sparsity" in repr(other)
    nm = _module(native.ActSparsity('structured', 2, 4, 0.0, 's'))
    other.load_state_dict(nm.state_dict())
    assert other.x_sparsity == native.ActSparsity('structured', 2, 4, 0.0, 's')


def test_packed_linear_loads_a_state_without_the_activation_keys():
    """a state dict saved before activation pruning existed has no x_sparsity: it loads as dense activations"""
    m = _module(native.ActSparsity('structured', 2, 4, 0.0, 's'))
    sd = m.state_dict()
    key = [k for k in sd if k.endswith("_extra_state")][0]
    old = dict(sd[key])
    del old["x_sparsity"]
    sd[key] = old
    m.load_state_dict(sd)
    assert m.x_sparsity is None
