"""The host restatement of the unstructured contract (tests/unstructured_ref.py) checked against the C oracle and against the
reference's own output (G5), so that the GPU tests that compare the engine with it cannot merely agree with a wrong helper.
The oracle prunes ties in its introselect's order and the helper lowest flat index first (the documented divergence), so the
two must agree on the threshold, on the count and on every element outside the tie class."""
import numpy as np
import pytest
import torch

from util import DT, load, from_bits, bits
from gen import int_bits_tensor
from oracle import oracle as O
from unstructured_ref import (flat_order_prune, flat_order_threshold, mag_keys, special_values, SPECIAL_KINDS, SPECIAL_LAYOUTS,
                              NAN_BITS, SUBNORMAL_BITS, INF_BITS, SIGN_BIT)


def _key_value(tau, dt):
    """the float magnitude a key stands for (NaN for the NaN class)"""
    inf = INF_BITS[dt]
    if tau > inf:
        return float("nan")
    return float(from_bits(np.array([tau]), dt).float()[0])


def _agree_with_oracle(xc, frac, what):
    dt = xc.dtype
    got = flat_order_prune(xc, frac)
    want, tau_o, k_o = O.unstructured_sparsity(xc, frac, return_stats=True)
    k, tau, need = flat_order_threshold(xc, frac)
    assert k == k_o, (what, k, k_o)
    keys = mag_keys(xc)
    if k == 0:
        assert np.array_equal(bits(got), bits(xc)) and np.array_equal(bits(want), bits(xc)), what
        return
    tv = _key_value(tau, dt)
    assert (tv == tau_o) or (tv != tv and tau_o != tau_o), (what, tv, tau_o)
    gz, wz = (got.view(-1) == 0).numpy(), (want.view(-1) == 0).numpy()
    assert int(gz.sum()) == int(wz.sum()), (what, int(gz.sum()), int(wz.sum()))                  # same pruned count
    outside = keys != tau
    assert np.array_equal(bits(got).reshape(-1)[outside], bits(want).reshape(-1)[outside]), what + " (outside the tie class)"
    assert int((keys < tau).sum()) + need == k, what
    tie = np.flatnonzero(~outside)
    pruned = bits(got).reshape(-1)[tie] == 0                                                     # +0.0: pruned (or a +0.0 kept)
    assert pruned[:need].all(), what                                                             # the first `need` ties in flat order
    if tau != 0:
        assert not pruned[need:].any(), what


@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
def test_hand_example(dname):
    """a tensor small enough to prune by hand: all NaNs are one class above +inf, -0.0 and +0.0 are one key, ties go lowest flat index first"""
    dt = DT[dname]
    nan, ninf = NAN_BITS[dt], INF_BITS[dt]
    neg = SIGN_BIT[dt]
    sub = SUBNORMAL_BITS[dt][2]
    one = int(bits(torch.tensor([1.0], dtype=dt))[0])
    x = np.array([one, neg, sub | neg, 0, nan[2], one | neg, nan[1], ninf, sub, ninf | neg, one], dtype=np.uint32)
    xc = from_bits(x, dt)
    z = 0
    cases = {
        1: [one, z, sub | neg, 0, nan[2], one | neg, nan[1], ninf, sub, ninf | neg, one],                 # first zero (-0.0) -> +0.0
        3: [one, z, z, 0, nan[2], one | neg, nan[1], ninf, sub, ninf | neg, one],                         # zeros, then first subnormal
        5: [z, z, z, 0, nan[2], one | neg, nan[1], ninf, z, ninf | neg, one],                             # first 1.0 (index 0)
        8: [z, z, z, 0, nan[2], z, nan[1], z, z, ninf | neg, z],                                          # first inf (index 7)
        10: [z, z, z, 0, z, z, nan[1], z, z, z, z],                                                       # first NaN (index 4)
        11: [z] * 11,
    }
    for k, want in cases.items():
        got = flat_order_prune(xc, (k + 0.5) / x.size)
        assert np.array_equal(bits(got), np.array(want, dtype=bits(got).dtype)), (dname, k, [hex(v) for v in bits(got)])
        _agree_with_oracle(xc, (k + 0.5) / x.size, f"hand {dname} k={k}")


@pytest.mark.parametrize("layout", SPECIAL_LAYOUTS)
@pytest.mark.parametrize("kind", SPECIAL_KINDS)
@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
def test_special_values_against_oracle(dname, kind, layout):
    """NaNs of several payloads and signs, +-inf, +-0 and subnormals of the dtype, the threshold in each of their classes"""
    dt = DT[dname]
    xc, frac = special_values((256, 512), dt, kind, layout, seed=3)
    k, tau, _ = flat_order_threshold(xc, frac)
    cls = {"zero": tau == 0, "subnormal": 0 < tau < (0x800000 if dname == "f32" else 0x80 if dname == "bf16" else 0x400),
           "inf": tau == INF_BITS[dt], "nan": tau == INF_BITS[dt] + 1}[kind]
    assert cls, (dname, kind, layout, hex(tau))                                                  # the case is the one it names
    _agree_with_oracle(xc, frac, f"special {dname} {kind} {layout} frac={frac}")


@pytest.mark.parametrize("count", ["0", "1", "numel-1", "numel"])
@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
def test_extreme_counts_against_oracle(dname, count):
    dt = DT[dname]
    for kind in ("nan", "zero"):
        xc, _ = special_values((64, 96), dt, kind, "spread", seed=4)
        n = xc.numel()
        k = {"0": 0, "1": 1, "numel-1": n - 1, "numel": n}[count]
        frac = 1.0 if k == n else (k + 0.5) / n
        assert int(n * frac) == k
        _agree_with_oracle(xc, frac, f"extreme {dname} {kind} k={count}")


def test_g5_fixture():
    """the reference's own output: same pruned count, same elements outside the tie class"""
    g = load("g5_unstructured.npz")
    xc = from_bits(g["small_in"], torch.bfloat16).view(64, 256)
    for frac in (0.5, 0.25, 0.9, 0.001):
        got = flat_order_prune(xc, frac)
        want = g[f"small_out_{frac}"].reshape(-1)
        _, tau, _ = flat_order_threshold(xc, frac)
        outside = mag_keys(xc) != tau
        assert int((got.view(-1) == 0).sum()) == int((from_bits(want, torch.bfloat16) == 0).sum()), frac
        assert np.array_equal(bits(got).reshape(-1)[outside], want[outside]), frac
        _agree_with_oracle(xc, frac, f"g5 small {frac}")
    for dname, shape, seed in (("bf16", (512, 1024), 11), ("f16", (256, 512), 12), ("f32", (256, 512), 13)):
        xc = from_bits(int_bits_tensor(shape, dname, seed), DT[dname]).view(shape)
        got = flat_order_prune(xc, 0.5)
        ref_zero = np.unpackbits(g[f"big_zero_{dname}"])[: xc.numel()].astype(bool)
        _, tau, _ = flat_order_threshold(xc, 0.5)
        outside = mag_keys(xc) != tau
        gz = (got.view(-1) == 0).numpy()
        assert int(gz.sum()) == int(ref_zero.sum()), dname
        assert np.array_equal(gz[outside], ref_zero[outside]), dname
        _agree_with_oracle(xc, 0.5, f"g5 big {dname}")
