"""The sweep skeleton of the fused quantize kernel at its edges (csrc/bfpq_fused.h, the packed-output sweep): 0, 1 and 2 full sweeps
left over by the three-way unrolled loop (0 and 1 by the drop-in sweep's two-way one), a last sweep that is exactly full, a ragged last sweep whose last workgroup has waves wholly
in range, one straddling the end and waves wholly past it, a tensor smaller than one sweep and one of a single chunk.  These loops only
exist when a tensor has more chunks of 256 lane items than the grid cap, so the shapes are far larger than the rest of the suite's
(cols = 64, up to 34 MB); grid_for_cap is restated here and the shapes are checked to reach every one of those paths.

Expected values come from the C oracle, bit for bit: the drop-in tensor, and for the packed form the 4-bit codes and the exponent bytes
derived from the oracle's dequantised values and block exponents (codes of a NaN block are "don't care": there the marker byte -128 is
checked, and the codes against the general instantiation's)."""
import functools

import numpy as np
import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from util import DT, bits, assert_bits_equal
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLS, BLOCK, MANT = 64, 64, 3
THREADS, VEC = 256, 8                       # a workgroup's lane items per sweep; elements of a 16-bit dtype per lane item
CAP_DROPIN, CAP_PACKED, CAP_MX8 = 1024, 2752, 2752   # kMaxGrid, grid_for_packed, launch_fused_mx8 (csrc/bfpq_device.h, bfpq_fused.h)


def grid_for_cap(n_items, cap):
    """csrc/bfpq_device.h: workgroups for n_items lane items, balanced over the sweeps"""
    g = max(1, (n_items + THREADS - 1) // THREADS)
    if g <= cap:
        return g
    sweeps = (g + cap - 1) // cap
    return (g + sweeps - 1) // sweeps


def sweep_shape(rows, cap):
    n = rows * COLS // VEC
    grid = grid_for_cap(n, cap)
    stride = grid * THREADS
    return dict(n=n, chunks=(n + THREADS - 1) // THREADS, grid=grid, full=n // stride, total=(n + stride - 1) // stride, ragged=n % THREADS)


# rows (x 64 columns): 32 rows are one chunk; "+ 12" leaves 96 lane items in the last chunk -- wave 0 whole, wave 1 half, waves 2 and 3 out
MULTI = [96012, 196716, 265580]             # 3001 / 6148 / 8300 chunks: 2, 3, 4 sweeps of the packed grid; full sweeps 1, 2, 3
EXACT = 176128                              # 5504 chunks = 2 sweeps x 2752 workgroups, nothing ragged
SMALL = [32012, 12]                         # less than one sweep (1001 chunks); a single chunk
DROPIN = [111980, 98304]                    # the drop-in grid (two-way unrolled): 3500 chunks = 3 full sweeps + a ragged one; 3072 = 3 x 1024 exactly
SHAPES = MULTI + [EXACT] + SMALL + DROPIN


def test_the_shapes_reach_every_path_of_the_sweep():
    multi = [sweep_shape(r, CAP_PACKED) for r in MULTI]
    assert {s["full"] % 3 for s in multi} == {0, 1, 2}
    assert all(2 <= s["total"] <= 5 and s["chunks"] > CAP_PACKED and s["n"] * 16 <= 40e6 for s in multi)
    assert all(s["total"] == s["full"] + 1 for s in multi)                      # each ends in a ragged sweep ...
    assert all(s["ragged"] % 64 != 0 and 64 < s["ragged"] < 192 for s in multi)  # ... whose last chunk: whole / straddling / empty waves
    e = sweep_shape(EXACT, CAP_PACKED)
    assert e["total"] == e["full"] >= 2 and e["ragged"] == 0 and e["chunks"] == e["full"] * e["grid"]
    s = sweep_shape(SMALL[0], CAP_PACKED)
    assert s["full"] == 0 and s["total"] == 1 and 1 < s["chunks"] < CAP_PACKED and s["ragged"] % 64 != 0
    assert sweep_shape(SMALL[1], CAP_PACKED)["chunks"] == 1
    m = sweep_shape(MULTI[1], CAP_MX8)
    assert m["chunks"] > CAP_MX8 and m["total"] >= 2
    # the drop-in sweep (unrolled by two): 0 and 1 full sweeps left over in front of a ragged one, and one left over with nothing ragged
    d = [sweep_shape(r, CAP_DROPIN) for r in MULTI + DROPIN[:1]]
    assert all(s["total"] == s["full"] + 1 and s["ragged"] % 64 != 0 for s in d) and {s["full"] % 2 for s in d} == {0, 1}
    x = sweep_shape(DROPIN[1], CAP_DROPIN)
    assert x["total"] == x["full"] and x["full"] % 2 == 1 and x["ragged"] == 0 and x["chunks"] == x["full"] * x["grid"]


def special_rows(rows):
    """(power-of-two block maximum, NaN) row pairs inside the last sweep of the packed grid: in its first chunk, and in the last chunk's
    whole wave and straddling wave (rows of 8 lane items: wave w of the last chunk holds its rows 8 w .. 8 w + 7)"""
    s = sweep_shape(rows, CAP_PACKED)
    first = (s["total"] - 1) * s["grid"] * THREADS * VEC // COLS             # first row of the last sweep
    last_chunk = (s["chunks"] - 1) * THREADS * VEC // COLS
    pairs = {(first + 3, first + 5), (last_chunk + 1, last_chunk + 6)}
    if s["ragged"] > 64:
        pairs.add((last_chunk + 8, min(last_chunk + 10, rows - 1)))
    return sorted((p, q) for p, q in pairs if p < rows and q < rows and p != q)


@functools.lru_cache(maxsize=None)
def inputs(dname, rows, special):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, COLS, generator=g) * 0.02).to(DT[dname])
    if special:
        for p, q in special_rows(rows):
            x[p, :] = x[p, :].clamp(-0.03, 0.03)
            x[p, 17] = 0.0625                                    # the block maximum is a power of two
            x[q, 40] = float("nan")
    return x


@functools.lru_cache(maxsize=None)
def reference(dname, rows, special, sparse):
    """(dequantised tensor, block exponents) from the oracle; computed once per input and left alone"""
    x = inputs(dname, rows, special)
    want = O.float_to_bfp_blocked(x, mant_bits=MANT, epsilon=1e-8, rounding_mode='determ', device='cpu', block_size=BLOCK, num_format='bfp',
                                  weight_mant_bits=15, in_sparsity=False, w_sparsity=sparse, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4,
                                  sparsity_num_format='bfp', first='s', sparsity_mode='structured', identifier='w')
    pruned = O.structured_N_M_sparsity(x, 2, 4).view(x.shape) if sparse else x
    again, e = O.no_sparsity_float_to_bfp(pruned, BLOCK, MANT, 1e-8, return_exponents=True)
    assert_bits_equal(bits(again), bits(want), DT[dname], "oracle, two steps")
    return want, e.view(rows)


def expected_packed(want, e):
    """4-bit codes (two per byte, low nibble first) and exponent bytes of the oracle's result; nan = rows the reference turns into NaN"""
    nan = torch.isnan(e)
    es = torch.nan_to_num(e, nan=0.0).clamp(-127, 127)
    q = want.double() / torch.exp2(es.double() - MANT).unsqueeze(1)
    q = torch.nan_to_num(q, nan=0.0)
    assert torch.equal(q, q.round()) and float(q.abs().max()) <= (1 << MANT) - 1
    n = (q.to(torch.int16) & 0xF).to(torch.uint8)
    codes = n[:, 0::2] | (n[:, 1::2] << 4)
    exps = torch.where(nan, torch.full_like(es, -128.0), es).to(torch.int8).view(-1, 1)
    return codes, exps, nan


def check_packed(dname, rows, special, sparse):
    x = inputs(dname, rows, special).to(DEV)
    want, e = reference(dname, rows, special, sparse)
    nm = dict(N=2, M=4, first='s') if sparse else {}
    codes, exps = bfp_ops.float_to_bfp_packed(x, MANT, BLOCK, code_bits=4, **nm)
    wc, we, nan = expected_packed(want, e)
    assert bool(nan.any()) == bool(special)
    assert torch.equal(exps.cpu(), we), "exponent bytes"
    c = codes.cpu()
    assert torch.equal(c[~nan], wc[~nan]), "codes"
    if special:                                   # the NaN blocks' codes: whatever the general instantiation (drop-in sweep) writes
        c2, e2, _ = bfp_ops.float_to_bfp_packed(x, MANT, BLOCK, code_bits=4, with_dequant=True, **nm)
        assert torch.equal(c2, codes) and torch.equal(e2, exps)


@pytest.mark.parametrize("rows", SHAPES)
@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_packed_24_at_the_sweep_edges(dname, rows):
    check_packed(dname, rows, False, True)


@pytest.mark.parametrize("rows", SHAPES)
@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_dropin_24_at_the_sweep_edges(dname, rows):
    x = inputs(dname, rows, False).to(DEV)
    want, _ = reference(dname, rows, False, True)
    got = bfp_ops.float_to_bfp_blocked(x, mant_bits=MANT, epsilon=1e-8, rounding_mode='determ', device='cuda', block_size=BLOCK,
                                       num_format='bfp', weight_mant_bits=15, in_sparsity=False, w_sparsity=True, grad_sparsity=False,
                                       sparsity_frac=0.5, N=2, M=4, sparsity_num_format='bfp', first='s', sparsity_mode='structured',
                                       identifier='w')
    assert_bits_equal(bits(got), bits(want), DT[dname], "drop-in")


def test_packed_dense_at_the_sweep_edges():
    check_packed("bf16", MULTI[1], False, False)


@pytest.mark.parametrize("rows", MULTI + [EXACT, SMALL[1]])
@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_cold_tier_in_the_last_sweep(dname, rows):
    """a power-of-two block maximum and a NaN in the last sweep: in a workgroup wholly in range, and in the last chunk's whole wave and its
    straddling wave"""
    assert special_rows(rows)
    check_packed(dname, rows, True, True)


def test_mx8_image_at_a_multi_sweep_size():
    """bfpq_quantize_mx8 runs the same sweep (PACK == 8): its e4m3 bytes and E8M0 scales decode to the oracle's values"""
    rows = MULTI[1]
    x = inputs("bf16", rows, False).to(DEV)
    want, e = reference("bf16", rows, False, False)
    x8, xs = native.quantize_mx8(x, MANT)
    e4 = np.zeros(256, dtype=np.float64)
    for m, byte in enumerate([0, 0x38, 0x40, 0x44, 0x48, 0x4a, 0x4c, 0x4e]):
        e4[byte] = m
        e4[byte | 0x80] = -m
    assert torch.equal(xs.cpu().view(-1).to(torch.float32), e - MANT + 127), "E8M0 scales"
    val = torch.from_numpy(e4[x8.cpu().numpy()]) * torch.exp2(xs.cpu().double() - 127)
    assert torch.equal(val, want.double())
    known = np.isin(x8.cpu().numpy(), np.flatnonzero(e4 != 0).tolist() + [0, 0x80])
    assert known.all()
