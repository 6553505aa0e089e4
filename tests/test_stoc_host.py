"""CPU pin of the stochastic-rounding law (tests/stoc_law.py) to the reference's own op sequence: the pure-torch
restatement (oracle/torch_restatement.py) with its 'stoc' branch draws torch.rand on the CPU generator; every draw must
lie in the law's support and every class frequency must sit within a binomial bound of the law's probability."""
import numpy as np
import pytest
import torch

import stoc_law as SL
from oracle import torch_restatement as R

DRAWS = 2000


def _draws(x, block_size, mant_bits, seed):
    torch.manual_seed(seed)
    return np.stack([SL.canon_bits(R.hbfp(x, block_size, mant_bits, 1e-8, 'stoc')).reshape(-1) for _ in range(DRAWS)])


def _check_against_law(x, block_size, mant_bits, seed):
    bits, probs, ncls = SL.law(x, block_size, mant_bits)
    d = _draws(x, block_size, mant_bits, seed)
    idx = np.stack([SL.class_index(row, bits, ncls) for row in d])
    bad = np.argwhere(idx < 0)
    assert bad.size == 0, (f"{bad.shape[0]} draws outside the law's support; first: element {bad[0][1]}, "
                           f"x = {x.reshape(-1)[bad[0][1]].item()!r}, got bits {d[bad[0][0], bad[0][1]]:#010x}, "
                           f"support {[hex(b) for b in bits[bad[0][1], :ncls[bad[0][1]]]]}")
    for c in range(3):
        freq = (idx == c).mean(0)
        tol = SL.binom_tol(probs[:, c], DRAWS)
        off = np.abs(freq - probs[:, c]) > tol
        assert not off.any(), (f"class {c}: element {np.argmax(off)} x = {x.reshape(-1)[np.argmax(off)].item()!r} "
                               f"frequency {freq[np.argmax(off)]} against {probs[np.argmax(off), c]}")
    return bits, probs, ncls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("mant_bits", [3, 7])
def test_law_matches_reference_op_sequence(dtype, mant_bits):
    x = SL.class_rows(dtype, mant_bits)
    bits, probs, ncls = _check_against_law(x, 16, mant_bits, seed=11 + mant_bits)
    assert np.allclose(probs.sum(1), 1.0)
    assert (ncls == 3).any() and (ncls == 1).any()                  # both signed zeros and on-grid values occur


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_law_mant_bits_above_the_dtype_significand(dtype):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(8, 16, generator=g) * torch.exp2(-torch.randint(0, 14, (8, 16), generator=g).double())).to(dtype)
    bits, probs, ncls = _check_against_law(x, 16, 15, seed=5)
    # small elements of a block have codes with a fraction (two or three classes)
    assert (ncls > 1).any()


def test_law_fp16_block_whose_power_of_two_overflows():
    """max 60000, mant_bits 3: e = 16, 2^16 is inf in fp16, so max_v = inf and nothing clamps; the fp32 result is 57344 or
    65536 -- the law (and the reference) return 65536.0, not +inf"""
    x = torch.tensor([[60000.0, 1.0, -0.0, 0.0] * 4], dtype=torch.float16)
    bits, probs, ncls = _check_against_law(x, 16, 3, seed=2)
    vals = bits[0, :ncls[0]].view(np.float32)
    assert sorted(vals.tolist()) == [57344.0, 65536.0]
    assert abs(probs[0, 1] - (60000 / 8192 - 7)) < 1e-3


def test_law_signed_zeros_and_pruned_elements():
    x = torch.tensor([[0.75, 0.0, -0.0, 0.3, -0.3, 0.5, -0.5, 0.6]], dtype=torch.bfloat16)
    mask = torch.tensor([[False, False, False, True, True, False, False, True]])
    b, p, n = SL.law(x, 8, 3, mask=mask, first='s')
    for i in (1, 2, 3, 4, 7):                         # zeros and s-first pruned elements: +-0, one half each
        assert n[i] == 2 and set(b[i, :2].tolist()) == {0x80000000, 0}
        assert abs(p[i, 0] - 0.5) < 1e-6
    bq, pq, nq = SL.law(x, 8, 3, mask=mask, first='q')
    for i in (3, 4, 7):                               # q-first pruned: always +0
        assert nq[i] == 1 and bq[i, 0] == 0 and pq[i, 0] == 1.0
    assert nq[1] == 2 and nq[2] == 2                  # a kept zero still rounds to +-0
