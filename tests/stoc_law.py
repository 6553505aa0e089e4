"""The law of the reference's stochastic rounding ('stoc'), computed exactly -- TEST INFRASTRUCTURE.

The reference (bfp_ops.py:20-44) rounds a block stochastically as
    t = x / interval                      in the tensor's dtype
    r = round_half_even(fl32(u + t))      u = torch.rand(...) - 0.5, fp32: u in {k 2^-24 - 0.5 : 0 <= k < 2^24}
    y = clamp(r * interval, -max_v, max_v) in fp32 (the fp32 dither promotes everything after it)
with the block's exponent e, interval = 2^(e - m) and max_v = 2^e - interval computed in the dtype.  For one element
the output is a monotone function of k, so its distribution is a handful of fp32 bit patterns (at most three: lo, hi
and the signed zero when lo or hi is 0) with probabilities that are counts of k over 2^24.  law() finds the class
boundaries by bisection over k in float32 arithmetic -- no sampling -- for every element of a tensor.

Exponents come from the C oracle (oracle/bfp_oracle.c), whose exponent does not depend on the rounding mode.  Pruning:
  * first == 's': pruned elements are +0 before quantization (torch.where(mask, 0, t)); the dither rounds them to +-0;
  * first == 'q': pruned elements are +0 after quantization.  The q-first mask is taken on the input, so a q-first
    caller must build inputs on which the mask does not depend on the rounding (pruned magnitudes below one
    interval, kept ones at two or more).
NaN outputs are one class, canonical bits 0x7fc00000 (see canon_bits).
"""
import numpy as np
import torch

from oracle import oracle as O

NAN_BITS = np.uint32(0x7fc00000)
KBITS = 24
K = 1 << KBITS                  # dither values of the reference: torch.rand's 24-bit grid
HOT_DITHER_RES = 2.0 ** -16     # the engine's hot loop draws 16-bit dithers: each class probability may differ by this


def _rnd(a, dtype):
    """float32 array -> nearest value of `dtype` (round half to even), as float32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == torch.float32:
        return a
    return torch.from_numpy(a).to(dtype).float().numpy()


def canon_bits(y):
    """fp32 bit patterns of a float32 array / tensor, every NaN as 0x7fc00000"""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().float().numpy()
    y = np.ascontiguousarray(y, dtype=np.float32)
    b = y.view(np.uint32).copy()
    b[np.isnan(y)] = NAN_BITS
    return b


def _order_key(bits):
    """total order of fp32 bit patterns by value, -0 < +0 (monotone in the value for non-NaN patterns)"""
    bits = bits.astype(np.uint64)
    neg = (bits >> np.uint64(31)) != 0
    return np.where(neg, np.uint64(0xffffffff) - bits, bits | np.uint64(0x80000000))


def _outcome(t, interval, max_v, k):
    """output bits for dither index k (arrays of one shape; float32 arithmetic, as the reference's fp32 ops)"""
    with np.errstate(invalid='ignore', over='ignore'):
        u = (k.astype(np.float64) * 2.0 ** -KBITS - 0.5).astype(np.float32)          # exact
        s = (u + t).astype(np.float32)                                                # one fp32 rounding
        r = np.rint(s).astype(np.float32)                                             # half to even, keeps the sign of 0
        y = (r * interval).astype(np.float32)
        y = np.where(np.isnan(y) | np.isnan(max_v), np.float32(np.nan), y)
        y = np.where(y < -max_v, -max_v, y)                                           # torch.max(y, -max_v)
        y = np.where(y > max_v, max_v, y).astype(np.float32)                          # torch.min(y, max_v)
    return canon_bits(y)


def block_scale(xs2, block_size, mant_bits, epsilon):
    """per element of the 2-D (pruned) input: (t, interval, max_v) as float32 arrays, computed in the dtype"""
    dtype = xs2.dtype
    rows, cols = xs2.shape
    _, exps = O.no_sparsity_float_to_bfp(xs2, block_size, mant_bits, epsilon, return_exponents=True)
    e = np.repeat(exps.numpy().astype(np.float32), block_size, axis=1)[:, :cols]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        em = _rnd(e - np.float32(mant_bits), dtype)
        interval = _rnd(np.power(np.float32(2.0), em, dtype=np.float32), dtype)
        p2e = _rnd(np.power(np.float32(2.0), e, dtype=np.float32), dtype)
        max_v = _rnd(p2e - interval, dtype)
        t = _rnd(xs2.float().numpy() / interval, dtype)
    return t, interval, max_v


def law(x, block_size, mant_bits, epsilon=1e-8, N=0, M=0, first='s', mask=None):
    """The distribution of the reference's 'stoc' output for every element of the CPU tensor x.
    mask: bool tensor of x's shape, True where the element is pruned (None: no pruning; with 0 < N < M and no mask,
    the N:M mask the C oracle picks on x).  Returns (bits [n, 3] uint32, probs [n, 3] float64, ncls [n] int) over the
    flattened x: per element its candidate fp32 patterns in increasing order and their probabilities (unused slots 0)."""
    x = x.detach().cpu().contiguous()
    cols = x.shape[-1] if x.dim() else 1
    x2 = x.view(-1, cols)
    if mask is None and 0 < N < M:
        pruned = O.structured_N_M_sparsity(x2, N, M)
        mask = (pruned == 0) & (x2 != 0)
    m2 = None if mask is None else mask.cpu().reshape(x2.shape).bool()
    xs2 = torch.where(m2, torch.zeros((), dtype=x.dtype), x2) if (m2 is not None and first == 's') else x2
    t, interval, max_v = (a.reshape(-1) for a in block_scale(xs2, block_size, mant_bits, epsilon))
    n = t.size
    bits = np.zeros((n, 3), np.uint32)
    probs = np.zeros((n, 3), np.float64)
    ncls = np.zeros(n, np.int64)
    lo_k = np.zeros(n, np.int64)
    last = _outcome(t, interval, max_v, np.full(n, K - 1, np.int64))
    cur = _outcome(t, interval, max_v, lo_k)
    active = np.ones(n, bool)
    for c in range(3):
        bits[active, c] = cur[active]
        ncls[active] += 1
        done = active & (_order_key(cur) == _order_key(last))
        probs[done, c] = (K - lo_k[done]) / K
        active &= ~done
        if not active.any():
            break
        assert c < 2, "more than three outcome classes"
        # first k whose outcome orders above cur: bisection on (lo, hi]
        lo, hi = lo_k.copy(), np.full(n, K - 1, np.int64)
        ck = _order_key(cur)
        while True:
            open_ = active & (hi - lo > 1)
            if not open_.any():
                break
            mid = (lo + hi) // 2
            above = _order_key(_outcome(t, interval, max_v, mid)) > ck
            hi = np.where(open_ & above, mid, hi)
            lo = np.where(open_ & ~above, mid, lo)
        probs[active, c] = (hi[active] - lo_k[active]) / K
        lo_k = np.where(active, hi, lo_k)
        cur = np.where(active, _outcome(t, interval, max_v, lo_k), cur)
    if m2 is not None and first != 's':                                              # q-first: pruned after Q -> +0
        pm = m2.reshape(-1).numpy()
        bits[pm] = 0
        probs[pm] = 0.0
        probs[pm, 0] = 1.0
        ncls[pm] = 1
    return bits, probs, ncls


def class_index(bits_out, law_bits, ncls):
    """index of each output pattern in its element's support, -1 where it is not in the support"""
    idx = np.full(bits_out.shape, -1, np.int64)
    for c in range(3):
        hit = (law_bits[:, c] == bits_out) & (c < ncls) & (idx < 0)
        idx[hit] = c
    return idx


def binom_tol(p, n, extra=0.0):
    """6 sigma of a frequency over n draws, plus 1/n and an allowed systematic offset `extra`: the true probability may lie
    anywhere in p +- extra, so sigma is taken at the point of that band nearest 1/2"""
    p = np.asarray(p, np.float64)
    pe = np.clip(0.5, p - extra, p + extra)
    return 6.0 * np.sqrt(pe * (1.0 - pe) / n) + 1.0 / n + extra


def class_rows(dtype, mant_bits, block_size=16, seed=0):
    """[rows, block_size] rows of `dtype` built to hit every outcome class of the law: per block one maximum (1.0, which
    rounds past qmax and is clamped, or 7.5 / 8 of it) and elements (j + f) * interval for fractions f in k/8, 2^-16 and
    1 - 2^-16 (where the dtype holds them), on-grid codes, +0 and -0, both signs; a subnormal-scale block; for fp16 a block
    whose 2^e overflows (max near 65504).  mant_bits is the one the rows are meant for (interval = 2^-mant_bits)."""
    g = torch.Generator().manual_seed(seed)
    iv = 2.0 ** -mant_bits
    qmax = 2 ** mant_bits - 1
    fr = [k / 8 for k in range(8)] + [2.0 ** -16, 1 - 2.0 ** -16]
    vals = []
    for j in (0, 1, 2, min(5, qmax - 1), max(qmax - 1, 0)):
        for f in fr:
            vals += [(j + f) * iv, -(j + f) * iv]
    vals += [0.0, -0.0]
    out = []
    for b in range(0, len(vals), block_size - 1):
        chunk = vals[b:b + block_size - 1]
        top = 1.0 if (b // (block_size - 1)) % 2 == 0 else (qmax + 0.5) * iv
        row = [top] + chunk + [0.0] * (block_size - 1 - len(chunk))
        out.append(row)
    rows = torch.tensor(out, dtype=torch.float64)
    rnd_row = torch.randn(2, block_size, generator=g, dtype=torch.float64)
    rnd_row[:, 0] = 0.0
    rnd_row[:, 1] = -0.0
    sub = rnd_row.clone()
    scale = {torch.float32: 2.0 ** -140, torch.float16: 2.0 ** -20, torch.bfloat16: 2.0 ** -132}[dtype]
    sub = sub * scale
    rows = torch.cat([rows, rnd_row, sub], 0)
    if dtype == torch.float16:
        big = torch.tensor([[60000.0, 65504.0, -65504.0, 40000.0, -33000.0, 1.0, -0.0, 0.0] * (block_size // 8)], dtype=torch.float64)
        rows = torch.cat([rows, big], 0)
    return rows.to(dtype)
