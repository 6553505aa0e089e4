"""The unstructured pruning contract restated on the host (numpy, no engine code): the tests compare the HIP path with it bit for bit.

DESIGN §5b / README ("documented divergences"): the same threshold and count as the reference's topk -- k = int(numel * frac) elements
pruned, the k-th smallest magnitude the threshold -- and of the elements EQUAL to the threshold (the tie class) the lowest flat indices
are pruned first.  Magnitudes compare as |v| does: -0.0 and +0.0 are one key, and every NaN (any payload, either sign) forms one class
above +inf, as in ATen's comparator.  A pruned element becomes +0.0."""
import numpy as np
import torch


def mag_keys(xc):
    """int64 magnitude keys of a host tensor in flat order: the bit pattern without its sign, every NaN canonicalised to inf + 1"""
    dt = xc.dtype
    if dt == torch.float32:
        keys = xc.contiguous().view(torch.int32).numpy().reshape(-1).astype(np.int64) & 0x7FFFFFFF
        inf = 0x7F800000
    else:
        keys = xc.contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1).astype(np.int64) & 0x7FFF
        inf = 0x7F80 if dt == torch.bfloat16 else 0x7C00
    return np.minimum(keys, inf + 1)


def flat_order_threshold(xc, frac, keys=None):
    """(k, tau, need): the count int(numel * frac), the k-th smallest magnitude key (None when k == 0) and how many elements of
    the tie class are pruned"""
    keys = mag_keys(xc) if keys is None else keys
    k = int(xc.numel() * frac)
    if k == 0:
        return 0, None, 0
    tau = int(np.partition(keys, k - 1)[k - 1])
    return k, tau, k - int((keys < tau).sum())


def flat_order_prune(xc, frac):
    """the engine's own rule, restated in numpy: everything below the k-th smallest magnitude, plus the first `need`
    elements EQUAL to it in flat index order (NaNs form one largest class, as in ATen's comparator)"""
    keys = mag_keys(xc)
    k, tau, need = flat_order_threshold(xc, frac, keys)
    out = xc.contiguous().view(-1).clone()
    if k == 0:
        return out.view(xc.shape)
    prune = keys < tau
    prune[np.flatnonzero(keys == tau)[:need]] = True
    raw = out.view(torch.int32 if xc.dtype == torch.float32 else torch.int16).numpy()
    raw[prune] = 0                                                             # +0.0
    return out.view(xc.shape)


# ---- inputs holding special values ------------------------------------------------------------------------------------------------
# bit patterns per dtype: NaNs of several payloads and both signs, the subnormals the selector must order by their bits
NAN_BITS = {torch.float32: [0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0xFF800123],
            torch.bfloat16: [0x7FC0, 0x7F81, 0xFFC0, 0x7FFF, 0xFF81],
            torch.float16: [0x7E00, 0x7C01, 0xFE00, 0x7FFF, 0xFC01]}
SUBNORMAL_BITS = {torch.float32: [0x1, 0x2, 0x3FF, 0x400000, 0x7FFFFF],
                  torch.bfloat16: [0x1, 0x2, 0x1F, 0x40, 0x7F],
                  torch.float16: [0x1, 0x2, 0x3F, 0x200, 0x3FF]}
INF_BITS = {torch.float32: 0x7F800000, torch.bfloat16: 0x7F80, torch.float16: 0x7C00}
SIGN_BIT = {torch.float32: 0x80000000, torch.bfloat16: 0x8000, torch.float16: 0x8000}

# the class the threshold lands in (in magnitude order: zeros < subnormals < normal finite < inf < NaN) and the share of
# the tensor each special class takes ('spread' and 'run' layouts) or its count ('segment' layout)
SPECIAL_KINDS = ("zero", "subnormal", "inf", "nan")
_SHARES = {"zero": dict(zero=0.30, sub=0.05, inf=0.05, nan=0.05),
           "subnormal": dict(zero=0.10, sub=0.30, inf=0.05, nan=0.05),
           "inf": dict(zero=0.05, sub=0.05, inf=0.30, nan=0.10),
           "nan": dict(zero=0.05, sub=0.05, inf=0.05, nan=0.60)}
_SEGMENT_COUNTS = {"zero": dict(zero=1500, sub=300, inf=200, nan=200),
                   "subnormal": dict(zero=300, sub=1500, inf=200, nan=200),
                   "inf": dict(zero=200, sub=200, inf=1500, nan=300),
                   "nan": dict(zero=200, sub=200, inf=300, nan=1500)}
SPECIAL_LAYOUTS = ("spread", "run", "segment")


def special_values(shape, dtype, kind, layout, seed=0):
    """(x, frac): a host tensor of normal values (randn) holding +-0, subnormals, +-inf and NaNs, and the fraction whose
    threshold falls in the middle of the `kind` class of x.  layout 'spread': the specials at random positions; 'run': the
    same specials as one contiguous run; 'segment': a few thousand specials inside one 4096-element window."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    wide = np.uint32 if dtype == torch.float32 else np.uint16
    base = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dtype)
    raw = base.view(torch.int32 if dtype == torch.float32 else torch.int16).numpy().view(wide)
    raw[(raw & ~wide(SIGN_BIT[dtype])) == 0] = 0x1 << (23 if dtype == torch.float32 else 7 if dtype == torch.bfloat16 else 10)  # no stray zeros
    counts = (_SEGMENT_COUNTS[kind] if layout == "segment" else {c: int(s * n) for c, s in _SHARES[kind].items()})
    sign = lambda m: rng.integers(0, 2, m).astype(wide) * wide(SIGN_BIT[dtype])        # noqa: E731
    vals = np.concatenate([
        sign(counts["zero"]),
        np.array(SUBNORMAL_BITS[dtype], dtype=wide)[rng.integers(0, 5, counts["sub"])] | sign(counts["sub"]),
        np.full(counts["inf"], INF_BITS[dtype], dtype=wide) | sign(counts["inf"]),
        np.array(NAN_BITS[dtype], dtype=wide)[rng.integers(0, 5, counts["nan"])]])
    rng.shuffle(vals)
    m = vals.size
    if layout == "spread":
        pos = rng.choice(n, m, replace=False)
    elif layout == "run":
        start = int(rng.integers(0, n - m + 1))
        pos = np.arange(start, start + m)
    else:
        start = int(rng.integers(0, n - 4096 + 1))
        pos = start + rng.choice(4096, m, replace=False)
    raw[pos] = vals
    order = ("zero", "sub", "normal", "inf", "nan")
    sizes = dict(counts, normal=n - m)
    lo = sum(sizes[c] for c in order[:order.index({"subnormal": "sub"}.get(kind, kind))])
    size = sizes[{"subnormal": "sub"}.get(kind, kind)]
    k = lo + (size * 9 // 10 if kind == "nan" else size // 2)                         # inside the class (NaN: frac near 1)
    return base.view(shape), (k + 0.5) / n
