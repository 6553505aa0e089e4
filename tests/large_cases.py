"""The geometries of the large-offset tests (tests/test_large_offsets_host.py, tests/test_large_offsets_gpu.py) as data, and
the byte arithmetic both tests share: what a cache of a geometry allocates, and which sequence or head holds a given byte of a buffer.

Nothing here needs the library or a device.  The host test holds these formulas to the library's own predicates and workspace entries,
so a geometry edited below its point -- a buffer under 2^32 bytes, a grid dimension under 65536, a shape a guard refuses -- fails there
before the GPU test runs on premises that no longer hold."""

GiB = 1 << 30
P31, P32 = 1 << 31, 1 << 32
BUDGET = 24 * GiB                      # the most one test function may hold at its peak
GRID = 65535                           # a grid dimension of the launches: more heads or tiles take a second trip of a kernel's loop
ESIZE = 2                              # every case runs bf16


def pitch(n):
    """native.code_pitch: n rounded up to 64-byte chunks"""
    return (n + 63) // 64 * 64


def dec_ws_bytes(BH, Tq, D, L, block):
    """bfpq_kv_dec_ws_bytes: the int32 block sums [BH, Tq, nbw, D], then x's block exponents"""
    return (BH * Tq * ((L + block - 1) // block) * (4 * D + 1) + 15) // 16 * 16


def score_ws_bytes(BH, Tq, L):
    """bfpq_kv_attend_ws_bytes and bfpq_kv_attend_rows_ws_bytes: fp32 score rows [BH, Tq, L rounded up to 4]"""
    return (BH * Tq * ((L + 3) // 4 * 4) * 4 + 15) // 16 * 16


def kv(batch, heads, kv_heads, head_dim, capacity, block, device_lengths=True, max_query_rows=16, prompt_rows=0, starts=False, **run):
    """a cache geometry; `run` holds what the case does with it (slab: sequences per twin; the rest is the case's own)"""
    return dict(batch=batch, heads=heads, kv_heads=kv_heads, head_dim=head_dim, capacity=capacity, block=block, device_lengths=device_lengths,
                max_query_rows=max_query_rows, prompt_rows=prompt_rows, starts=starts, **run)


def cache_kwargs(c, batch=None, capacity=None):
    """what HBFPKVCache takes of a geometry beside the bfp_args (a twin: fewer sequences, perhaps another capacity)"""
    kw = dict(batch=c['batch'] if batch is None else batch, heads=c['heads'], head_dim=c['head_dim'],
              capacity=c['capacity'] if capacity is None else capacity, kv_heads=c['kv_heads'], device_lengths=c['device_lengths'])
    if c['device_lengths']:
        kw.update(max_query_rows=c['max_query_rows'], prompt_rows=c['prompt_rows'], starts=c['starts'])
    return kw


def allocations(c, batch=None, capacity=None, attend=True):
    """bytes of everything an HBFPKVCache of the geometry holds (attend: after its first attend()), by name"""
    B = c['batch'] if batch is None else batch
    cap = pitch(c['capacity'] if capacity is None else capacity)
    H, Hq, D, blk = c['kv_heads'], c['heads'], c['head_dim'], c['block']
    a = dict(k_codes=B * H * cap * pitch(D), k_exps=B * H * cap * (D // blk), v_codes=B * H * D * cap, v_exps=B * H * D * (cap // blk),
             v_tail=B * H * blk * D * ESIZE)
    if c['device_lengths']:
        a['sum_ws'] = dec_ws_bytes(B * Hq, c['max_query_rows'], D, cap, blk)
        if attend:
            a['score_ws'] = score_ws_bytes(B * Hq, c['max_query_rows'], cap)
            if c['prompt_rows']:
                a['rows_ws'] = score_ws_bytes(B * Hq, c['prompt_rows'], cap)
    return a


def holder(nbytes_per_unit, point):
    """(the unit -- sequence, head or batch -- that holds byte `point` of a buffer of equal units, whether a unit starts exactly there)"""
    return point // nbytes_per_unit, point % nbytes_per_unit == 0


def per_sequence(c, name):
    return allocations(c, batch=1)[name]


def per_head(c, name):
    return allocations(c, batch=1)[name] // (c['heads'] if name.endswith('_ws') else c['kv_heads'])


def ragged_counts(batch, t):
    """what sequence b takes of a chunk of t rows: every count 0..t occurs once batch > t"""
    return [(7 * b + 5) % (t + 1) for b in range(batch)]


# ---- A / B: the serving shape.  640 sequences x 8 kv heads x 8000 tokens x 128: 5.24 GB of k_codes and of v_codes ---------------------------
A = kv(640, 32, 8, 128, 8000, 64, max_query_rows=3, slab=32, chunk=70, max_len=256, tqs=(1, 3), window=48,
       over=('k_codes', 'v_codes'), straddle={'k_codes': (262, 524), 'v_codes': (262, 524)}, anchors=(524, 639))
B = kv(640, 32, 8, 128, 8000, 64, device_lengths=False, slab=32, chunk=70, tqs=(3, 40),
       over=('k_codes', 'v_codes'), straddle={'k_codes': (262, 524), 'v_codes': (262, 524)}, anchors=(524, 639))

# ---- C: long sequences.  3 x 8 heads x 2^20 tokens x 256: 6 GiB per code buffer, head 8 starts at byte 2^31 and head 16 at byte 2^32 -------
C = kv(3, 8, 8, 256, 1 << 20, 64, max_query_rows=1, prompt_rows=16, starts=True, slab=3, lens=(200, 70, 130), early_starts=(5, 0, 17),
       early_capacity=320, late_capacity=1024, tqs=(1, 40), over=('k_codes', 'v_codes'), exact_heads={'k_codes': (8, 16), 'v_codes': (8, 16)})
C['late_at'] = C['capacity'] - C['late_capacity']         # P0: where phase 2 puts the tokens

# ---- D: workspaces and p past 4 GiB at a small cache ---------------------------------------------------------------------------------------
D = kv(33, 16, 2, 16, 128000, 16, slab=3, tq=16, over=('score_ws', 'sum_ws'))
D['p_bytes'] = D['batch'] * D['heads'] * D['tq'] * D['capacity'] * ESIZE

# ---- E: the batched matmul's output past 4 GiB -----------------------------------------------------------------------------------------------
E = dict(B=160, T=4080, N=4096, K=64, blocks=(64, 16), slab=8, mant_bits=5, x_marker=(150, 1234), w_marker=(155, 4001))
E['out_batch_bytes'] = E['T'] * E['N'] * ESIZE

# ---- F: more heads, tiles or batches than a grid dimension -----------------------------------------------------------------------------------
F_HOST = kv(8200, 8, 8, 64, 64, 64, device_lengths=False, slab=410, chunk=40, tqs=(3,), anchors=(GRID // 8,))        # 65600 heads
F_DEV = kv(33000, 2, 1, 64, 64, 64, slab=1500, tq=16, chunk=64)                                                       # 66000 tiles of 16 rows
F_BMM = dict(B=66000, T=16, N=16, K=64, slab=4125, mant_bits=7)
F_BLOCKS = (64, 16)


def f_dev_lengths(batch, cap):
    """ragged lengths 0..cap, different for the heads a trip of 65535 tiles apart (two tiles per sequence: 32767 or 32768 sequences on)"""
    return [(12 * b + 3) % (cap + 1) for b in range(batch)]


def with_block(c, block):
    return dict(c, block=block)
