"""The premises of tests/test_large_offsets_gpu.py, checked without a device: every geometry of tests/large_cases.py is taken
by the entries it is meant for (the library's own predicates and workspace entries), the buffer each case names really passes 2^32 bytes,
bytes 2^31 and 2^32 fall in the sequence or head the case says (inside it where it says "straddles", on its first byte where it says
"starts"), the loops it is for really take a second trip, and everything one test function holds fits the memory budget.  A geometry
shrunk below its point fails here."""
import pytest

import large_cases as LC
from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

KV_CASES = {'A': LC.A, 'B': LC.B, 'C': LC.C, 'D': LC.D, 'F_HOST': LC.F_HOST, 'F_DEV': LC.F_DEV}


def _blocks(name):
    return LC.F_BLOCKS if name.startswith('F') else (KV_CASES[name]['block'],)


@pytest.mark.parametrize("name", sorted(KV_CASES))
def test_the_library_takes_the_geometry_and_sizes_agree(name):
    for block in _blocks(name):
        c = LC.with_block(KV_CASES[name], block)
        cap, D = LC.pitch(c['capacity']), c['head_dim']
        assert cap == native.code_pitch(c['capacity']) and LC.pitch(D) == native.code_pitch(D)
        assert native.kv_ok(D, cap, block) and c['heads'] % c['kv_heads'] == 0 and D % block == 0
        for twin_cap in (c.get('early_capacity'), c.get('late_capacity')):
            assert twin_cap is None or native.kv_ok(D, LC.pitch(twin_cap), block)
        a = LC.allocations(c)
        if c['device_lengths']:
            BH = c['batch'] * c['heads']
            assert a['sum_ws'] == native.kv_dec_ws_bytes(BH, c['max_query_rows'], D, cap, block)
            assert a['score_ws'] == native.kv_attend_ws_bytes(BH, c['max_query_rows'], cap)
            if c['prompt_rows']:
                assert a['rows_ws'] == native.kv_attend_rows_ws_bytes(BH, c['prompt_rows'], cap)
                assert 16 <= c['prompt_rows'] <= bfp_ops.HBFPKVCache.prompt_rows_max(c['batch'], c['heads'], c['capacity'])
                assert D <= native.KV_ROWS_MAX_HEAD_DIM
        # the per-head guards of the entries (dec_shapes_ok, att_shapes_ok): a head's codes, and its rows of the outputs, below 2^31
        assert cap * LC.pitch(D) < LC.P31 and D * cap < LC.P31
        rows = c['heads'] // c['kv_heads'] * c['max_query_rows'] if c['device_lengths'] else 0
        assert rows * cap < LC.P31


@pytest.mark.parametrize("name", ('A', 'B', 'C', 'D'))
def test_the_named_buffers_pass_4gib(name):
    c = KV_CASES[name]
    a = LC.allocations(c)
    for buf in c['over']:
        assert a[buf] > LC.P32, f"case {name}: {buf} holds {a[buf]} bytes, no more than 2^32"
    if name == 'D':
        assert LC.P31 < c['p_bytes'] < LC.P32                                # p passes 2^31; the workspaces pass 2^32
        assert a['k_codes'] + a['v_codes'] < LC.GiB                          # ... next to a small cache


@pytest.mark.parametrize("name", ('A', 'B'))
def test_bytes_2_31_and_2_32_lie_inside_the_sequences_named(name):
    c = KV_CASES[name]
    for buf, (s31, s32) in c['straddle'].items():
        unit = LC.per_sequence(c, buf)
        assert LC.holder(unit, LC.P31) == (s31, False), (name, buf)
        assert LC.holder(unit, LC.P32) == (s32, False), (name, buf)
        assert s32 < c['batch'] - 1                                         # whole sequences lie above the point
    assert c['anchors'] == (c['straddle']['k_codes'][1], c['batch'] - 1)    # the oracle anchors: the straddling and the last sequence
    counts = LC.ragged_counts(c['batch'], c['chunk'])
    assert {0, 1, 63, 64, 65, 70} <= set(counts) and max(counts) == c['chunk'] == 70
    assert all(counts[b] > 0 for b in c['anchors'])
    assert c['batch'] % c['slab'] == 0


def test_case_c_has_heads_that_start_exactly_on_the_points():
    c = LC.C
    for buf, (h31, h32) in c['exact_heads'].items():
        unit = LC.per_head(c, buf)
        assert LC.holder(unit, LC.P31) == (h31, True) and LC.holder(unit, LC.P32) == (h32, True), buf
        assert h32 < c['batch'] * c['kv_heads']
    P0 = c['late_at']
    assert P0 % 1024 == 0 and P0 % c['block'] == 0 and P0 + max(c['lens']) <= c['capacity'] and c['late_capacity'] == c['capacity'] - P0
    assert max(c['lens']) <= c['early_capacity'] and max(c['lens']) <= c['late_capacity']
    # the 32-bit tail n * ldw of k_kv_bmm_dec: the live key rows are the last 1024 of the capacity, the largest n * ldw the geometry has
    assert P0 + max(c['lens']) > c['capacity'] - 1024 and c['capacity'] * LC.pitch(c['head_dim']) < LC.P31
    assert (P0 + max(c['lens'])) * LC.pitch(c['head_dim']) > (1 << 28) - 1024 * LC.pitch(c['head_dim'])
    assert max(c['tqs']) > 2 * c['prompt_rows'] and max(c['tqs']) % c['prompt_rows']                       # three panels, the last one short


def test_case_d_runs_whole_workspaces():
    c = LC.D
    assert c['tq'] == c['max_query_rows'] == native.KV_DEC_MAX_TOKENS
    tiles = c['batch'] * c['kv_heads'] * ((c['heads'] // c['kv_heads'] * c['tq'] + 15) // 16)
    assert tiles <= LC.GRID and c['batch'] % c['slab'] == 0
    for ws in c['over']:                                                         # bytes 2^31 and 2^32 of either workspace: inside sequence 16, and the last
        assert LC.holder(LC.per_sequence(c, ws), LC.P31) == (16, False) and LC.holder(LC.per_sequence(c, ws), LC.P32) == (c['batch'] - 1, False), ws


@pytest.mark.parametrize("block", LC.E['blocks'])
def test_case_e_output_passes_4gib(block):
    e = LC.E
    assert native.hbfp_bmm_i8_ok(e['B'], e['T'], e['N'], e['K'], e['mant_bits'], e['mant_bits'], block)
    assert native.hbfp_bmm_i8_ok(e['slab'], e['T'], e['N'], e['K'], e['mant_bits'], e['mant_bits'], block)
    unit = e['out_batch_bytes']
    assert e['B'] * unit > LC.P32 and e['B'] % e['slab'] == 0 and e['K'] // block <= 4
    b31, on31 = LC.holder(unit, LC.P31)
    b32, on32 = LC.holder(unit, LC.P32)
    assert not on31 and not on32 and b31 == 64 and b32 == 128
    assert e['x_marker'][0] > b32 and e['w_marker'][0] > b32 and e['x_marker'][0] != e['w_marker'][0]  # both markers in batches past 2^32
    assert e['x_marker'][1] < e['T'] and e['w_marker'][1] < e['N']
    assert e['T'] % 64                                                                              # a ragged last tile of rows


@pytest.mark.parametrize("block", LC.F_BLOCKS)
def test_case_f_takes_a_second_trip(block):
    h, d, m = LC.with_block(LC.F_HOST, block), LC.with_block(LC.F_DEV, block), LC.F_BMM
    # (i) k_kv_bmm_dec kHost: blockIdx.y runs over the heads
    assert h['batch'] * h['kv_heads'] > LC.GRID and h['heads'] == h['kv_heads'] and h['batch'] % h['slab'] == 0
    assert h['slab'] * h['kv_heads'] <= LC.GRID and h['chunk'] + 1 <= h['capacity']
    assert h['anchors'][0] * h['kv_heads'] <= LC.GRID < (h['anchors'][0] + 1) * h['kv_heads']       # the anchor holds head 65535
    # (ii) k_kv_bmm_dec kDev, GRP: blockIdx.y runs over (head, tile of 16 rows)
    group = d['heads'] // d['kv_heads']
    per_head = (group * d['tq'] + 15) // 16
    tiles = d['batch'] * d['kv_heads'] * per_head
    assert group == 2 and per_head == 2 and tiles > LC.GRID and d['batch'] % d['slab'] == 0 and d['slab'] * per_head <= LC.GRID
    lens = LC.f_dev_lengths(d['batch'], d['capacity'])
    assert min(lens) == 0 and max(lens) == d['capacity'] == d['chunk']
    for y in range(tiles - LC.GRID):                                                                # the tile a trip on reads another length
        assert lens[y // per_head] != lens[(y + LC.GRID) // per_head], y
    assert lens[LC.GRID // per_head] > 0                                                            # the first head of the second trip
    # scores() takes that many tiles; attend() and context() refuse them (tests/test_kvcache_gqa_host.py pins the refusal)
    assert native.kv_dec_ws_bytes(d['batch'] * d['heads'], d['tq'], d['head_dim'], d['capacity'], block) > 0
    # (iii) k_bmm_i8 and k_codes_t: blockIdx.y / blockIdx.z run over the batches
    assert m['B'] > LC.GRID and m['B'] % m['slab'] == 0 and m['slab'] <= LC.GRID
    assert native.hbfp_bmm_i8_ok(m['B'], m['T'], m['N'], m['K'], m['mant_bits'], m['mant_bits'], block)


def _inputs_and_outputs(name, c):
    """bytes of the tensors a GPU test of the case holds beside the caches, each counted at its largest, the twin's copies included"""
    B, Hq, H, D, cap = c['batch'], c['heads'], c['kv_heads'], c['head_dim'], c['capacity']
    es = LC.ESIZE
    if name in ('A', 'B', 'F_HOST'):
        tq = max(c['tqs'])
        L = c.get('max_len', c['chunk'] + 1)
        tokens = 2 * B * H * (c['chunk'] + 1) * D * es
        per_call = B * Hq * tq * (D + L) * es                               # a context and a p (or the scores) of one call
        calls = 2 * len(c['tqs']) + 2
        return tokens + B * Hq * tq * D * es * len(c['tqs']) + 2 * calls * per_call + 4 * B * Hq * tq * L   # the fp32 softmax of a p
    if name == 'C':
        tq = max(c['tqs'])
        return 4 * (2 * B * H * max(c['lens']) * D * es + B * Hq * tq * D * es * 2 + 3 * B * Hq * cap * es)
    if name == 'D':
        slab = c['slab'] / B
        return int((1 + slab) * (c['p_bytes'] * 2 + 2 * B * Hq * c['tq'] * D * es)) + 2 * B * H * 256 * D * es
    if name == 'F_DEV':
        return 2 * B * H * c['chunk'] * D * es + 3 * B * Hq * c['tq'] * (D + cap) * es
    raise KeyError(name)


@pytest.mark.parametrize("name", sorted(KV_CASES))
def test_everything_a_test_holds_fits_the_budget(name):
    for block in _blocks(name):
        c = LC.with_block(KV_CASES[name], block)
        big = sum(LC.allocations(c).values())
        twins = [sum(LC.allocations(c, batch=c['slab'], capacity=cp).values()) for cp in (c.get('early_capacity'), c.get('late_capacity')) if cp]
        twin = max(twins) if twins else sum(LC.allocations(c, batch=c['slab']).values())
        total = big + twin + _inputs_and_outputs(name, c)
        assert total <= LC.BUDGET, f"case {name} block {block}: {total / LC.GiB:.2f} GiB"
        assert big > twin


@pytest.mark.parametrize("block", LC.E['blocks'])
def test_the_matmul_cases_fit_the_budget(block):
    for e in (LC.E, LC.F_BMM):
        nb = e['K'] // block
        operands = e['B'] * (e['T'] + e['N']) * (native.code_pitch(e['K']) + nb)
        out = e['B'] * e['T'] * e['N'] * LC.ESIZE
        slab = e['slab'] * e['T'] * e['N'] * LC.ESIZE
        fp64 = 3 * e['T'] * e['N'] * 8 + 2 * (e['T'] + e['N']) * e['K'] * 8         # the product, |x| |w| and the bound of one batch
        floats = e['B'] * (e['T'] + e['N']) * e['K'] * (LC.ESIZE + 4)                # (F) the float operands and their fp32 draws
        assert operands + out + 2 * slab + fp64 + floats <= LC.BUDGET
