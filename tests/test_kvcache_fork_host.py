"""Host-side checks of page sharing on the paged HBFP KV cache (HBFPKVCache.fork / reorder): the reference counts of the page
allocator, the plan of a reorder (lists, counts, queue, jobs -- a pure function of the host state), its refusals, and the C entry
bfpq_kv_rows_move -- exported, declared in include/bfpq.h as native.py binds it, refusing bad arguments before any launch.  No GPU
needed: caches live on device='meta', `tokens` is always given (nothing can be read back), and the pointers are not memory."""
import ctypes
import os
import re

import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops

E_ARG, E_UNSUPPORTED = -1, -2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bfpq.h")
PT = 64
P = ctypes.c_void_p(16)
Z = None
S = ctypes.c_void_p(0)


def L():
    return native.load_library()


def _args(**kw):
    base = dict(num_format='bfp', sparsity_num_format='bfp', rounding_mode='determ', block_size=64, mant_bits=7, epsilon=1e-8)
    base.update(kw)
    return dict(bfp_ops.unpack_bfp_args(base), device='meta')


def paged(batch=4, pages=12, **kw):
    kw = dict(dict(device_lengths=True, page_tokens=PT, pages=pages), **kw)
    return bfp_ops.HBFPKVCache(batch, 4, 64, 256, dtype=torch.bfloat16, **dict(_args(), **kw))


def state(c):
    return c._table_host.clone(), list(c._free), [list(o) for o in c._owned], c.page_refs


def same_state(a, b):
    return torch.equal(a[0], b[0]) and a[1:] == b[1:]


def consistent(c):
    """owned and free make up the pool, a page is free exactly when its count is 0, the counts add up to the lists, and the host
    mirror of the table is the lists"""
    refs, owned, free = c.page_refs, [p for o in c._owned for p in o], list(c._free)
    assert len(set(free)) == len(free) and set(owned) | set(free) == set(range(c.page_count)) and not set(owned) & set(free)
    assert [p for p in range(c.page_count) if refs[p] == 0] == sorted(free)
    assert refs == [owned.count(p) for p in range(c.page_count)] and sum(refs) == sum(len(o) for o in c._owned)
    assert c.pages_shared == sum(1 for n in refs if n > 1) and c.pages_free == len(free)
    for b, o in enumerate(c._owned):
        assert len(set(o)) == len(o) and c._table_host[b].tolist() == o + [-1] * (c._table_host.shape[1] - len(o)), b


# ---- the counts after a fork ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 128])
def test_fork_shares_the_full_pages_and_copies_the_open_one(length):
    c = paged()
    c.reserve([length, 0, 70, 0])
    src, other, free = list(c._owned[0]), list(c._owned[2]), list(c._free)
    full, part = length // PT, length % PT != 0
    assert len(src) == full + part
    before = state(c)
    plan = c._plan_reorder([0, 0, 2, 0], [length, 0, 0, 0])
    assert same_state(before, state(c))                                  # planning is pure
    c.fork(0, [1, 3], length)
    consistent(c)
    assert c._owned[0] == src and c._owned[2] == other                   # the source is the heir of itself: its own pages, all of them
    fresh = free[:2 * part]                                              # one page per destination, from the left of the queue
    assert c._owned[1] == src[:full] + fresh[:1] and c._owned[3] == src[:full] + fresh[1:2]
    assert list(c._free) == free[2 * part:] and c.pages_free == len(free) - 2 * part
    refs = c.page_refs
    assert all(refs[p] == 3 for p in src[:full]) and all(refs[p] == 1 for p in src[full:] + fresh + other)
    assert c.pages_shared == full
    jobs = [(0, d, src[full] if part else -1, f if part else -1, length) for d, f in zip((1, 3), fresh or (None, None))]
    assert plan[3] == jobs and [list(o) for o in plan[0]] == c._owned and plan[1] == refs and list(plan[2]) == list(c._free)


def test_fork_takes_an_int_a_list_or_a_range_and_releases_what_dst_held():
    c = paged()
    c.reserve([130, 64, 0, 200])
    held1, held3, src = list(c._owned[1]), list(c._owned[3]), list(c._owned[0])
    c.fork(0, 1, 130)
    consistent(c)
    assert c._owned[1][:2] == src[:2] and c._owned[1][2] not in src + held1 and c.page_refs[held1[0]] == 0
    assert list(c._free)[-1:] == held1                                   # released to the right of the queue
    c.fork(0, range(1, 4), 130)
    consistent(c)
    assert all(c._owned[d][:2] == src[:2] and len(c._owned[d]) == 3 for d in (1, 2, 3)) and c.page_refs[src[0]] == 4
    assert not set(held3) & {p for o in c._owned for p in o} - set(c._owned[1] + c._owned[2] + c._owned[3])


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------------
def test_release_keeps_shared_pages_until_the_last_owner_lets_go():
    c = paged()
    c.reserve([130, 0, 0, 0])
    src = list(c._owned[0])
    c.fork(0, [1, 2], 130)
    mine = {d: c._owned[d][2] for d in (1, 2)}
    free = list(c._free)
    c.release(0)
    consistent(c)
    assert list(c._free) == free + [src[2]] and c.page_refs[src[0]] == 2 and c._owned[0] == []    # only its open page comes back
    c.release(1)
    consistent(c)
    assert list(c._free) == free + [src[2], mine[1]] and c.page_refs[src[0]] == 1 and c.pages_shared == 0
    c.release(2)                                                         # the last owner: the shared pages return, to the right, in row order
    consistent(c)
    assert list(c._free) == free + [src[2], mine[1], src[0], src[1], mine[2]] and c.pages_free == 12


def test_reserve_after_fork_extends_from_the_forked_rows_pages():
    c = paged()
    c.reserve([200, 0, 0, 0])                                            # four pages: the heir keeps the reserve beyond its open page
    src = list(c._owned[0])
    c.fork(0, 1, 70)
    assert c._owned[0] == src and len(c._owned[1]) == 2 and c._owned[1][0] == src[0]
    before = list(c._owned[1])
    c.reserve([0, 71, 0, 0])                                             # has the pages already
    assert c._owned[1] == before
    c.reserve([0, 129, 0, 0])
    consistent(c)
    assert c._owned[1][:2] == before and len(c._owned[1]) == 3 and c.page_refs[c._owned[1][2]] == 1
    c.fork(0, 2, 128)                                                    # L % P == 0: nothing copied, the new row owns exactly the full pages
    assert c._owned[2] == src[:2] and c.page_refs[src[0]] == 3 and c.page_refs[src[1]] == 2
    free = c.pages_free
    c.reserve([0, 0, 129, 0])
    consistent(c)
    assert c._owned[2][:2] == src[:2] and len(c._owned[2]) == 3 and c.pages_free == free - 1


def test_reset_returns_everything():
    c = paged()
    c.reserve([130, 64, 0, 5])
    c.fork(0, [1, 2], 130)
    c.reorder([3, 3, 0, 1], [130, 130, 130, 5])
    consistent(c)
    c.reset()
    consistent(c)
    assert c.pages_free == 12 and c.page_refs == [0] * 12 and c.pages_shared == 0 and c._owned == [[], [], [], []]
    assert torch.equal(c._table_host, torch.full((4, 4), -1, dtype=torch.int32))


# ---- reorder -------------------------------------------------------------------------------------------------------------------------------
def test_the_heir_rule_names_the_jobs():
    c = paged()
    tokens = [70, 129, 5, 64]
    c.reserve(tokens)
    o, free = [list(x) for x in c._owned], list(c._free)
    c_plan = c._plan_reorder([1, 0, 0, 3], tokens)
    c.reorder([1, 0, 0, 3], tokens)
    consistent(c)
    # old 1 -> row 0 alone: the heir, its pages move with the table row.  old 0 -> rows 1 and 2: row 1, the lowest, is the heir; row 2
    # shares the full page and gets a copy of the open one.  Row 3 is its own source: no job.  Old row 2 is named by nobody: released
    assert c._owned == [o[1], o[0], [o[0][0], free[0]], o[3]]
    assert c_plan[3] == [(1, 0, -1, -1, 129), (0, 1, -1, -1, 70), (0, 2, o[0][1], free[0], 70)]
    assert list(c._free) == free[1:] + o[2] and c.page_refs[o[0][0]] == 2 and c.pages_shared == 1
    c.reorder([0, 1, 2, 3], [129, 70, 70, 64])                           # the identity: nothing moves, nothing is planned
    assert c._plan_reorder([0, 1, 2, 3], [129, 70, 70, 64])[3] == [] and c._owned == [o[1], o[0], [o[0][0], free[0]], o[3]]
    # the source among its own heirs keeps its pages wherever it stands
    c.reorder([2, 2, 2, 3], [129, 70, 70, 64])
    consistent(c)
    assert c._owned[2] == [o[0][0], free[0]] and c._owned[0][0] == o[0][0] and c._owned[1][0] == o[0][0] and c.page_refs[o[0][0]] == 3


def test_a_cycle_loses_no_page():
    c = paged(pages=8)
    tokens = [70, 129, 5, 64]
    c.reserve(tokens)                                                    # 2 + 3 + 1 + 1 of 8 pages
    o, free = [list(x) for x in c._owned], list(c._free)
    plan = c._plan_reorder([1, 2, 0, 3], tokens)
    c.reorder([1, 2, 0, 3], tokens)
    consistent(c)
    assert c._owned == [o[1], o[2], o[0], o[3]] and list(c._free) == free and c.pages_shared == 0
    assert plan[3] == [(1, 0, -1, -1, 129), (2, 1, -1, -1, 5), (0, 2, -1, -1, 70)]      # rows move; no page is copied
    c.reorder([1, 0, 2, 3], [129, 5, 70, 64])                            # a swap
    consistent(c)
    assert c._owned == [o[2], o[1], o[0], o[3]] and list(c._free) == free


def test_exhaustion_raises_and_changes_nothing():
    c = paged(pages=5)
    c.reserve([70, 70, 0, 0])                                            # four pages taken, one free
    before = state(c)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.reorder([0, 0, 1, 1], [70, 70, 0, 0])                          # two copies wanted, one free, nothing released
    with pytest.raises(RuntimeError, match="exhausted"):
        c.fork(0, [2, 3], 70)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.reorder([0, 0, 0, 1], [70, 70, 0, 0])                          # row 1 moves to row 3 and keeps its pages: still two wanted
    assert same_state(before, state(c)) and c._move_ws is None
    c.fork(0, 2, 70)                                                     # what fits still fits
    consistent(c)
    assert c.pages_free == 0
    c = paged(pages=6)                                                   # one page more, and two copies fit
    c.reserve([70, 70, 0, 0])
    c.reorder([0, 0, 0, 1], [70, 70, 0, 0])
    consistent(c)
    assert c.pages_free == 0 and c.pages_shared == 1 and c.page_refs[c._owned[0][0]] == 3


def test_pages_released_in_the_same_call_count_toward_the_supply():
    c = paged(pages=5)
    c.reserve([70, 130, 0, 0])                                           # all five pages taken
    o = [list(x) for x in c._owned]
    assert c.pages_free == 0
    with pytest.raises(RuntimeError, match="exhausted"):
        c.fork(0, 2, 70)                                                 # row 1 stays: nothing to copy into
    c.fork(0, [1, 2], 70)                                                # row 1 goes: its three pages serve, in its row order
    consistent(c)
    assert c._owned == [o[0], [o[0][0], o[1][0]], [o[0][0], o[1][1]], []] and list(c._free) == [o[1][2]]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_change_nothing():
    c = paged()
    c.reserve([70, 64, 0, 0])
    before = state(c)
    for src, dst in ((0, 0), (0, [1, 0]), (0, [1, 1]), (0, 4), (4, 1), (-1, 1), (0, -1), (True, 1), (0, True), (0, [True]), (0, 1.0), (0, "1")):
        with pytest.raises(ValueError, match="fork"):
            c.fork(src, dst, 70)
    for tokens in (-1, 257, True, 70.0, [70], 129):                      # outside the capacity; more than row 0 has pages for
        with pytest.raises(ValueError):
            c.fork(0, 1, tokens)
    for index in ([0, 1, 2], [0, 1, 2, 3, 0], [0, 1, 2, 4], [0, -1, 2, 3], [0, True, 2, 3], [0, 1.0, 2, 3], 3,
                  torch.zeros(4), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="reorder"):
            c.reorder(index, [70, 64, 0, 0])
    for tokens in ([70, 64, 0], [70, 64, 0, 0, 0], [70, 64, 0, True], [70, 64, 0, 1.0], [70, 64, 0, -1], [70, 64, 0, 257], 70,
                   [129, 64, 0, 0], [70, 65, 0, 0], [70, 64, 1, 0]):     # the last three: more than the source has pages for
        with pytest.raises(ValueError, match="reorder"):
            c.reorder([0, 1, 2, 3], tokens)
    assert same_state(before, state(c))
    c.reorder(torch.tensor([1, 0, 0, 3]), [70, 64, 0, 0])                # an integer tensor on the host is an index like a list
    consistent(c)
    assert c.pages_shared == 1


def test_a_cache_without_pages_refuses():
    plain = bfp_ops.HBFPKVCache(4, 4, 64, 256, dtype=torch.bfloat16, device_lengths=True, **_args())
    with pytest.raises(ValueError, match="paged cache"):
        plain.fork(0, 1, 0)
    with pytest.raises(ValueError, match="paged cache"):
        plain.reorder([0, 1, 2, 3], [0, 0, 0, 0])
    for name in ("pages_shared", "page_refs"):
        with pytest.raises(ValueError, match="paged cache"):
            getattr(plain, name)


def test_what_exists_keeps_its_behaviour_when_nothing_is_shared():
    c = paged(batch=3, pages=8)
    c.reserve([128, 64, 192])
    assert c.page_refs == [1, 1, 1, 1, 1, 1, 0, 0] and c.pages_shared == 0
    c.page_refs[0] = 7                                                   # a copy
    assert c.page_refs[0] == 1
    c.release(1)
    c.assign(1, [7])
    consistent(c)
    assert list(c._free) == [6, 2] and c.page_refs == [1, 1, 0, 1, 1, 1, 0, 1]


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------------
def _ctype(param):
    if '*' in param:
        return ctypes.c_void_p
    for word, t in (('int64_t', ctypes.c_int64), ('double', ctypes.c_double), ('int', ctypes.c_int)):
        if re.search(rf"\b{word}\b", param):
            return t
    raise AssertionError(param)


def test_the_entry_is_exported_and_declared_as_bound():
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, ret, rtype in (("bfpq_kv_rows_move", "int", ctypes.c_int), ("bfpq_kv_rows_move_ws_bytes", "int64_t", ctypes.c_int64)):
        assert name in native.EXPORTED_SYMBOLS and hasattr(L(), name), name
        m = re.search(rf"\b{ret}\s+{name}\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/bfpq.h"
        restype, argtypes = native.PROTOTYPES[name]
        assert restype is rtype and [_ctype(a.strip()) for a in m.group(1).split(',')] == list(argtypes), name
    names = [a.split()[-1].lstrip('*') for a in re.search(r"\bint\s+bfpq_kv_rows_move\s*\(([^)]*)\)", header).group(1).split(',')]
    assert names == ["k_codes_dev", "k_exps_dev", "v_codes_dev", "v_exps_dev", "v_tail_dev", "lens_dev", "overflow_dev", "jobs_dev", "n_jobs",
                     "stage_dev", "stage_bytes", "B", "kv_heads", "D", "block_size", "dtype", "page_tokens", "pages", "stream"]
    paged_at, move_at = text.index("int bfpq_kv_attend_rows_paged"), text.index("int64_t bfpq_kv_rows_move_ws_bytes")
    assert paged_at < move_at < text.index("2:4-compressed packed weights")                    # beside the _paged entries
    comment = text[:move_at].rsplit("/*", 1)[1]
    for word in ("_reorder_cache", "modeling_gpt2.py:1370-1379", "src_row, dst_row", "tokens", "BFPQ_E_ARG", "BFPQ_E_UNSUPPORTED", "cycle",
                 "cannot fault"):
        assert word in comment, word


def move(*, kc=P, ke=P, vc=P, ve=P, vt=P, ln=P, ov=P, jobs=P, n=3, st=P, sb=1 << 40, B=4, kvh=2, D=64, blk=64, dt=2, pt=64, pages=8):
    return L().bfpq_kv_rows_move(kc, ke, vc, ve, vt, ln, ov, jobs, n, st, sb, B, kvh, D, blk, dt, pt, pages, S)


def test_the_entry_refuses_before_any_launch():
    for kw in (dict(pt=0), dict(pt=32), dict(pt=96), dict(pt=-64), dict(pages=0), dict(pages=-3), dict(n=-1), dict(dt=3), dict(blk=48),
               dict(B=0), dict(kvh=0)):
        assert move(**kw) == E_ARG, kw
    for name in ("kc", "ke", "vc", "ve", "vt", "ln", "ov", "jobs", "st"):
        assert move(**{name: Z}) == E_ARG, name                     # a null pointer
        assert move(**{name: ctypes.c_void_p(18)}) == E_ARG, name   # a misaligned one
    need = L().bfpq_kv_rows_move_ws_bytes(3, 2, 64, 64, 2)
    assert move(sb=need - 1) == E_ARG and move(sb=0) == E_ARG       # a short staging buffer
    for kw in (dict(D=8), dict(D=72), dict(D=2048), dict(D=32, blk=64), dict(pages=1 << 31), dict(B=1 << 31), dict(n=1 << 31)):
        assert move(**kw) == E_UNSUPPORTED, kw                      # what bfpq_kv_ok refuses of (D, P, block); sizes past int32
    assert move(n=0) == 0 and move(n=0, kc=Z, jobs=Z, st=Z, sb=0) == 0                         # no jobs: success, nothing launched
    assert move(n=0, pt=32) == E_ARG and move(n=0, D=8) == E_UNSUPPORTED                       # ... after the checks of the values


@pytest.mark.parametrize("dtype,size", [(torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)])
def test_ws_bytes_matches_its_formula(dtype, size):
    for n, kvh, D, blk in ((0, 2, 64, 64), (1, 1, 16, 16), (3, 2, 64, 64), (4, 2, 64, 16), (5, 12, 128, 32), (8, 32, 1024, 64)):
        want = n * kvh * blk * D * size + (4 * n + 15) // 16 * 16       # the v_tail rows of n jobs, then n int32 rounded up to 16 bytes
        assert native.kv_rows_move_ws_bytes(n, kvh, D, blk, dtype) == want
        assert L().bfpq_kv_rows_move_ws_bytes(n, kvh, D, blk, native.DTYPE_CODE[dtype]) == want
    W = L().bfpq_kv_rows_move_ws_bytes
    assert W(-1, 2, 64, 64, 2) == E_ARG and W(1, 0, 64, 64, 2) == E_ARG and W(1, 2, 64, 48, 2) == E_ARG and W(1, 2, 64, 64, 3) == E_ARG
    assert W(1, 2, 72, 64, 2) == E_UNSUPPORTED and W(1, 2, 2048, 64, 2) == E_UNSUPPORTED and W(1 << 31, 2, 64, 64, 2) == E_UNSUPPORTED
    with pytest.raises(RuntimeError, match="bfpq_kv_rows_move_ws_bytes"):
        native.kv_rows_move_ws_bytes(1, 2, 72, 64, dtype)


def test_the_cache_keeps_one_staging_buffer_for_a_batch_of_jobs():
    c = paged()
    c.reserve([70, 0, 0, 0])
    assert c._move_ws is None
    c.fork(0, 1, 70)
    ws = c._move_ws
    assert ws.numel() == native.kv_rows_move_ws_bytes(4, 4, 64, 64, torch.bfloat16) and ws.dtype == torch.uint8
    c.reorder([0, 0, 0, 0], [70, 70, 0, 0])
    assert c._move_ws is ws
