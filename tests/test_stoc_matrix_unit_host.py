"""The route table of BFPLinear.enable_stochastic_matrix_unit, row by row, on the host: the native predicates answer without a GPU and
every launch is replaced by a recorder.  Also: bad switch values raise, and patch_linear_layers leaves every route alone by default."""
import pytest
import torch
import torch.nn.functional as F

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp import bfp_ops
from quantization_sparsity_interplay_amd.patch import patch_linear_layers

TOKENS = (0, 1, 16, 31, 32, 64, 65, 512, 2048)
WIDTHS = (1, 3, 4, 5, 7)
BLOCKS = (64, 32, 16)
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008), (24, 512), (32, 96), (768, 3072))
mx8_ok, i8_ok = native.hbfp_linear_mx8_ok, native.hbfp_linear_i8_ok


def want_route(T, N, K, m, block, matrix_unit, dtype=torch.bfloat16, limits=None):
    lim = (bfp_ops.STOC_MIN_TOKENS if limits is None else limits).get(dtype, 512)
    if lim is None or T < lim:
        return 'fake'
    if matrix_unit is True and block == 64 and m <= 4 and T >= 32 and mx8_ok(T, N, K, m, m):
        return 'mx8'
    if matrix_unit in (True, 'int8') and T >= 1 and i8_ok(T, N, K, m, m, block):
        return 'int8'
    return 'fake'


def _cfg(m, block, **kw):
    c = dict(num_format='bfp', sparsity_num_format='bfp', block_size=block, mant_bits=m, rounding_mode='stoc', epsilon=1e-8)
    c.update(kw)
    return c


def test_route_table():
    for N, K in SHAPES:
        for m in WIDTHS:
            for block in BLOCKS:
                a = _cfg(m, block)
                for T in TOKENS:
                    for mu in (True, 'int8', False):
                        for dt in (torch.bfloat16, torch.float32, torch.float16):
                            assert bfp_ops._stoc_route(T, N, K, a, mu, dt) == want_route(T, N, K, m, block, mu, dt), (T, N, K, m, block, mu, dt)


def test_token_limits(monkeypatch):
    """the measured limits: bf16 (and unlisted dtypes) from 512 tokens, fp32 never; with the limits lifted the table alone decides"""
    assert bfp_ops.STOC_MIN_TOKENS == {torch.bfloat16: 512, torch.float32: None}
    a = _cfg(7, 64)
    assert bfp_ops._stoc_route(511, 4096, 4096, a, 'int8', torch.bfloat16) == 'fake'
    assert bfp_ops._stoc_route(512, 4096, 4096, a, 'int8', torch.bfloat16) == 'int8'
    assert bfp_ops._stoc_route(2048, 4096, 4096, a, 'int8', torch.float32) == 'fake'
    monkeypatch.setattr(bfp_ops, 'STOC_MIN_TOKENS', {torch.bfloat16: 1, torch.float32: 1})
    for T in TOKENS:
        for mu in (True, 'int8'):
            assert bfp_ops._stoc_route(T, 768, 3072, a, mu, torch.float32) == want_route(T, 768, 3072, 7, 64, mu, torch.float32,
                                                                                             bfp_ops.STOC_MIN_TOKENS)


# ---- the forwards, launches replaced by recorders --------------------------------------------------------------------------------------
def _zeros(shape, dtype=torch.bfloat16):
    return torch.zeros((), dtype=dtype).expand(*shape)


class _OnDevice(torch.Tensor):
    @property
    def device(self):
        return torch.device('cuda', 0)


@pytest.fixture
def calls(monkeypatch):
    log = []
    monkeypatch.setattr(bfp_ops, 'STOC_MIN_TOKENS', {torch.bfloat16: 1, torch.float32: 1})     # (the table alone; limits: test_token_limits)

    def gemm(name, n_of):
        def f(x, *args, **kwargs):
            log.append(name)
            return _zeros(tuple(x.shape[:-1]) + (n_of(args),), torch.float32)
        return f

    def stoc_codes(t, block, m, eps, seed, act=None):
        log.append(('codes', seed, act))
        return _zeros(t.shape, torch.int8), _zeros((t.shape[0], t.shape[1] // block), torch.int8)

    monkeypatch.setattr(native, 'stoc_codes', stoc_codes)
    monkeypatch.setattr(native, 'exp_top_flag', lambda a, b: torch.zeros(1, dtype=torch.int32))
    monkeypatch.setattr(native, 'mx8_from_hbfp', lambda codes, exps, cols, mb, cb: (_zeros((exps.shape[0], cols), torch.uint8), exps))
    monkeypatch.setattr(native, 'hbfp_linear_mx8', gemm('mx8', lambda a: a[0].shape[0]))
    monkeypatch.setattr(native, 'hbfp_linear_i8', gemm('int8', lambda a: a[0].shape[0]))
    monkeypatch.setattr(F, 'linear', gemm('fake', lambda a: a[0].shape[0]))
    monkeypatch.setattr(bfp_ops, 'MxM_pre_processing', lambda x, w, tr, **a: (log.append('fake-operands') or x, w))
    return log


def _gemm(log):
    g = [c for c in log if c in ('mx8', 'int8', 'fake')]
    assert len(g) <= 1, log
    return g[0] if g else 'empty'


@pytest.mark.parametrize("mu", [True, 'int8'])
def test_forward_routes_and_counters(calls, mu):
    for N, K in ((4096, 4096), (24, 512), (768, 3072)):
        w = _zeros((N, K)).as_subclass(_OnDevice)
        for m, block in ((3, 64), (5, 32), (7, 16), (7, 64)):
            lin = bfp_ops.BFPLinear(64, 16, bias=False, **_cfg(m, block)).eval().enable_stochastic_matrix_unit(mu)
            st = lin._stoc_matrix_unit
            assert lin.linear_op.stoc_matrix_unit is st
            for T in TOKENS:
                del calls[:]
                mx, i8 = st.stoc_mx_calls, st.stoc_i8_calls
                before = torch.get_rng_state()
                with torch.no_grad():
                    y = lin.linear_op(_zeros((T, K)).as_subclass(_OnDevice), w)
                assert y.shape == (T, N)
                want = want_route(T, N, K, m, block, mu, limits=bfp_ops.STOC_MIN_TOKENS)
                got = _gemm(calls)
                if want == 'fake':
                    assert got in ('fake', 'empty') and not [c for c in calls if isinstance(c, tuple)], (T, N, K, m, block)
                    continue
                assert got == want, (T, N, K, m, block)
                assert (st.stoc_mx_calls - mx, st.stoc_i8_calls - i8) == ((want == 'mx8') * 1, (want == 'int8') * 1)
                seeds = [c[1] for c in calls if isinstance(c, tuple)]
                # the two seeds the fake route draws, activation first
                torch.set_rng_state(before)
                assert seeds == [bfp_ops._seed_for('stoc'), bfp_ops._seed_for('stoc')]


def test_operand_sparsity_specs(calls):
    """each operand is pruned as float_to_bfp_blocked prunes it: activations by in_sparsity, weights by w_sparsity, either order"""
    w = _zeros((256, 512)).as_subclass(_OnDevice)
    x = _zeros((64, 512)).as_subclass(_OnDevice)
    cases = [(dict(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='q'), None, ('unstructured', 0, 0, 0.5, 'q')),
             (dict(w_sparsity=True, sparsity_mode='unstructured', sparsity_frac=0.5, first='s'), None, ('unstructured', 0, 0, 0.5, 's')),
             (dict(w_sparsity=True, sparsity_mode='structured', N=2, M=4, first='q'), None, ('structured', 2, 4, 0.0, 'q')),
             (dict(in_sparsity=True, sparsity_mode='structured', N=2, M=4, first='s'), ('structured', 2, 4, 0.0, 's'), None)]
    for sp, want_x, want_w in cases:
        lin = bfp_ops.BFPLinear(512, 256, bias=False, **_cfg(7, 64, **sp)).eval().enable_stochastic_matrix_unit('int8')
        del calls[:]
        with torch.no_grad():
            lin.linear_op(x, w)
        acts = [c[2] for c in calls if isinstance(c, tuple)]
        assert [None if a is None else tuple(a) for a in acts] == [want_x, want_w], sp


def test_other_forwards_stay(calls):
    """grad-enabled, 'determ', fp16 and bf16-bias forwards, and configurations outside the route, never reach it"""
    w = _zeros((256, 512)).as_subclass(_OnDevice)
    x = _zeros((64, 512)).as_subclass(_OnDevice)
    lin = bfp_ops.BFPLinear(512, 256, bias=False, **_cfg(3, 64)).eval().enable_stochastic_matrix_unit(True)
    a = lin.bfp_args
    assert bfp_ops._stoc_eligible(x, w, None, a)
    assert not bfp_ops._stoc_eligible(x, w, torch.zeros(256, dtype=torch.bfloat16), a)
    assert bfp_ops._stoc_eligible(x, w, torch.zeros(256), a)
    assert not bfp_ops._stoc_eligible(x.half(), w.half(), None, a)
    assert not bfp_ops._stoc_eligible(x.float(), w, None, a)
    assert not bfp_ops._stoc_eligible(x, w, None, dict(a, rounding_mode='determ'))
    assert not bfp_ops._stoc_eligible(x, w, None, dict(a, sparsity_num_format='int'))
    assert not bfp_ops._stoc_eligible(x, w, None, dict(a, mant_bits=8))
    assert not bfp_ops._stoc_eligible(x, w, None, dict(a, block_size=128))
    assert not bfp_ops._stoc_eligible(_zeros((64, 512)), _zeros((256, 512)), None, a)          # host tensors
    del calls[:]
    lin.linear_op(x, w)                                                                         # grad enabled: the autograd path
    assert not [c for c in calls if isinstance(c, tuple)]
    assert lin._stoc_matrix_unit.stoc_mx_calls == lin._stoc_matrix_unit.stoc_i8_calls == 0


def test_switch_values():
    lin = bfp_ops.BFPLinear(64, 16, **_cfg(3, 64))
    for bad in ('mx8', 'true', 2, None, 0.5):
        with pytest.raises(ValueError):
            lin.enable_stochastic_matrix_unit(bad)
    assert lin.enable_stochastic_matrix_unit(True)._stoc_matrix_unit.matrix_unit is True
    assert lin.enable_stochastic_matrix_unit('int8')._stoc_matrix_unit.matrix_unit == 'int8'
    assert lin.enable_stochastic_matrix_unit(False)._stoc_matrix_unit is None
    assert lin.linear_op.stoc_matrix_unit is None
    # the switch and the weight cache are independent: enabling one keeps the other
    lin.enable_stochastic_matrix_unit('int8').enable_weight_cache(matrix_unit=True)
    assert lin.linear_op.stoc_matrix_unit is lin._stoc_matrix_unit and lin.linear_op.weight_cache is lin._weight_cache
    lin.enable_stochastic_matrix_unit(True)
    assert lin.linear_op.weight_cache is lin._weight_cache and lin._weight_cache.matrix_unit is True


def _model():
    return torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 16))


def test_patch_linear_layers_switch():
    cfg = _cfg(3, 64)
    m = _model()
    with pytest.raises(ValueError):
        patch_linear_layers(m, cfg, stoc_matrix_unit='mx8')
    assert all(type(c) is not bfp_ops.BFPLinear for c in m.modules())          # validated before any module is replaced
    m = _model()
    assert patch_linear_layers(m, cfg) == ['0', '2']
    for c in m.modules():
        if isinstance(c, bfp_ops.BFPLinear):
            assert getattr(c, '_stoc_matrix_unit', None) is None and c.linear_op.stoc_matrix_unit is None
    m = _model()
    patch_linear_layers(m, cfg, stoc_matrix_unit='int8')
    mods = [c for c in m.modules() if isinstance(c, bfp_ops.BFPLinear)]
    assert len(mods) == 2 and all(c._stoc_matrix_unit.matrix_unit == 'int8' and c.linear_op.stoc_matrix_unit is c._stoc_matrix_unit
                                  for c in mods)
