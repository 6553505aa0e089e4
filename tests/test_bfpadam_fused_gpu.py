"""BFPAdam(fused=True) on the GPU: every step bit for bit equal to the loop (fused=False) on the same GPU -- parameters, both moments
and amsgrad's running max -- over block sizes, widths, rounding modes, amsgrad, weight decay, ragged rows, missing and late grads,
several groups, NaN / inf, mixed lists that partly fall back, state_dict round trips, and the G10 fixtures of the reference."""
import numpy as np
import pytest
import torch

from quantization_sparsity_interplay_amd import native
from quantization_sparsity_interplay_amd.bfp.bfp_optim_lstm import BFPAdam
from util import load, from_bits, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(64, 128), (96,), (1,), (33, 65), (768, 3072), (64, 3, 7, 7), (256, 64, 1, 1)]


def cfg(**kw):
    c = dict(mant_bits=7, epsilon=1e-8, rounding_mode='determ', device='cpu', block_size=32, num_format='bfp',
             weight_mant_bits=15, in_sparsity=False, w_sparsity=False, grad_sparsity=False, sparsity_frac=0.5, N=2, M=4,
             sparsity_num_format='bfp', first='s', sparsity_mode='structured')
    c.update(kw)
    return c


def _params(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(DEV)) for s in shapes]


def _grads(shapes, step, seed=100):
    g = torch.Generator().manual_seed(seed + step)
    return [torch.randn(s, generator=g) * 0.01 for s in shapes]


def _state_bits(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append([bits(p)] + [bits(st[k]) for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq') if k in st])
    return out


def _run(fused, shapes, steps=5, groups=None, grad_mask=None, edit_grad=None, dtypes=None, **opt_kw):
    """`steps` steps of BFPAdam from the same start: (per step the bit images of every p and its states, the optimizer, the CPU RNG
    state after).  grad_mask(step, i) False: parameter i has no grad at that step; edit_grad(step, i, g): the grad to set instead"""
    torch.manual_seed(1234)
    params = _params(shapes)
    if dtypes:
        params = [torch.nn.Parameter(p.detach().to(dt)) if dt is not None else p for p, dt in zip(params, dtypes)]
    pg = params if groups is None else [dict(params=[params[i] for i in idx], **kw) for idx, kw in groups]
    opt = BFPAdam(pg, fused=fused, **opt_kw)
    snaps = []
    for step in range(steps):
        for i, (p, g) in enumerate(zip(params, _grads(shapes, step))):
            if grad_mask is not None and not grad_mask(step, i):
                p.grad = None
                continue
            g = g.to(DEV).to(p.dtype)
            p.grad = edit_grad(step, i, g) if edit_grad is not None else g
        opt.step()
        torch.cuda.synchronize()
        snaps.append(_state_bits(opt, params))
    return snaps, opt, torch.get_rng_state()


def _same(a, b):
    assert len(a) == len(b)
    for step, (sa, sb) in enumerate(zip(a, b)):
        for i, (ta, tb) in enumerate(zip(sa, sb)):
            assert len(ta) == len(tb), (step, i)
            for k, (x, y) in enumerate(zip(ta, tb)):
                assert np.array_equal(x, y), f"step {step}, parameter {i}, array {k}: {int((x != y).sum())} of {x.size} differ"


def _check(shapes, n_fused=None, **kw):
    want, _, rng_a = _run(False, shapes, **kw)
    got, opt, rng_b = _run(True, shapes, **kw)
    _same(want, got)
    assert torch.equal(rng_a, rng_b), "the CPU generator is not where the loop leaves it"
    if n_fused is not None:
        assert opt.fused_tensors == n_fused
    return opt


@pytest.mark.parametrize("block", [16, 32, 64])
@pytest.mark.parametrize("mant", [15, 7])
@pytest.mark.parametrize("mode", ['determ', 'stoc'])
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0, 0.01])
def test_fused_equals_loop(block, mant, mode, amsgrad, wd):
    _check(SHAPES, n_fused=len(SHAPES), lr=1e-2, amsgrad=amsgrad, weight_decay=wd,
           bfp_args=cfg(block_size=block, weight_mant_bits=mant, rounding_mode=mode))


@pytest.mark.parametrize("args", [dict(num_format='fp32'), dict(sparsity_num_format='fp32')], ids=["fp32", "bfp_fp32"])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_fused_without_snap(args, amsgrad):
    _check(SHAPES, n_fused=len(SHAPES), lr=1e-2, amsgrad=amsgrad, weight_decay=0.01, bfp_args=cfg(rounding_mode='stoc', **args))


@pytest.mark.parametrize("mode", ['determ', 'stoc'])
def test_missing_and_late_grads_two_groups(mode):
    # parameter 1 never gets a grad, parameter 3 only from step 3 on (its step count lags the others' in the same launch)
    mask = lambda step, i: i != 1 and (i != 3 or step >= 2)  # noqa: E731
    groups = [([0, 1, 2, 3], dict(lr=1e-2)), ([4, 5, 6], dict(lr=3e-3))]
    opt = _check(SHAPES, groups=groups, grad_mask=mask, amsgrad=True, bfp_args=cfg(rounding_mode=mode))
    assert opt.fused_tensors == len(SHAPES) - 1 and opt.loop_tensors == 0
    assert opt.state[opt.param_groups[0]['params'][3]]['step'] == 3


@pytest.mark.parametrize("mode", ['determ', 'stoc'])
def test_nan_and_inf_in_one_grad_block(mode):
    def edit(step, i, g):
        if i == 0 and step == 1:
            g = g.clone()
            g.view(-1)[5], g.view(-1)[9] = float('nan'), float('inf')
        if i == 4 and step == 2:
            g = g.clone()
            g.view(-1)[100] = float('-inf')
        return g
    _check(SHAPES, n_fused=len(SHAPES), edit_grad=edit, lr=1e-2, bfp_args=cfg(rounding_mode=mode))


@pytest.mark.parametrize("mode", ['determ', 'stoc'])
def test_mixed_list_falls_back_per_tensor(mode):
    # parameter 1 is bf16, parameter 0's grad is a non-contiguous view: both take the loop, the rest the fused launch
    def edit(step, i, g):
        return g.t().contiguous().t() if i == 0 else g
    dtypes = [None, torch.bfloat16] + [None] * (len(SHAPES) - 2)
    opt = _check(SHAPES, dtypes=dtypes, edit_grad=edit, lr=1e-2, bfp_args=cfg(rounding_mode=mode))
    assert opt.fused_tensors == len(SHAPES) - 2 and opt.loop_tensors == 2


def _save_load_run(first_fused, mode):
    """2 steps with fused=first_fused, state_dict() into a new fused=False optimizer, 2 more steps.  (torch.optim.Adam's
    __setstate__ turns a loaded 'step' into a float tensor, which changes the loop's step-size arithmetic: the yardstick makes the
    same round trip.)"""
    torch.manual_seed(1234)
    params = _params(SHAPES)
    opt = BFPAdam(params, fused=first_fused, amsgrad=True, lr=1e-2, bfp_args=cfg(rounding_mode=mode))
    out = []
    for step in range(4):
        if step == 2:
            sd = opt.state_dict()
            opt = BFPAdam(params, fused=False, amsgrad=True, lr=1e-2, bfp_args=cfg(rounding_mode=mode))
            opt.load_state_dict(sd)
        for p, g in zip(params, _grads(SHAPES, step)):
            p.grad = g.to(DEV)
        opt.step()
        torch.cuda.synchronize()
        out.append(_state_bits(opt, params))
    return out, torch.get_rng_state()


@pytest.mark.parametrize("mode", ['determ', 'stoc'])
def test_state_dict_from_fused_continues_in_the_loop(mode):
    want, rng_a = _save_load_run(False, mode)
    got, rng_b = _save_load_run(True, mode)
    _same(want, got)
    assert torch.equal(rng_a, rng_b)


@pytest.mark.parametrize("tag,amsgrad", [("plain", False), ("ams", True)])
def test_g10_fixtures(tag, amsgrad):
    g = load("g10_bfpadam.npz")
    res = {}
    for fused in (False, True):
        params = [torch.nn.Parameter(from_bits(g[f"{tag}_p0_init"], torch.float32).view(64, 128).to(DEV)),
                  torch.nn.Parameter(from_bits(g[f"{tag}_p1_init"], torch.float32).view(96).to(DEV))]
        opt = BFPAdam(params, lr=1e-2, amsgrad=amsgrad, bfp_args=cfg(), fused=fused)
        out = []
        for step in range(3):
            for i, p in enumerate(params):
                p.grad = from_bits(g[f"{tag}_g{i}_s{step}"], torch.float32).view(p.shape).to(DEV)
            opt.step()
            out.append([p.detach().cpu().clone() for p in params])
        res[fused] = out
        if fused:
            assert opt.fused_tensors == 2
    for step in range(3):
        for i in range(2):
            want = from_bits(g[f"{tag}_p{i}_s{step}"], torch.float32).view(res[True][step][i].shape)
            got = res[True][step][i]
            assert float((got - want).abs().max()) <= 2.0 ** -15                # the bound test_bfpadam_gpu holds the loop to
            assert float((got == want).float().mean()) > 0.97
            assert torch.equal(got.view(torch.int32), res[False][step][i].view(torch.int32))


def test_200_small_tensors_take_at_most_4_launches():
    shapes = [(8 + i % 5, 16 + 4 * (i % 3)) for i in range(200)]
    before = native.adam_launches
    opt = _check(shapes, steps=2, lr=1e-2, bfp_args=cfg())
    assert opt.fused_tensors == 200
    assert native.adam_launches - before <= 2 * 4
