"""BFPAdam with the reference's name and module path (src/transformers/bfp/bfp_optim_lstm.py:12-93): Adam whose
freshly updated parameters are snapped to the wide-mantissa HBFP grid -- float_to_bfp_blocked(p, sgd_update=True),
i.e. `weight_mant_bits` instead of `mant_bits`, no sparsity (identifier '') -- so that weights are stored at HBFP16
precision between steps.  The moment math is plain Adam; only the snap runs in the BFP engine.

fused=True (opt-in): the fp32 ROCm parameters of a step go through ONE launch per 64 tensors (native.AdamStepList:
moments, update and snap in one pass, bit for bit the loop's result on the same GPU); every other parameter takes the
loop below unchanged.  plan_step() decides which is which."""
import math
import numbers

import torch

from . import bfp_ops
from .. import native
from .bfp_util import get_bfp_args

required = object()


def _snap_of(bfp_args):
    """(takes, block_size, mant_bits, stoch) of a configuration for the fused step: takes is False where the loop must run it
    ('int', block_size 0, a rounding mode or width the kernel does not take); block_size 0 with takes: no snap"""
    fmt = bfp_args['num_format']
    if fmt == 'fp32' or (fmt == 'bfp' and bfp_args['sparsity_num_format'] == 'fp32'):
        return True, 0, 0, False
    if fmt != 'bfp' or bfp_args['sparsity_num_format'] != 'bfp' or bfp_args['rounding_mode'] not in bfp_ops.rounding_modes.modes:
        return False, 0, 0, False
    bs, mb = int(bfp_args['block_size']), int(bfp_args['weight_mant_bits'])
    if not (bs > 0 and 1 <= mb <= 23 and native.adam_snap_ok(bs, mb)):
        return False, 0, 0, False
    return True, bs, mb, bfp_args['rounding_mode'] == bfp_ops.rounding_modes.STOC


def _is_number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, (bool, torch.Tensor))


def _fusable(p, group, state):
    """None if parameter p of `group` can take the fused step, else the reason it takes the loop"""
    g = p.grad
    if p.device.type != 'cuda':
        return 'not on a ROCm device'
    if p.dtype != torch.float32 or g.dtype != torch.float32:
        return 'not fp32'
    if g.is_sparse or g.layout != torch.strided:
        return 'sparse grad'
    if not p.is_contiguous() or not g.is_contiguous():
        return 'not contiguous'
    if g.data_ptr() == p.data_ptr() and p.numel():
        return 'grad aliases the parameter'
    if not all(_is_number(x) for x in (group['lr'], group['betas'][0], group['betas'][1], group['eps'], group['weight_decay'])):
        return 'hyperparameter is not a Python number'
    if len(state):
        keys = ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq',) if group['amsgrad'] else ())
        if not isinstance(state.get('step'), int) or any(k not in state for k in keys):
            return 'state not made by BFPAdam'
        for k in keys:
            s = state[k]
            if s.device != p.device or s.dtype != torch.float32 or not s.is_contiguous() or s.shape != p.shape:
                return 'state not contiguous fp32'
    return None


def plan_step(param_groups, state, bfp_args, injected=False):
    """The split of one fused step, in the loop's order: per group, the list of (p, reason) for the parameters with a grad --
    reason None: the fused launch takes it, else why the loop does.  Pure: reads the parameters, grads and states only."""
    takes, _, _, _ = _snap_of(bfp_args)
    plan = []
    for group in param_groups:
        rows = []
        for p in group['params']:
            if p.grad is None:
                continue
            if injected:
                rows.append((p, 'quantize_fn injected'))
            elif not takes:
                rows.append((p, 'configuration not taken by the fused step'))
            else:
                rows.append((p, _fusable(p, group, state.get(p, {}))))
        plan.append(rows)
    return plan


def step_size_of(lr, beta1, beta2, step):
    """the loop's step size at `step` (bfp_optim_lstm.py:76-78), a Python double"""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return lr * math.sqrt(bc2) / bc1


class BFPAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 bfp_args=None, quantize_fn=None, fused=False):
        """bfp_args: the `hbfp` config dict (default: bfp_util.get_bfp_args(), like the reference, :15).
        quantize_fn: callable with float_to_bfp_blocked's signature (default: the HIP engine; tests may inject a CPU checker).
        fused: run the fp32 ROCm parameters through the fused list kernel (same result, see the module docstring).  Not torch's
        own `fused` flag, which is not passed on."""
        self.bfp_args = dict(bfp_args) if bfp_args is not None else get_bfp_args()
        self._injected = quantize_fn is not None
        self._quantize = quantize_fn or bfp_ops.float_to_bfp_blocked
        self.fused = bool(fused)
        self.fused_tensors = 0                  # parameters the last step ran through the fused launch
        self.loop_tensors = 0                   # ... and through the loop
        self._lists = {}                        # (group index, device) -> (ids of the bound parameters, native.AdamStepList)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)

    def _loop_param(self, p, group, fmt, known):
        """one parameter of the reference's loop (bfp_optim_lstm.py:38-87)"""
        grad = p.grad
        if grad.is_sparse:
            raise RuntimeError('Adam does not support sparse gradients, please consider SparseAdam instead')
        beta1, beta2 = group['betas']
        state = self.state[p]
        if len(state) == 0:                                     # reference :45-53
            state['step'] = 0
            state['exp_avg'] = torch.zeros_like(p)
            state['exp_avg_sq'] = torch.zeros_like(p)
            if group['amsgrad']:
                state['max_exp_avg_sq'] = torch.zeros_like(p)
        state['step'] += 1
        if group['weight_decay'] != 0:
            grad = grad.add(p, alpha=group['weight_decay'])     # :62-63
        m, v = state['exp_avg'], state['exp_avg_sq']
        m.mul_(beta1).add_(grad, alpha=1 - beta1)               # :66
        v.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)     # :67
        if group['amsgrad']:
            torch.max(state['max_exp_avg_sq'], v, out=state['max_exp_avg_sq'])   # :70
            denom = state['max_exp_avg_sq'].sqrt().add_(group['eps'])
        else:
            denom = v.sqrt().add_(group['eps'])                 # :74
        bc1 = 1 - beta1 ** state['step']
        bc2 = 1 - beta2 ** state['step']
        step_size = group['lr'] * math.sqrt(bc2) / bc1          # :76-78
        p.addcdiv_(m, denom, value=-step_size)                  # :82 / :85
        if fmt == 'bfp':
            p.copy_(self._quantize(p, sgd_update=True, **known))   # :85-87

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        fmt = self.bfp_args['num_format']
        if fmt not in ('fp32', 'bfp'):
            raise NotImplementedError('NumFormat not implemented')
        known = bfp_ops.unpack_bfp_args(dict(self.bfp_args))            # float_to_bfp_blocked takes exactly the 20 known keys
        if self.fused:
            self._fused_step(fmt, known)
            return loss
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is not None:
                    self._loop_param(p, group, fmt, known)
        return loss

    def _fused_step(self, fmt, known):
        """plan, seeds, launch: the fused parameters' states advance as the loop's would, a 'stoc' seed is drawn per snapped
        parameter in the loop's order (a loop parameter's own seed is handed to its snap through _replay_seeds)"""
        _, block_size, mant_bits, stoch = _snap_of(self.bfp_args)
        plan = plan_step(self.param_groups, self.state, self.bfp_args, self._injected)
        # a loop parameter whose snap draws a 'stoc' seed (on a ROCm device, 'bfp' into 'bfp' with a block): the draw is in order
        draws = (fmt == 'bfp' and self.bfp_args['sparsity_num_format'] == 'bfp' and self.bfp_args['block_size'] > 0
                 and self.bfp_args['rounding_mode'] == bfp_ops.rounding_modes.STOC)
        n_fused = n_loop = 0
        launches, loops = [], []
        for gi, (group, rows) in enumerate(zip(self.param_groups, plan)):
            beta1, beta2 = group['betas']
            per_dev = {}
            for p, why in rows:
                if why is not None:
                    seed = bfp_ops._seed_for(bfp_ops.rounding_modes.STOC) if draws and p.device.type == 'cuda' else None
                    loops.append((p, group, seed))
                    n_loop += 1
                    continue
                state = self.state[p]
                if len(state) == 0:                              # as the loop makes it
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p)
                    state['exp_avg_sq'] = torch.zeros_like(p)
                    if group['amsgrad']:
                        state['max_exp_avg_sq'] = torch.zeros_like(p)
                state['step'] += 1
                seed = bfp_ops._seed_for(bfp_ops.rounding_modes.STOC) if stoch else 0
                slot = (p, p.grad, state['exp_avg'], state['exp_avg_sq'], state.get('max_exp_avg_sq') if group['amsgrad'] else None)
                per_dev.setdefault(p.device, []).append((slot, step_size_of(group['lr'], beta1, beta2, state['step']), seed))
                n_fused += 1
            for dev, items in per_dev.items():
                launches.append((gi, group, dev, items))
        for gi, group, dev, items in launches:
            ids = tuple(id(s[0]) for s, _, _ in items)
            key = (gi, dev)
            hp = (tuple(group['betas']), group['eps'], group['weight_decay'], group['amsgrad'], block_size, mant_bits, stoch, known['epsilon'])
            bound = self._lists.get(key)
            if bound is None or bound[0] != ids or bound[1] != hp:
                bound = (ids, hp, native.AdamStepList([s for s, _, _ in items], group['betas'], group['eps'], group['weight_decay'],
                                                      group['amsgrad'], block_size, mant_bits, stoch, known['epsilon']))
                self._lists[key] = bound
            bound[2].run([s for s, _, _ in items], [z for _, z, _ in items], [sd for _, _, sd in items] if stoch else None)
        for p, group, seed in loops:
            if seed is None:
                self._loop_param(p, group, fmt, known)
            else:
                with bfp_ops._replay_seeds((seed,)):
                    self._loop_param(p, group, fmt, known)
        self.fused_tensors, self.loop_tensors = n_fused, n_loop
