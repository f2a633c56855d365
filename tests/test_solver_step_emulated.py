"""The single-iteration checks of the solver (tests/solver_step_checks.py) on the host, against tests/hip_emulation.py: the
harness, the admissibility of the chosen seeds and the bars themselves, on a machine without a GPU -- and the proof that
the checks bite: five faults seeded into a copy of the emulation's iteration, each caught by the check it is aimed at.

What the trajectory check makes of the same faults: two of them also run the check the GPU suite has had so far (11
iterations against oracle.insert_explicit, rel(dW) < 1e-4; test_solver_against_oracle_explicit_arithmetic's own problem).
Measured on the emulation: unfaulted 5.3e-7; the gradient multiplied per row by the demodulation factor once more 1.4e-2;
the demodulation term of the gradient scaled by 1 + 1e-4 (5e-6 of the gradient's norm) 1.5e-3.  It notices both here --
the factor changes from one iteration to the next, so Adam's ratio does not cancel it, and the sign-like first steps
amplify a perturbation of the gradient about 300 times.  That amplification is also why its bar cannot move: it carries the
device's own rounding (1e-7) to 5e-5 of the 1e-4 allowed, so a miss says neither which term nor which iteration, and a
defect at a few 1e-7 of the gradient is indistinguishable from rounding.  One iteration holds the same two faults at
7.7e5 and 100 times d_ref against a margin of 8, and names the measure that failed."""
import math
import types

import numpy
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests import hip_emulation
from tests import solver_reference as S
from tests import solver_step_checks as C


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_single_iteration_on_the_emulation(emulated_hip, monkeypatch, name):
    """All 20 cases, every kind: the emulation is the reference's float32 arithmetic, so every figure sits near d_ref."""
    C.assert_admissible(name)
    C.set_path(monkeypatch, name)
    for kind in C.kinds(name):
        fig, bad = C.evaluate(name, kind, C.run(name, kind, 'cpu'))
        assert not bad, (name, kind, bad, fig)


def faulted_iteration(fault):
    """hip_emulation._solve_iteration with one seeded fault (stride-1 targets with bias, no linear_insert)."""
    def iteration(s, problem, it, project):
        W = s._w
        O, I = W.shape[1:3]
        scale = 1 / math.sqrt(I * 9)
        Wg = W.clone().requires_grad_(True)
        with torch.enable_grad():
            conv = R.demod_conv(s.key[None], s.style[None], Wg, False)
            conv.retain_grad()
            out = conv + s.noise_w * s.noise.view(1, 1, *conv.shape[2:])
            out = R.fused_leaky_relu(out, s.bias)
            loss = F.l1_loss(s.val[None], out)
            if fault == 'padded_count':             # mean over the 64-padded row of positions
                positions = conv.shape[2] * conv.shape[3]
                loss = loss * (positions / (-(-positions // 64) * 64))
            loss.backward()
        s.losses[it] = loss.detach()
        dW = Wg.grad
        demod = torch.rsqrt(((scale * W * s.style.view(1, 1, I, 1, 1)) ** 2).sum([2, 3, 4]) + 1e-8)
        cot = conv.grad * demod[:, :, None, None]           # d loss / d (the scaled convolution)
        if fault == 'demod_twice':
            dW = dW * demod.view(1, O, 1, 1, 1)
        if fault == 'border_tap':                   # tap (0,0) loses the crop's top-left sample (position (1,1) reads it)
            dW = dW.clone()
            dW[0, :, :, 0, 0] -= scale * cot[0, :, 1, 1, None] * s.key[None, :, 0, 0]
        if fault == 'second_term':                  # the demodulation derivative, 1e-4 too large
            shape = types.SimpleNamespace(O=O, I=I, upsample=False)
            first = S._wgrad(shape, s.key[None], cot, torch.float32)
            dW = dW + 1e-4 * (dW - first)
        at = it - 1 if fault == 'table' else it     # the bias-correction tables read one entry early
        if s.low_rank_gradient:
            dW = R.projected_conv(dW, s.context)
        m, v = s.exp_avg, s.exp_avg_sq
        m += (dW - m) * (1 - 0.9)
        v.mul_(0.999).add_((1 - 0.999) * dW * dW)
        W += (-s.step_size[at] * m) / (v.sqrt() / s.bc2_sqrt[at] + 1e-8)
        if project:
            W.copy_(s.ortho + R.projected_conv(W, s.context))
    return iteration


# fault -> (case, kind, the checks that must fail)
FAULTS = {
    'demod_twice': ('S2', 'cold', {'m.row', 'm.elem', 'v.row', 'v.elem'}),
    'border_tap': ('S2', 'cold', {'m.elem', 'v.elem'}),
    'padded_count': ('S2', 'cold', {'loss', 'm.row', 'v.row'}),
    'table': ('S2', 'warm', {'x.row', 'x.elem', 'adam'}),
    'second_term': ('S2', 'cold', {'m.row'}),
}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_a_seeded_fault_fails_the_check_aimed_at_it(emulated_hip, monkeypatch, fault):
    name, kind, aimed = FAULTS[fault]
    C.set_path(monkeypatch, name)
    fig, bad = C.evaluate(name, kind, C.run(name, kind, 'cpu'))
    assert not bad, (bad, fig)                      # the same run without the fault holds every bar
    monkeypatch.setattr(hip_emulation, '_solve_iteration', faulted_iteration(fault))
    fig, bad = C.evaluate(name, kind, C.run(name, kind, 'cpu'))
    print(fault, sorted(bad), fig)
    assert aimed <= set(bad), (fault, sorted(bad), fig)
    if fault == 'table':                            # ... and only the arithmetic after the moments: they read no table
        assert not {'m.row', 'm.elem', 'v.row', 'v.elem', 'loss'} & set(bad), bad


def _trajectory_rel():
    """test_solver_against_oracle_explicit_arithmetic's problem and bar, 11 iterations, on the installed emulation."""
    from rewriting_amd.rewrite import hipsolve
    rs = numpy.random.RandomState(4)
    O = I = 128
    h, w = 6, 11
    W0 = torch.from_numpy(rs.randn(1, O, I, 3, 3).astype('float32'))
    key = torch.from_numpy(rs.randn(1, I, h, w).astype('float32'))
    style = torch.from_numpy((1 + 0.3 * rs.randn(1, I)).astype('float32'))
    val = torch.from_numpy(rs.randn(1, O, h, w).astype('float32'))
    bias = torch.from_numpy((0.1 * rs.randn(O)).astype('float32'))
    nw = torch.tensor([0.1])
    ctx = torch.linalg.qr(torch.from_numpy(rs.randn(I, 2).astype('float32')))[0].t().contiguous()
    Wd = W0.clone()
    hipsolve.run(Wd, key, style, val, bias, nw, ctx, niter=11, piter=10, lr=0.05, low_rank_insert=True,
                 low_rank_gradient=False)
    _, _, snaps = R.insert_explicit(W0, key, style, val, bias, nw, ctx, niter=11, piter=10, snapshots=(11,))
    return ((Wd - W0).double() - (snaps[11] - W0).double()).norm().item() / (snaps[11] - W0).double().norm().item()


def test_what_the_trajectory_check_makes_of_two_of_the_faults(emulated_hip, monkeypatch):
    """The figures of the module docstring, printed; asserted is only what cannot move: the unfaulted emulation holds the
    trajectory bar, and each fault moves the trajectory away from it."""
    monkeypatch.setenv('RW_SOLVE_ONE_LAUNCH', '0')
    clean = _trajectory_rel()
    seen = {}
    for fault in ('demod_twice', 'second_term'):
        monkeypatch.setattr(hip_emulation, '_solve_iteration', faulted_iteration(fault))
        seen[fault] = _trajectory_rel()
    print('trajectory rel: clean %.2e' % clean, {k: '%.2e' % v for k, v in seen.items()})
    assert clean < 1e-4
    assert all(v > clean for v in seen.values()), seen
