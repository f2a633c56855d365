"""TEST INFRASTRUCTURE -- the single-iteration checks of the solver, shared by the GPU test (tests/test_gpu_solver_step.py)
and by its host twin on the emulation (tests/test_solver_step_emulated.py).

A case is one target shape, one mode and one kernel path.  Three runs of ONE iteration each:

* cold   it = 0, m = v = 0, no projection: the loss, exp_avg = 0.1 g, exp_avg_sq = 0.001 g^2;
* warm   it = 7 of 12 with seeded moments (teacher-forced): m', v', W' (Lambda' for linear_insert), the loss slot, the counter;
* proj   it = 0 with low_rank_insert, which projects there: W = ortho + P(Adam result).

Where each bar comes from:

* measured against the float32 host run of the same reference (d_ref), with the margin of 8 that
  test_whole_generator_gradients_against_the_float64_oracle uses: every ``row`` and ``elem`` figure, d_hip <= 8 d_ref, both
  of that case and that measure.  ``row`` is the worst relative L2 error of an out-channel row (one bad row cannot hide in a
  global norm); ``elem`` the worst element error over that element's float64 sum of magnitudes (one bad tap or border
  position cannot hide in a row norm).  The loss: |l - l64| <= max(8 |l32 - l64|, 2^-22 l64); the floor is one rounding of
  the final sum and two of the mean, for the cases where |l32 - l64| is near zero by luck.
* derived: the Adam arithmetic, see ``adam_bound``.
* taken from test_projection_kernel: rel < 1e-5 for the projected weight.
"""
import functools
import types

import torch

from oracle import restatement as R
from tests import solver_reference as S

NITER, PITER, WARM_IT = 12, 10, 7
MARGIN = 8


def _case(O, I, h, w, path, rank=0, up=False, plain=False, lrg=False, linear=False, force_stream=False, seed=0):
    return types.SimpleNamespace(O=O, I=I, h=h, w=w, path=path, rank=rank, up=up, plain=plain, lrg=lrg, linear=linear,
                                 force_stream=force_stream, seed=seed)


# seed: the first of 0, 1, 2, ... at which the nearest position is 64 float32 deviations from the leaky ReLU's kink at every
# weight the case evaluates -- four times what solver_reference.admissible demands, because the device's rounding is not
# the host's; found on the host.  Admissibility itself is asserted by every test before anything is launched.
CASES = {
    # the step kernels
    'S1': _case(64, 16, 1, 1, 'step'),                          # one position in a 64-padded row; 9 K-chunks clamp split-K
    'S2': _case(64, 48, 3, 5, 'step', rank=2),                  # in_ch % 64 != 0, odd crop
    'S3': _case(128, 80, 5, 13, 'step', rank=1, seed=5),              # 65 positions: the second block holds one; 45 chunks / 32
    'S4': _case(64, 896, 2, 2, 'step', rank=1, lrg=True),       # in_ch at the projection's LDS limit
    'S5': _case(64, 32, 3, 4, 'step', up=True, seed=1),             # pre-blur map 7 x 9 = 63 < 64; blur and its adjoint
    'S6': _case(64, 16, 4, 4, 'step', up=True),                 # 9 x 9 = 81 > 64
    'S7': _case(64, 32, 3, 4, 'step', up=True, plain=True),     # val on the (2h+1) x (2w+1) map
    'S8': _case(64, 64, 4, 4, 'step', rank=8, plain=True, lrg=True),
    'S9': _case(64, 64, 4, 4, 'step', rank=3, linear=True),     # project_kernel<2>, Lambda's state
    'S10': _case(192, 64, 2, 3, 'step', seed=1),                # three out-channel blocks
    # one launch, the crop resident in the LDS
    'R1': _case(64, 64, 1, 1, 'resident'),                      # smallest launch (64 threads)
    'R2': _case(64, 192, 3, 17, 'resident', rank=2),            # odd width
    'R3': _case(64, 512, 5, 8, 'resident', rank=1),             # the full-size edit's shape class, 512 threads
    'R4': _case(64, 128, 7, 1, 'resident', rank=2, lrg=True),   # one column
    'R5': _case(64, 256, 4, 4, 'resident', rank=8, plain=True, lrg=True),       # rank at its cap
    # one launch, the crop streamed
    'T1': _case(64, 512, 8, 9, 'streamed', rank=1),             # streamed by necessity
    'T2': _case(64, 128, 7, 1, 'streamed', rank=2, force_stream=True),
    'T3': _case(64, 192, 3, 16, 'streamed', rank=2, lrg=True, force_stream=True),   # gradient from the d_r^T key maps
    'T4': _case(64, 512, 16, 16, 'streamed', rank=1, plain=True, lrg=True),     # the erase's whole-map class
    'T5': _case(64, 256, 13, 15, 'streamed', rank=1, plain=True),
}


def set_path(monkeypatch, name):
    c = CASES[name]
    monkeypatch.setenv('RW_SOLVE_ONE_LAUNCH', '0' if c.path == 'step' else '1')
    if c.force_stream:
        monkeypatch.setenv('RW_SOLVE_STREAM', '1')
    else:
        monkeypatch.delenv('RW_SOLVE_STREAM', raising=False)


@functools.lru_cache(maxsize=None)
def problem(name):
    c = CASES[name]
    return S.make_problem(c.O, c.I, c.h, c.w, c.rank, c.up, c.plain, c.seed)


def _state_shape(name):
    c = CASES[name]
    return (c.O, c.rank, 9) if c.linear else (1, c.O, c.I, 3, 3)


@functools.lru_cache(maxsize=None)
def start(name, kind):
    """(W, m, v, lam) an iteration of this kind starts from: float32, shared, never modified."""
    c, p = CASES[name], problem(name)
    shape = _state_shape(name)
    if kind != 'warm':
        z = torch.zeros(shape)
        return p.W0, z, z, (z if c.linear else None)
    g = references(name, 'cold')[0].g
    rms = g.pow(2).mean().sqrt().item()
    gen = torch.Generator().manual_seed(1000 + c.seed)
    m = (rms * torch.randn(shape, generator=gen)).float()
    v = (rms ** 2 * (0.5 + 1.5 * torch.rand(shape, generator=gen))).float()
    if not c.linear:
        return p.W0, m, v, None
    lam = 0.01 * torch.randn(shape, generator=gen)
    W = p.W0 + torch.einsum('ody,di->oiy', lam, p.context).reshape(p.W0.shape)
    return W, m, v, lam


@functools.lru_cache(maxsize=None)
def references(name, kind):
    """(float64, float32) reference of the iteration: computed once, shared, never modified."""
    c, p = CASES[name], problem(name)
    W, m, v, lam = start(name, kind)
    it = WARM_IT if kind == 'warm' else 0
    return tuple(S.reference_iteration(p, W, m, v, it, low_rank_gradient=c.lrg, linear=c.linear, lam=lam, dtype=dt)
                 for dt in (torch.float64, torch.float32))


def kinds(name):
    """every case does cold and warm; the projection where there is one on the iteration (not rank 0, not linear)"""
    c = CASES[name]
    return ('cold', 'warm', 'proj') if (c.rank and not c.linear) else ('cold', 'warm')


def assert_admissible(name):
    """The leaky ReLU decides every position the same way in float32 and in float64, at every weight the case evaluates:
    asserted before anything is launched, so that no case can pass by skipping positions."""
    p = problem(name)
    for kind in ('cold', 'warm'):
        W = start(name, kind)[0]
        nearest, dev = S.undecided(p, W)
        assert nearest > 16 * dev, (name, kind, nearest, dev)
    assert (references(name, 'cold')[0].pre is None) == p.plain


def run(name, kind, device):
    """One iteration of ``kind`` through hipsolve.Solver on ``device``; what it left, on the host."""
    from rewriting_amd import hip
    from rewriting_amd.rewrite import hipsolve
    c, p = CASES[name], problem(name)
    W, m, v, lam = start(name, kind)

    def dev(t):
        return None if t is None else t.to(device)
    constrained = c.rank > 0
    assert hip.solve_supported(c.O, c.I, c.h, c.w, c.up, c.plain, constrained)
    if c.path != 'step':
        assert hip.solve_run_supported(c.O, c.I, c.h, c.w, c.rank, c.up, c.linear)
    Wd = p.W0.clone().to(device)
    s = hipsolve.Solver(Wd, dev(p.key), dev(p.style), dev(p.val), dev(p.bias), dev(p.noise_w), dev(p.context), NITER, PITER,
                        S.LR, constrained and not c.linear, c.lrg, blur_kernel=dev(p.blur_k), linear=c.linear, upsample=c.up)
    # the path: what the driver decided and recorded, and (one launch) which of its two kernels the library sized for
    assert s.one_launch == (c.path != 'step')
    assert hipsolve.LAST['one_launch'] == (c.path != 'step')
    assert (hipsolve.LAST['out_ch'], hipsolve.LAST['in_ch'], hipsolve.LAST['h'], hipsolve.LAST['w']) == (c.O, c.I, c.h, c.w)
    if s.one_launch:
        crop_copy = s.lpart.numel() - (NITER * c.O + 3) // 4 * 4       # the streamed kernel's copy of the crop
        assert (crop_copy > 0) == (c.path == 'streamed'), (name, crop_copy)
    n = m.numel()
    if kind == 'warm':
        s.exp_avg.view(-1)[:n].copy_(m.reshape(-1))
        s.exp_avg_sq.view(-1)[:n].copy_(v.reshape(-1))
        if c.linear:
            s.lam.copy_(lam)
            Wd.copy_(W)
    it = WARM_IT if kind == 'warm' else 0
    project = kind == 'proj'
    if s.one_launch:
        s.run_range(it, it + 1, project=project)
    else:
        s.counter.fill_(it - 1)
        s.step(it, project=project)
    shape = _state_shape(name)
    return types.SimpleNamespace(
        losses=s.losses.cpu().clone(), counter=int(s.counter.item()), W=Wd.cpu().clone(),
        m=s.exp_avg.view(-1)[:n].view(shape).cpu().clone(), v=s.exp_avg_sq.view(-1)[:n].view(shape).cpu().clone(),
        lam=s.lam.cpu().clone() if c.linear else None,
        step_size=s.step_size[it].item(), bc2_sqrt=s.bc2_sqrt[it].item(), eps=s.problem.eps, it=it)


# ------------------------------------------------------------------------------------------------ measures
def row_error(got, want, rows, scale=None):
    """worst relative L2 error of a row; ``scale``: what the rows' norms are taken of instead of ``want``"""
    d = (got.double() - want).reshape(rows, -1).norm(dim=1)
    n = (want if scale is None else scale).reshape(rows, -1).norm(dim=1)
    return (d / n).max().item()


def elem_error(got, want, mag):
    return ((got.double() - want).abs() / mag).max().item()


def adam_bound(x_new, update):
    """What the device's weight may differ by from the update formula evaluated in float64 on the device's OWN m', v' and
    the float32 table entries.  The formula is w' = w + update, update = -(step_size m) / (sqrt(v) / bc2_sqrt + eps).
    Every float32 operation returns its exact result times (1 + d), |d| <= 2^-24.  The update passes through five: the
    product, the square root, the quotient by bc2_sqrt, the sum with eps, the last quotient; to first order each enters
    the update's relative error once, the three of the denominator with a weight <= 1.  The final sum rounds once more:
    2^-24 |w'|.  Worst case, all at their extreme and of one sign: 2^-24 |w'| + 5 * 2^-24 |update|.
    The bar is 2^-23 |w'| + 4 * 2^-24 |update| = that worst case + 2^-24 (|w'| - |update|): it holds the worst case
    wherever |w'| >= |update| (nearly every element: |update| <= lr = 0.05), and where |w'| is smaller it falls short of
    the worst case by at most 2^-24 |update| -- reached only with all five roundings within a fifth of their extreme and
    of one sign.  A wrong table entry, eps or order of operations is off by 1e-3 and more of the update, 10^4 times the
    bar.  No measurement enters it."""
    return 2.0 ** -23 * x_new.abs() + 4 * 2.0 ** -24 * update.abs()


def evaluate(name, kind, got):
    """(figures, names of the checks that fail) for what ``run`` returned."""
    c, p = CASES[name], problem(name)
    ref, f32 = references(name, 'cold' if kind == 'proj' else kind)
    W0, m0, v0, lam0 = start(name, kind)
    rows = c.O
    fig, bad = {}, []

    def hold(check, ok):
        if not ok:
            bad.append(check)

    # bookkeeping: the loss slot of this iteration and no other, the counter of the step path
    others = torch.cat([got.losses[:got.it], got.losses[got.it + 1:]])
    hold('bookkeeping', got.losses[got.it].item() != 0 and bool((others == 0).all())
         and (c.path != 'step' or got.counter == got.it))
    x0 = (lam0 if c.linear else W0).double()
    x_dev = got.lam if c.linear else got.W
    # the Adam arithmetic alone, on the device's own moments
    denom = got.v.double().sqrt() / got.bc2_sqrt + got.eps
    update = -(got.step_size * got.m.double()) / denom
    x_adam = x0 + update
    if kind == 'proj':
        ctx = p.context.double()
        ortho = W0.double() - R.projected_conv(W0.double(), ctx)
        want = ortho + R.projected_conv(x_adam, ctx)
        fig['proj_rel'] = ((got.W.double() - want).norm() / want.norm()).item()
        hold('proj', fig['proj_rel'] < 1e-5)
        return fig, bad
    excess = ((x_dev.double() - x_adam).abs() / adam_bound(x_adam, update)).max().item()
    fig['adam_excess'] = excess                   # worst |difference| / bound
    hold('adam', excess <= 1)
    # the loss
    d_hip, d_ref = abs(got.losses[got.it].item() - ref.loss), abs(f32.loss - ref.loss)
    fig['loss'] = dict(d_hip=d_hip / ref.loss, d_ref=d_ref / ref.loss, ratio=d_hip / max(d_ref, 2.0 ** -22 * ref.loss / MARGIN))
    hold('loss', d_hip <= max(MARGIN * d_ref, 2.0 ** -22 * ref.loss))
    # the moments, and for a warm iteration what Adam made of them
    one = 1 - S.BETA1, 1 - S.BETA2
    mag_m = S.BETA1 * m0.double().abs() + one[0] * ref.mag
    mag_v = S.BETA2 * v0.double().abs() + one[1] * ref.mag ** 2
    things = [('m', got.m, ref.m, f32.m, mag_m, None), ('v', got.v, ref.v, f32.v, mag_v, None)]
    if kind == 'warm':
        x64 = ref.lam if c.linear else ref.W
        x32 = f32.lam if c.linear else f32.W
        step_size, bc2_sqrt = S.tables(got.it)
        den64 = ref.v.sqrt() / bc2_sqrt + S.EPS
        mag_x = x0.abs() + step_size * mag_m / den64 + 0.5 * (x64 - x0).abs() * mag_v / ref.v
        things.append(('x', x_dev, x64, x32, mag_x, x64 - x0))
        if c.linear:
            things.append(('W', got.W, ref.W, f32.W, None, ref.W - W0.double()))
    for what, dev, want, host, mag, scale in things:
        measures = [('row', row_error(dev, want, rows, scale), row_error(host, want, rows, scale))]
        if mag is not None:
            measures.append(('elem', elem_error(dev, want, mag), elem_error(host, want, mag)))
        for measure, d_hip, d_ref in measures:
            fig['%s.%s' % (what, measure)] = dict(d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref)
            hold('%s.%s' % (what, measure), d_hip <= MARGIN * d_ref)
    return fig, bad
