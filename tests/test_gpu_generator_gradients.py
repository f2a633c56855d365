"""Gradients from the image on the device: the two ToRGB kernels of rw_grad.hip against float64 einsums, the whole
generator's gradients and ``all_weights_insert`` against float64 autograd over oracle/restatement.py on the host.
Figures go to generator_gradients.json in the directory RW_REPORT_DIR names (default: test_reports/ at the repository's
root, which git ignores)."""
import functools
import json
import os

import pytest
import torch

from tests import generator_gradient_checks as C
from tests import grad_emulation as G
from tests.conftest import build_stylegan, oracle_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TRUNCATION = 0.7
# Where the report goes is the run's choice, not this file's: whoever collects reports from a GPU run names the directory in
# RW_REPORT_DIR (the older GPU tests hard-code the output directory of one particular job runner, which new code must not
# depend on); the default is a git-ignored directory of the repository's own.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get('RW_REPORT_DIR') or os.path.join(ROOT, 'test_reports')
REPORT = os.path.join(REPORT_DIR, 'generator_gradients.json')


def report(section, value):
    os.makedirs(REPORT_DIR, exist_ok=True)
    data = {}
    if os.path.isfile(REPORT):
        with open(REPORT) as f:
            data = json.load(f)
    data[section] = value
    with open(REPORT, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------- the two kernels
KERNEL_SHAPES = [
    (1, 32, 4, 4),          # smallest map
    (2, 48, 5, 7),          # hw % 4 != 0: the scalar forms
    (3, 512, 8, 8),         # many channels: several channel groups
    (1, 64, 64, 64),        # several workgroups per image, the second reduction stage
    (2, 16, 33, 31),        # odd map, few channels
]


@pytest.mark.parametrize('shape', KERNEL_SHAPES)
def test_to_rgb_adjoint_kernels_match_float64_einsums(shape):
    """rel <= 1e-6 for the input gradient (a sum of three products per element: conv_wgrad's bar between two float32
    evaluations), <= 1e-5 for the sums over the pixels (rowdot's bar); the sums twice, bit for bit."""
    from rewriting_amd import hip
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(11 + c + h)
    g = torch.randn(b, 3, h, w, generator=gen)
    x = torch.randn(b, c, h, w, generator=gen)
    wt = torch.randn(3, c, generator=gen)
    style = 1 + 0.3 * torch.randn(b, c, generator=gen)
    scale = c ** -0.5
    gd, xd = g.to(DEV), x.to(DEV)
    want_gx = scale * style.double()[:, :, None, None] * torch.einsum('ci,bchw->bihw', wt.double(), g.double())
    want_t = torch.einsum('bchw,bihw->bci', g.double(), x.double())
    got_gx = hip.to_rgb_input_grad(gd, wt.to(DEV), style.to(DEV), scale)
    got_t = hip.to_rgb_weight_sums(gd, xd)
    again = hip.to_rgb_weight_sums(gd, xd)
    assert tuple(got_gx.shape) == (b, c, h, w) and tuple(got_t.shape) == (b, 3, c)
    e_gx, e_t = G.rel(got_gx, want_gx), G.rel(got_t, want_t)
    print('%s: input gradient rel %.2e, sums rel %.2e' % (shape, e_gx, e_t))
    assert e_gx <= 1e-6, e_gx
    assert e_t <= 1e-5, e_t
    assert torch.equal(got_t, again)


def test_the_adjoint_wrappers_refuse_other_dtypes():
    from rewriting_amd import hip
    g, x = torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 16, 4, 4, device=DEV)
    for bad in (torch.float64, torch.float16):
        with pytest.raises(RuntimeError, match='fp32 only'):
            hip.to_rgb_weight_sums(g.to(bad), x)
        with pytest.raises(RuntimeError, match='fp32 only'):
            hip.to_rgb_input_grad(g, torch.zeros(3, 16, device=DEV, dtype=bad), torch.ones(1, 16, device=DEV), 1.0)


# ---------------------------------------------------------------------------------------------- the whole generator
@functools.lru_cache(maxsize=None)
def generator(size):
    """(model on the device, its state dict on the host, its parameter names): built once per size."""
    model = build_stylegan(size, TRUNCATION, device=DEV)
    return model, oracle_state_dict(model), tuple(n for n, _ in model.named_parameters())


@functools.lru_cache(maxsize=None)
def oracle(size, seed, dtype, frozen=False):
    """The recipe's oracle on the host, computed once and shared (never modified)."""
    _, sd, names = generator(size)
    z, target = G.recipe(size, seed)
    return G.oracle_gradients(sd, () if frozen else names, z, target, size, TRUNCATION, dtype)


@pytest.mark.parametrize('size', [8, 16])
def test_whole_generator_gradients_against_the_float64_oracle(size):
    """Seeds 0..4 of the recipe: d_hip, the worst per-tensor relative gradient error against float64, beside d_ref,
    the same for the float32 run of the restatement on the host (1.3e-6 .. 1.8e-6 on these inputs).  Every seed has
    d_hip < 5e-3 and at least 4 of the 5 have d_hip <= 8 d_ref(seed): 8 is the margin over the reference's own float32
    deviation (the grad-mode routes split operands into f16 pairs, 2^-21 per product against 2^-24, and sum in another
    order); the one miss allowed per size is for a leaky-ReLU input within rounding of zero that the device's rounding
    hits where the host's did not (seed 7 does that in float32 alone: 2e-4 .. 5e-4)."""
    model, _, names = generator(size)
    rows = []
    for seed in range(5):
        z, target = G.recipe(size, seed)
        want_loss, want_img, want = oracle(size, seed, torch.float64)
        _, _, ref = oracle(size, seed, torch.float32)
        loss, img, got = G.model_gradients(model, z, target)
        missing = [name for name in want if got[name] is None]
        assert not missing, 'no gradient reached %s' % missing
        d_hip, where = G.worst_relative_error(got, want)
        d_ref, _ = G.worst_relative_error(ref, want)
        rows.append(dict(seed=seed, d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref, worst_tensor=where,
                         loss_rel=abs(loss.item() - want_loss.item()) / abs(want_loss.item()),
                         image_linf=(img.double().cpu() - want_img).abs().max().item()))
        print('size %d seed %d: d_hip %.3e (%s)  d_ref %.3e  ratio %.2f  loss rel %.2e  image Linf %.2e'
              % (size, seed, d_hip, where, d_ref, d_hip / d_ref, rows[-1]['loss_rel'], rows[-1]['image_linf']))
    report('whole_generator_size%d' % size, rows)
    for r in rows:
        assert r['loss_rel'] <= 2e-6, r
        assert r['image_linf'] <= 5e-5, r
        assert r['d_hip'] < 5e-3, r
    assert sum(r['d_hip'] <= 8 * r['d_ref'] for r in rows) >= 4, rows


def test_latent_only_gradient():
    """Every parameter frozen, z requires a gradient (projecting a picture into the generator): z.grad at the bar above --
    8 times the float32 restatement's own deviation, here on the one tensor there is -- and no parameter has a .grad."""
    from rewriting_amd.utils import nethook
    size, seed = 16, 0
    model, _, names = generator(size)
    z, target = G.recipe(size, seed)
    _, _, want = oracle(size, seed, torch.float64, frozen=True)
    _, _, ref = oracle(size, seed, torch.float32, frozen=True)
    nethook.set_requires_grad(False, model)
    try:
        _, _, got = G.model_gradients(model, z, target)
    finally:
        nethook.set_requires_grad(True, model)
    d_hip, d_ref = G.rel(got['z'], want['z']), G.rel(ref['z'], want['z'])
    print('latent only: d_hip %.3e  d_ref %.3e  ratio %.2f' % (d_hip, d_ref, d_hip / d_ref))
    report('latent_only_size%d' % size, dict(seed=seed, d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref))
    assert all(got[name] is None for name in names)
    assert d_hip <= 8 * d_ref, (d_hip, d_ref)


def test_all_weights_insert_at_16():
    """The reference's overfit loop, 20 iterations, with the convolution-free perceptual network (no MIOpen behind it):
    the first loss within 1e-5 of the float64 oracle's, the last below the first; the losses in between are recorded
    beside the oracle's and not asserted (Adam's first steps are sign-like: a gradient entry within rounding of zero
    moves its weight the other way)."""
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    size, niter = 16, 20
    model = build_stylegan(size, TRUNCATION, device=DEV)
    zds = zdataset.z_dataset_for_model(model, size=10)
    gw = ganrewrite.SeqStyleGanRewriter(model, zds, 6, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    bounds = (4, 4, 12, 12)
    with pytest.raises(NotImplementedError, match='feature_net'):
        gw.all_weights_insert(x, z, bounds=bounds, niter=niter)
    names = [n for n, _ in gw.model.named_parameters()]
    want = G.overfit_oracle(oracle_state_dict(gw.model), names, x.cpu(), z.cpu(), bounds, size, TRUNCATION, niter=niter,
                            lr=0.01, feature_net=G.PooledMix())
    losses = []
    gw.all_weights_insert(x, z, bounds=bounds, niter=niter, lr=0.01, feature_net=G.PooledMix().to(DEV),
                          update_callback=lambda it, loss: losses.append(loss.item()))
    report('all_weights_insert_size%d' % size, dict(losses=losses, oracle=want))
    print('all_weights_insert: loss[0] %.6f (oracle %.6f), loss[19] %.6f (oracle %.6f)'
          % (losses[0], want[0], losses[-1], want[-1]))
    assert len(losses) == niter
    assert abs(losses[0] - want[0]) <= 1e-5 * abs(want[0]), (losses[0], want[0])
    assert losses[19] < losses[0], losses


# ---------------------------------------------------------------------------------- 32^2 and 64^2: pinned decisions
# From the 32^2 map up the forward and the backward take routes that the 8^2 and 16^2 models never reach: the general
# tile form of conv3x3_wino, the split f16-pair form of conv_transpose3x3s2_wino with its strips on the auxiliary stream,
# conv3x3_direct16 measuring its own bound, the fused blocks in front of a partly frozen model, and in the backward
# conv3x3(impl=0) / conv_wgrad / rowdot on maps of up to 65 x 65.  The measure, its bars and where they come from:
# tests/generator_gradient_checks.py.  Every test below records its launches (tests/route_spy.py), asserts the ones that
# make it worth running, and asserts that planting the decision hooks changed none (C.recorded_run).  Figures:
# DESIGN.md section 8.1.

@pytest.fixture
def launches(monkeypatch):
    from tests import route_spy
    log = []
    route_spy.install_spies(monkeypatch, log)
    return log


def held(section, tag, run, names, z, target, size):
    """C.check of one run; the figures into the report and the output BEFORE anything is asserted"""
    _, sd, _ = generator(size)
    figures, bad = C.check(run, sd, names, z, target, size, TRUNCATION)
    report(section, figures)
    print(C.describe(tag, figures))
    assert not bad, bad


@pytest.mark.parametrize('size,seed', [(32, 0), (32, 2), (64, 1), (64, 2)])
def test_pinned_every_parameter_and_the_latent(launches, size, seed):
    """Scenario A: everything trainable and z.  Every tensor receives a gradient and is within 8 d_ref of the float64
    oracle on the run's own branches (one-element tensors: 8 times the largest d_ref among them), no seed exempted.
    What ran, from the record: conv3x3_wino on the 32^2 map (and the 64^2 one at size 64); at size 64 the transposed
    convolution of the 32^2 map in the split form -- conv_transpose3x3s2_wino with a bound, measured by absmax, beside the
    strip launch (impl 8); in the backward conv_wgrad with the stride-2 gather and conv3x3(impl=0) with demod as its
    on-load factor on the (size + 1)^2 gradient map of the last transposed convolution: 65 x 65 at size 64, 33 x 33 at 32.
    Measured on one MI355X: the largest ratio on a multi-element tensor is 2.55 / 4.33 / 2.63 / 3.36 in the order of the
    cases (to_rgb2.rgb.bias on three of them); a noise strength reaches 9.77 times its OWN d_ref (layer7, size 64, seed 2)
    and half of the one-element bar at most."""
    model, _, names = generator(size)
    z, target = G.recipe(size, seed)
    run = C.recorded_run(model, z, target, launches)
    held('pinned_all_size%d_seed%d' % (size, seed), 'A size %d seed %d' % (size, seed), run, names + ('z',), z, target, size)
    wide = (2, 512, size + 1, size + 1)
    for side in sorted({32, size}):
        assert C.launched(run.launches, 'conv3x3_wino', (2, 512, side, side)), run.launches
    assert C.launched(run.launches, 'conv_wgrad', wide, flags=('upsample', 'gscale')), run.launches
    assert C.launched(run.launches, 'conv3x3', wide, impl=0, flags=('style',)), run.launches
    if size == 64:
        assert C.launched(run.launches, 'conv_transpose3x3s2_wino', (2, 512, 32, 32), flags=('x_amax',)), run.launches
        assert C.launched(run.launches, 'conv_transpose3x3s2', (2, 512, 32, 32), impl=8), run.launches
        assert not C.launched(run.launches, 'conv_transpose3x3s2_wino', (2, 512, 16, 16), flags=('x_amax',))


@pytest.mark.parametrize('size,seed', [(32, 0), (64, 1)])
def test_pinned_latent_only(launches, size, seed):
    """Scenario B: every parameter frozen, z.grad at the bar (one multi-element tensor), no parameter with a .grad.
    weight_changes is false: the stride-1 layers from the 32^2 map up are conv3x3_direct16, measuring their own bound.
    Measured on one MI355X: ratio 1.26 at size 32, 1.56 at size 64."""
    model, _, names = generator(size)
    z, target = G.recipe(size, seed)
    with C.only_trainable(model, ()):
        run = C.recorded_run(model, z, target, launches)
    held('pinned_latent_only_size%d' % size, 'B size %d seed %d' % (size, seed), run, ('z',), z, target, size)
    assert all(run.grads[name] is None for name in names)
    assert all(p.requires_grad for p in model.parameters())
    for side in sorted({32, size}):
        assert C.launched(run.launches, 'conv3x3_direct16', (2, 512, side, side)), run.launches
        assert C.launched(run.launches, 'absmax', (2, 512, side, side)), run.launches
        assert not C.launched(run.launches, 'conv3x3_wino', (2, 512, side, side))


def test_pinned_partly_frozen_model(launches):
    """Scenario C at size 64: only the parameters of layer10 and to_rgb5 trainable, z without a gradient.  Every
    trainable tensor at the bar, nothing else with a .grad.  The hand-over, from the record: the layers in front run as
    fused blocks -- conv3x3_direct16 with its activation and conv_transpose3x3s2_blur_fused, both on the 32^2 map -- and
    layer10 behind them module by module: style_mul on the 64^2 map, then conv3x3_wino on it, then in the backward
    conv_wgrad on the 64^2 map.  Measured on one MI355X: ratio at most 2.38 (to_rgb5.rgb.bias); the one noise strength
    1.70 times its own d_ref."""
    size, seed = 64, 1
    model, _, names = generator(size)
    trainable = tuple(C.partly_frozen_names(model))
    assert len(trainable) == 9
    z, target = G.recipe(size, seed)
    with C.only_trainable(model, trainable):
        run = C.recorded_run(model, z, target, launches, z_grad=False)
    held('pinned_partly_frozen_size%d' % size, 'C size %d seed %d' % (size, seed), run, trainable, z, target, size)
    assert run.grads['z'] is None and all(run.grads[n] is None for n in names if n not in trainable)
    assert all(p.requires_grad for p in model.parameters())
    log = run.launches
    direct = C.index_of(log, 'conv3x3_direct16', (2, 512, 32, 32), flags=('act', 'noise', 'bias'))
    fused = C.index_of(log, 'conv_transpose3x3s2_blur_fused', (2, 512, 32, 32), flags=('act', 'noise', 'bias'))
    mul = C.index_of(log, 'style_mul', (2, 512, 64, 64))
    wino = C.index_of(log, 'conv3x3_wino', (2, 512, 64, 64))
    wgrad = C.index_of(log, 'conv_wgrad', (2, 512, 64, 64))
    assert direct < fused < mul < wino < wgrad, log
    assert not C.launched(log, 'style_mul', (2, 512, 32, 32)), log          # nothing in front ran module by module


def test_all_weights_insert_teacher_forced_at_32(monkeypatch):
    """Scenario D: all_weights_insert at size 32, 6 iterations, crop (8, 8, 24, 24), lr 0.01, the convolution-free
    perceptual network.  The loss reported at every iteration is the float64 restatement's at the state the loop was in
    (the initial one, then the snapshot taken after the optimizer.step() before), 1e-5 relative, no decision pinned; and
    every iteration packs every trained convolution weight in the forms iteration 0 packed it, each once.  A packed weight
    that outlives a step fails at iteration 1, which the first loss and `loss[19] < loss[0]` of the size-16 test do not see."""
    model = build_stylegan(C.OVERFIT['size'], TRUNCATION, device=DEV)
    rows, bad, packs = C.teacher_forced_overfit(model, TRUNCATION, DEV, monkeypatch)
    report('all_weights_insert_teacher_forced_size%d' % C.OVERFIT['size'], dict(rows=rows, packs_per_iteration=packs))
    print('\n'.join('it %(it)d: loss %(loss).6f  oracle %(oracle).6f  rel %(rel).1e' % r for r in rows))
    assert not bad, bad
    assert len(rows) == C.OVERFIT['niter']
