"""Gradients from the image, on the emulated path: the adjoints of ToRGB, EqualLinear, PixelNorm and AdjustLatent
(utils/stylegan2/grad.py) make the whole generator differentiable, ``all_weights_insert`` runs the reference's overfit
loop over them, and under ``torch.no_grad()`` nothing of it is entered."""
import functools

import pytest
import torch

from tests import generator_gradient_checks as C
from tests import grad_emulation as G
from tests.conftest import build_stylegan, oracle_state_dict

SIZE, TRUNCATION = 8, 0.7
# The float32 restatement of the reference differs from its float64 self by 1.3e-6 .. 1.8e-6 (worst tensor, 2-norm
# relative) on seeds 0..4 of this recipe at sizes 8 and 16; the emulated kernels are the same float32 arithmetic in
# another order.  The bar is 8 times the SMALLEST of those deviations -- the margin the device test allows over the
# reference's own float32 error (tests/test_gpu_generator_gradients.py), taken at its tightest.
D_REF_MIN = 1.3e-6
BAR = 8 * D_REF_MIN


@pytest.fixture
def emulated(emulated_hip, monkeypatch):
    G.install(monkeypatch)


@pytest.mark.parametrize('seed', [0, 3])
def test_every_parameter_and_the_latent_get_the_oracles_gradient(emulated, seed):
    """loss(image) -> every parameter and z, against float64 autograd over oracle/restatement.py's generator_forward.
    Before the adjoints existed z.grad was None: the graph ended at the first raw-pointer kernel."""
    model = build_stylegan(SIZE, TRUNCATION)
    names = [n for n, _ in model.named_parameters()]
    z, target = G.recipe(SIZE, seed)
    want_loss, want_img, want = G.oracle_gradients(oracle_state_dict(model), names, z, target, SIZE, TRUNCATION,
                                                   torch.float64)
    loss, img, got = G.model_gradients(model, z, target)
    missing = [name for name in want if got[name] is None]
    assert not missing, 'no gradient reached %s' % missing
    assert abs(loss.item() - want_loss.item()) <= 2e-6 * abs(want_loss.item())
    assert (img.double() - want_img).abs().max().item() < 5e-5
    errors = {name: G.rel(got[name], want[name]) for name in want}
    worst = max(errors, key=errors.get)
    print('seed %d: worst relative gradient error %.3e on %s (bar %.2e)' % (seed, errors[worst], worst, BAR))
    assert errors[worst] <= BAR, (worst, errors[worst])


def test_latent_only(emulated):
    """Every parameter frozen: the gradient still reaches z (projecting a picture into the latent space) and no
    parameter gets one."""
    from rewriting_amd.utils import nethook
    model = build_stylegan(SIZE, TRUNCATION)
    nethook.set_requires_grad(False, model)
    names = [n for n, _ in model.named_parameters()]
    z, target = G.recipe(SIZE, 0)
    _, _, want = G.oracle_gradients(oracle_state_dict(model), [], z, target, SIZE, TRUNCATION, torch.float64)
    _, _, got = G.model_gradients(model, z, target)
    assert G.rel(got['z'], want['z']) <= BAR
    assert all(got[name] is None for name in names)


# ---- the twin of the device's tests at 32^2 (tests/test_gpu_generator_gradients.py, scenarios A, B and D): the same checks
# module on the emulated path, so that the checks themselves run wherever the suite does ------------------------------------
WIDE = 32


@functools.lru_cache(maxsize=None)
def wide_model():
    """(the 32^2 model, its state dict, its parameter names): built once, its parameters never stepped"""
    model = build_stylegan(WIDE, TRUNCATION)
    return model, oracle_state_dict(model), tuple(n for n, _ in model.named_parameters())


@pytest.fixture
def launches(emulated, monkeypatch):
    from tests import route_spy
    log = []
    route_spy.install_spies(monkeypatch, log)
    return log


def test_pinned_decisions_at_32_every_tensor_at_the_bar(launches):
    """Scenario A at size 32, seed 2 -- the seed at which the per-tensor ratio against float64's OWN branches reaches 290
    on a noise strength and 8.01 on a multi-element tensor for honest float32 arithmetic.  With both oracles on the run's
    branches every tensor is within 8 d_ref (measured: 1.18 on the worst multi-element tensor, 1.51 on a noise strength
    against its own d_ref; one decision of 2.78 million differs from float64's own).  The record holds
    conv3x3_wino on the 32^2 map, and in the backward conv_wgrad and conv3x3(impl=0) on the 33 x 33 gradient map of the
    transposed convolution (65 x 65 belongs to size 64): launches the 8^2 and 16^2 models never make."""
    model, sd, names = wide_model()
    z, target = G.recipe(WIDE, 2)
    run = C.recorded_run(model, z, target, launches)
    figures, bad = C.check(run, sd, names + ('z',), z, target, WIDE, TRUNCATION)
    print(C.describe('A size %d seed 2' % WIDE, figures))
    assert not bad, bad
    assert C.launched(run.launches, 'conv3x3_wino', (2, 512, 32, 32))
    assert C.launched(run.launches, 'conv_wgrad', (2, 512, 33, 33), flags=('upsample', 'gscale'))
    assert C.launched(run.launches, 'conv3x3', (2, 512, 33, 33), impl=0, flags=('style',))


def test_pinned_decisions_at_32_latent_only(launches):
    """Scenario B at size 32: every parameter frozen, z.grad at the bar, no parameter with a .grad; weight_changes is
    false, so the stride-1 layer of the 32^2 map is the direct sum that measures its own bound."""
    model, sd, names = wide_model()
    z, target = G.recipe(WIDE, 0)
    with C.only_trainable(model, ()):
        run = C.recorded_run(model, z, target, launches)
    figures, bad = C.check(run, sd, ('z',), z, target, WIDE, TRUNCATION)
    print(C.describe('B size %d seed 0' % WIDE, figures))
    assert not bad, bad
    assert all(run.grads[name] is None for name in names)
    assert all(p.requires_grad for p in model.parameters())
    assert C.launched(run.launches, 'conv3x3_direct16', (2, 512, 32, 32))
    assert C.launched(run.launches, 'absmax', (2, 512, 32, 32))
    assert not C.launched(run.launches, 'conv3x3_wino', (2, 512, 32, 32))


@pytest.mark.parametrize('size', [8, 16])
def test_the_small_sizes_make_none_of_those_launches(launches, size):
    """What the tests at 32^2 and 64^2 assert from the record is out of reach of the 8^2 and 16^2 models: no launch of
    theirs, forward or backward, all parameters trainable or none, sees a map of 32 rows or more, and none is a direct sum,
    a fused transposed convolution or a transposed convolution with a bound."""
    model = build_stylegan(size, TRUNCATION)
    z, target = G.recipe(size, 0)
    seen = list(C.recorded_run(model, z, target, launches).launches)
    with C.only_trainable(model, ()):
        seen += C.recorded_run(model, z, target, launches).launches
    assert any(call.startswith('conv_wgrad ') for call in seen) and any(call.startswith('conv3x3_wino ') for call in seen)
    for call in seen:
        name, shape, _, _, on = call.split(' ')
        if not name.startswith('pack_'):
            assert int(shape.split('x')[2]) < 32, call
        assert name not in ('conv3x3_direct16', 'conv_transpose3x3s2_blur_fused', 'absmax'), call
        assert 'x_amax' not in on.split(','), call


def test_the_overfit_loop_teacher_forced_at_32(emulated, monkeypatch):
    """Scenario D: every loss all_weights_insert reports equals the float64 restatement's at the state the loop was in
    (1e-5 relative), and every iteration packs every trained convolution weight once in each form -- a pack that is not
    renewed after optimizer.step() fails both at iteration 1."""
    rows, bad, packs = C.teacher_forced_overfit(build_stylegan(WIDE, TRUNCATION), TRUNCATION, 'cpu', monkeypatch)
    print('\n'.join('it %(it)d: loss %(loss).6f  oracle %(oracle).6f  rel %(rel).1e' % r for r in rows), packs)
    assert not bad, bad
    assert len(rows) == C.OVERFIT['niter']


def test_the_decision_hooks_refuse_what_they_cannot_pin(emulated):
    """The oracle's side of the pinning: a decision of another shape, one too few and one too many raise; recorded
    decisions given back reproduce the unpinned run bit for bit."""
    from oracle import restatement as R
    model = build_stylegan(SIZE, TRUNCATION)
    sd = oracle_state_dict(model)
    z, _ = G.recipe(SIZE, 0)
    own = R.RecordDecisions()
    plain = R.generator_forward(sd, z, SIZE, truncation=TRUNCATION)
    assert torch.equal(R.generator_forward(sd, z, SIZE, truncation=TRUNCATION, decisions=own), plain)
    assert [tuple(d.shape) for d in own] == [(2, 512)] * 8 + [(2, 512, 4, 4), (2, 512, 8, 8), (2, 512, 8, 8)]
    assert torch.equal(R.generator_forward(sd, z, SIZE, truncation=TRUNCATION, decisions=list(own)), plain)
    flipped = [~d for d in own]
    assert not torch.equal(R.generator_forward(sd, z, SIZE, truncation=TRUNCATION, decisions=flipped), plain)
    with pytest.raises(ValueError, match='consumed'):
        R.generator_forward(sd, z, SIZE, truncation=TRUNCATION, decisions=list(own) + [own[-1]])
    with pytest.raises(ValueError, match='no pinned decision'):
        R.generator_forward(sd, z, SIZE, truncation=TRUNCATION, decisions=list(own)[:-1])
    with pytest.raises(ValueError, match='activation'):
        R.generator_forward(sd, z, SIZE, truncation=TRUNCATION, decisions=list(own)[:-1] + [own[-1][:, :, :4]])
    with C.decisions_of(model) as seen, torch.enable_grad():
        model(z.clone().requires_grad_(True))
    assert [name for name, _ in seen] == ['style.%d' % i for i in range(1, 9)] + ['layer2.conv', 'layer3.sconv', 'layer4.sconv']
    assert not any(m._forward_hooks for m in model.modules())


def test_all_weights_insert_runs_the_reference_loop(emulated):
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    model = build_stylegan(SIZE, TRUNCATION)
    zds = zdataset.z_dataset_for_model(model, size=4)
    gw = ganrewrite.SeqStyleGanRewriter(model, zds, 4, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    bounds = (2, 2, 6, 6)
    net = G.PooledMix()
    with pytest.raises(NotImplementedError, match='feature_net'):
        gw.all_weights_insert(x, z, bounds=bounds, niter=3)
    with pytest.raises(NotImplementedError, match='feature_net'):
        gw.apply_overfit({'object': [0, None], 'paste': [1, None]}, niter=3)
    names = [n for n, _ in gw.model.named_parameters()]
    before = oracle_state_dict(gw.model)
    want = G.overfit_oracle(before, names, x, z, bounds, SIZE, TRUNCATION, niter=1, lr=0.01, feature_net=net)
    seen = []
    gw.all_weights_insert(x, z, bounds=bounds, niter=3, lr=0.01, feature_net=net,
                          update_callback=lambda it, loss: seen.append((it, loss.item())))
    assert [it for it, _ in seen] == [0, 1, 2]
    assert abs(seen[0][1] - want[0]) <= 1e-5 * abs(want[0]), (seen[0][1], want[0])
    after = gw.model.state_dict()
    still = [name for name in names if torch.equal(after[name], before[name])]
    assert not still, 'parameters that did not move: %s' % still
    assert all(p.requires_grad for p in gw.model.parameters())          # set_requires_grad as the reference leaves it


def test_nothing_of_it_is_entered_under_no_grad(emulated, monkeypatch):
    """Under no_grad the modules call the kernel wrappers directly, in the order they did before the adjoints existed:
    the recording with the new Functions switched off is the recording with them in place, and none of them is
    entered -- while under grad mode they are (the spy sees what it should)."""
    from rewriting_amd.utils.stylegan2 import grad
    from tests import route_spy
    model = build_stylegan(SIZE, TRUNCATION)            # parameters require a gradient, as a fresh model's do
    z, _ = G.recipe(SIZE, 0)
    entered = []
    for name in ('ToRGB', 'EqualLinear', 'PixelNorm', 'AdjustLatent'):
        cls = getattr(grad, name)

        def spied(*args, _apply=cls.apply, _name=name):
            entered.append(_name)
            return _apply(*args)
        monkeypatch.setattr(cls, 'apply', spied)
    log = []
    route_spy.install_spies(monkeypatch, log)

    def repack():                                   # every recording packs its own weights
        for m in model.modules():
            if hasattr(m, '_derived'):
                m._derived.store.clear()
    with torch.no_grad():
        img = model(z)
    assert not entered
    with_functions = list(log)
    del log[:]
    repack()
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(grad, 'records', lambda *tensors: False)
        same = model(z)
    assert log == with_functions and any(call.startswith('to_rgb') for call in log)
    assert torch.equal(img, same)
    with torch.enable_grad():
        model(z)
    assert {'ToRGB', 'EqualLinear'} <= set(entered)          # parameters alone start the graph ...
    del entered[:]
    with torch.enable_grad():
        model(z.clone().requires_grad_(True))
    assert {'ToRGB', 'EqualLinear', 'PixelNorm', 'AdjustLatent'} <= set(entered)       # ... and so does the latent


def test_partly_frozen_styled_convolutions_still_get_their_gradients(emulated):
    """z, the mapping network, the constant, every dconv weight and ToRGB frozen; the modulations, noise strengths and
    activation biases of the styled convolutions trainable (style fine-tuning): a block with ANY trainable parameter
    runs module by module, so each of them gets the oracle's gradient -- none is left without one behind a fused
    raw-pointer kernel."""
    from rewriting_amd.utils import nethook
    model = build_stylegan(SIZE, TRUNCATION)
    nethook.set_requires_grad(False, model)
    names = [n for n, p in model.named_parameters()
             if 'to_rgb' not in n and ('.mconv.modulation.' in n or n.endswith('.noise.weight') or n.endswith('.activate.bias'))]
    assert len(names) == 4 * 3                      # three styled convolutions at size 8: modulation w, b; noise; bias
    params = dict(model.named_parameters())
    nethook.set_requires_grad(True, *[params[n] for n in names])
    z, target = G.recipe(SIZE, 0)
    _, _, want = G.oracle_gradients(oracle_state_dict(model), names, z, target, SIZE, TRUNCATION, torch.float64)
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        G.smooth_loss(model(z), target).backward()
    missing = [n for n in names if params[n].grad is None]
    assert not missing, 'no gradient reached %s' % missing
    errors = {n: G.rel(params[n].grad, want[n]) for n in names}
    worst = max(errors, key=errors.get)
    assert errors[worst] <= BAR, (worst, errors[worst])
    assert all(p.grad is None for n, p in params.items() if n not in names)


def test_apply_overfit_pastes_the_object_and_trains_toward_it(emulated, monkeypatch):
    """The request path (rewrite/ganrewrite.py:171-181): the object's pixels under its mask, pasted at the paste mask's
    centre, become the goal image; all_weights_insert gets it with the paste box as (top, left, bottom, right) -- a
    2 x 4 box here, so a swapped order would show -- and its first loss is the oracle's for exactly that goal."""
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    from tests.conftest import load_mask_request
    model = build_stylegan(SIZE, TRUNCATION)
    zds = zdataset.z_dataset_for_model(model, size=4)
    gw = ganrewrite.SeqStyleGanRewriter(model, zds, 4, cachedir=None)
    req = load_mask_request('recorded_horse_hat.json', 4)
    net = G.PooledMix()
    handed = {}
    inner = gw.all_weights_insert

    def spied(x, z, **kwargs):
        handed.update(kwargs, x=x.clone(), z=z.clone())
        return inner(x, z, **kwargs)
    monkeypatch.setattr(gw, 'all_weights_insert', spied)
    with torch.no_grad():
        host = gw.model(gw.get_z(req['paste'][0]))
        source = gw.model(gw.get_z(req['object'][0]))
    names = [n for n, _ in gw.model.named_parameters()]
    before = oracle_state_dict(gw.model)
    seen = []
    gw.apply_overfit(req, niter=1, lr=0.01, feature_net=net, update_callback=lambda it, loss: seen.append(loss.item()))
    t, l, b, r = handed['bounds']
    assert (b - t, r - l) == (2, 4) and handed['feature_net'] is net and handed['niter'] == 1
    assert torch.equal(handed['z'], gw.get_z(req['paste'][0]))
    outside = torch.ones_like(host, dtype=torch.bool)
    outside[:, :, t:b, l:r] = False
    assert torch.equal(handed['x'][outside], host[outside])                  # the goal is the host image ...
    assert not torch.equal(handed['x'][:, :, t:b, l:r], host[:, :, t:b, l:r])      # ... with the object pasted in
    ot, ol, ob, orr = ganrewrite.positive_bounding_box(gw._mask_on(req['object'][1], gw.x_shape))
    area = gw._mask_on(req['object'][1], gw.x_shape)[ot:ob, ol:orr]
    blend = (1 - area) * host[:, :, t:b, l:r] + area * source[:, :, ot:ob, ol:orr]
    assert torch.allclose(handed['x'][:, :, t:b, l:r], blend, atol=1e-6)
    want = G.overfit_oracle(before, names, handed['x'], handed['z'], handed['bounds'], SIZE, TRUNCATION, niter=1, lr=0.01,
                            feature_net=net)
    assert len(seen) == 1 and abs(seen[0] - want[0]) <= 1e-5 * abs(want[0]), (seen, want)
