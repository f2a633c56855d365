"""Gradients from the image, on the emulated path: the adjoints of ToRGB, EqualLinear, PixelNorm and AdjustLatent
(utils/stylegan2/grad.py) make the whole generator differentiable, ``all_weights_insert`` runs the reference's overfit
loop over them, and under ``torch.no_grad()`` nothing of it is entered."""
import pytest
import torch

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
