"""rewriting_amd/perceptual.py on the host: the state dict, the block structure, the emulated forward and input gradient
against a float64 twin written here from torch.nn.functional (tests/perceptual_checks.py), what no_grad leaves out, the
RW_VGG16_WEIGHTS default of all_weights_insert, the four entries of the C ABI and the refusals of their wrappers."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import _lib, hip, perceptual
from tests import generator_gradient_checks as C
from tests import perceptual_checks as P
from tests.conftest import build_stylegan

ENTRIES = ('rw_bias_relu_pool_f32', 'rw_bias_relu_pool_grad_f32', 'rw_conv3x3_rgb_f32', 'rw_conv3x3_rgb_input_grad_f32')
# The reference of every accuracy check is the float32 run of the same twin: its own 2-norm relative error d_ref against the
# float64 twin, measured in the test.  The emulated kernels are that float32 arithmetic in another order (the F(2x2,3x3)
# transforms included): d <= MARGIN * d_ref, the bar of the device test (DESIGN section 8.1's margin).
MARGIN = 8


@pytest.fixture
def emulated(emulated_hip, monkeypatch):
    log = []
    P.install(monkeypatch, log)
    return log


@pytest.fixture(scope='module')
def sd():
    return P.random_state_dict(0)


def image(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_state_dict_round_trip_bare_and_torchvision_keys(sd, tmp_path):
    names = ['%d.%s' % (index, kind) for index in (0, 2, 5, 7, 10, 12, 14, 17, 19) for kind in ('weight', 'bias')]
    net = perceptual.from_state_dict(sd)
    assert sorted(net.state_dict()) == sorted(names) == sorted(n for n, _ in net.named_parameters())
    assert all(torch.equal(net.state_dict()[k], sd[k]) for k in names)
    assert not any(p.requires_grad for p in net.parameters())
    whole = perceptual.from_state_dict(P.torchvision_style(sd))
    assert all(torch.equal(whole.state_dict()[k], sd[k]) for k in names)
    path = tmp_path / 'vgg16.pth'
    torch.save(P.torchvision_style(sd), str(path))
    loaded = perceptual.vgg16_features(str(path))
    assert all(torch.equal(loaded.state_dict()[k], sd[k]) and loaded.state_dict()[k].device.type == 'cpu' for k in names)
    again = perceptual.from_state_dict(net.state_dict())
    assert all(torch.equal(again.state_dict()[k], sd[k]) for k in names)
    with pytest.raises(KeyError, match='lacks 19.bias'):
        perceptual.from_state_dict({k: v for k, v in sd.items() if k != '19.bias'})
    with pytest.raises(ValueError, match='0.weight'):
        perceptual.from_state_dict(dict(sd, **{'0.weight': torch.zeros(64, 3, 1, 1)}))
    with pytest.raises(KeyError, match='3.weight'):
        perceptual.from_state_dict(dict(sd, **{'3.weight': torch.zeros(1)}))


@pytest.mark.parametrize('shape', [(2, 3, 32, 32), (1, 3, 20, 28)])
def test_block_structure_and_output_shape(emulated, sd, shape):
    net = perceptual.from_state_dict(sd)
    blocks = net.blocks()
    assert [(b.in_ch, b.out_ch, b.pool) for b in blocks] == [
        (3, 64, False), (64, 64, True), (64, 128, False), (128, 128, True), (128, 256, False), (256, 256, False),
        (256, 256, True), (256, 512, False), (512, 512, False)]
    trace = []
    with torch.no_grad():
        out = net(image(shape, 1), trace=trace)
    b, _, h, w = shape
    assert tuple(out.shape) == (b, 512, h // 8, w // 8)
    sizes = [(h, w)] * 2 + [(h // 2, w // 2)] * 2 + [(h // 4, w // 4)] * 3 + [(h // 8, w // 8)] * 2
    assert [tuple(y.shape) for y in trace] == [(b, blk.out_ch) + s for blk, s in zip(blocks, sizes)]


@pytest.mark.parametrize('shape,seed', [((2, 3, 32, 32), 2), ((1, 3, 20, 28), 3)])
def test_emulated_forward_and_input_gradient_against_the_float64_twin(emulated, sd, shape, seed):
    net = perceptual.from_state_dict(sd)
    gt, pred = image(shape, seed), image(shape, seed + 10).requires_grad_(True)
    trace = []
    got = net(pred, trace=trace)
    assert got.requires_grad and not net(gt).requires_grad
    loss = 1e-2 * F.mse_loss(net(gt), got)
    loss.backward()
    outputs, outputs32 = [], []
    want = P.twin(sd, pred.detach(), torch.float64, outputs=outputs)
    ref = P.twin(sd, pred.detach(), torch.float32, outputs=outputs32)
    assert P.rel(ref, want) < 1e-5 and P.rel(got, want) <= MARGIN * P.rel(ref, want)
    for y, (_, _, _, pool), o, o32 in zip(trace, perceptual.LAYERS, outputs, outputs32):
        assert P.rel(F.max_pool2d(y, 2, 2) if pool else y, o) <= MARGIN * P.rel(o32, o)
    forced = P.decisions(trace)
    wanted = {}
    for dtype in (torch.float64, torch.float32):
        p = pred.detach().to(dtype).requires_grad_(True)
        wanted[dtype] = 1e-2 * F.mse_loss(P.twin(sd, gt, dtype), P.twin(sd, p, dtype, forced=forced))
        wanted[dtype].backward()
        wanted[dtype] = (wanted[dtype].item(), p.grad)
    want_loss, want_grad = wanted[torch.float64]
    d_ref = P.rel(wanted[torch.float32][1], want_grad)
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    assert d_ref < 1e-5 and P.rel(pred.grad, want_grad) <= MARGIN * d_ref, (P.rel(pred.grad, want_grad), d_ref)
    assert gt.grad is None


def test_the_forced_twin_is_the_twin_on_its_own_decisions(sd):
    x = image((1, 3, 20, 28), 5)
    own = []
    want = P.twin(sd, x, torch.float64, own=own)
    assert torch.equal(P.twin(sd, x, torch.float64, forced=own), want)
    assert P.differing_share(own, own) == (0.0, 0.0)


def test_under_no_grad_no_function_is_entered_and_no_pooled_y_is_kept(emulated, sd, monkeypatch):
    net = perceptual.from_state_dict(sd)
    entered = []
    monkeypatch.setattr(perceptual._BlockFunction, 'apply',
                        lambda *a, _apply=perceptual._BlockFunction.apply: entered.append(1) or _apply(*a))
    x = image((1, 3, 16, 16), 4)
    with torch.no_grad():
        net(x.clone().requires_grad_(True))
    net(x)                                              # grad mode, an input without a gradient: VF(gt)
    assert not entered
    calls = [(kw.get('pool', False), kw.get('keep', True)) for name, _, kw in emulated if name == 'bias_relu_pool']
    assert len(calls) == 16 and all(keep == (not pool) for pool, keep in calls) and sum(pool for pool, _ in calls) == 6
    assert not [name for name, _, _ in emulated if name.endswith('_grad')]
    del emulated[:]
    net(x.clone().requires_grad_(True))
    assert len(entered) == 9
    assert all(kw['keep'] for name, _, kw in emulated if name == 'bias_relu_pool')


def test_a_parameter_that_requires_a_gradient_and_foreign_inputs_are_refused(emulated, sd, monkeypatch):
    net = perceptual.from_state_dict(sd)
    x = image((1, 3, 8, 8), 6)
    getattr(net, '7').weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='7.weight requires a gradient'):
        net(x)
    getattr(net, '7').weight.requires_grad_(False)
    net(x)
    with pytest.raises(RuntimeError, match='fp32 only'):
        net(x.double())
    with pytest.raises(ValueError, match=r'\(B, 3, H, W\)'):
        net(x[:, :2])
    with pytest.raises(ValueError, match='at least 8 x 8'):
        net(x[:, :, :7])
    monkeypatch.setattr(hip, 'on_device', lambda t: bool(t.is_cuda))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(x)


def test_weights_named_by_the_environment_are_the_default_feature_net(emulated, sd, tmp_path, monkeypatch):
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    from tests import grad_emulation
    grad_emulation.install(monkeypatch)                 # ToRGB's adjoints (the generator's backward)
    model = build_stylegan(8, 0.7)
    gw = ganrewrite.SeqStyleGanRewriter(model, zdataset.z_dataset_for_model(model, size=4), 4, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    monkeypatch.delenv(perceptual.WEIGHTS_ENV, raising=False)
    with pytest.raises(NotImplementedError, match='feature_net.*RW_VGG16_WEIGHTS'):
        gw.all_weights_insert(x, z, niter=1)
    monkeypatch.setenv(perceptual.WEIGHTS_ENV, str(tmp_path / 'absent.pth'))
    with pytest.raises(NotImplementedError, match='feature_net'):
        gw.apply_overfit({'object': [0, None], 'paste': [1, None]}, niter=1)
    path = tmp_path / 'vgg16.pth'
    torch.save(P.torchvision_style(sd), str(path))
    monkeypatch.setenv(perceptual.WEIGHTS_ENV, str(path))
    before = {k: v.detach().clone() for k, v in gw.model.state_dict().items()}
    seen = []
    gw.all_weights_insert(x, z, niter=1, lr=0.01, feature_net=None, update_callback=lambda it, loss: seen.append(loss.item()))
    want = C.overfit_loss(before, x, z, (0, 0, 8, 8), 8, 0.7, P.Twin(sd))
    assert len(seen) == 1 and abs(seen[0] - want) <= 1e-5 * abs(want), (seen, want)
    names = [n for n, _ in gw.model.named_parameters()]
    assert not [n for n in names if torch.equal(gw.model.state_dict()[n], before[n])]
    built = gw._feature_net(None)
    assert isinstance(built, perceptual.VGG16Features) and gw._feature_net(None) is built
    own = torch.nn.Identity()
    assert gw._feature_net(own) is own


def test_the_four_entries_are_bound_and_exported():
    assert _lib.ABI_VERSION == 11
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert not [n for n in ENTRIES if n.endswith('_supported') or n.startswith('rw_packed_')]


def test_the_wrappers_refuse_before_any_call(monkeypatch):
    """wrong dtype, shape and device: nothing reaches the library (lib() would raise here)"""
    def no_call():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(hip, 'lib', no_call)
    x, b = torch.zeros(1, 4, 4, 4), torch.zeros(4)
    w, rgb = torch.zeros(64, 3, 3, 3), torch.zeros(1, 3, 4, 4)
    for call in (lambda: hip.bias_relu_pool(x, b), lambda: hip.bias_relu_pool_grad(x, x),
                 lambda: hip.conv3x3_rgb(rgb, w, torch.zeros(64)), lambda: hip.conv3x3_rgb_input_grad(torch.zeros(1, 64, 4, 4), w)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))      # past the device check, on the host
    for call in (lambda: hip.bias_relu_pool(x.double(), b), lambda: hip.bias_relu_pool(x, b.half()),
                 lambda: hip.bias_relu_pool_grad(x.double(), x), lambda: hip.conv3x3_rgb(rgb.half(), w, torch.zeros(64)),
                 lambda: hip.conv3x3_rgb_input_grad(torch.zeros(1, 64, 4, 4), w.double())):
        with pytest.raises(RuntimeError, match='fp32 only'):
            call()
    for call in (lambda: hip.bias_relu_pool(x, torch.zeros(5)), lambda: hip.bias_relu_pool(x[0], b),
                 lambda: hip.bias_relu_pool(x, b, pool=False, keep=False),
                 lambda: hip.bias_relu_pool(x, b, out=torch.zeros(1, 4, 4, 2)),
                 lambda: hip.bias_relu_pool_grad(torch.zeros(1, 4, 2, 2), x), lambda: hip.bias_relu_pool_grad(x, x, pooled=True),
                 lambda: hip.conv3x3_rgb(x, w, torch.zeros(64)), lambda: hip.conv3x3_rgb(rgb, w, torch.zeros(32)),
                 lambda: hip.conv3x3_rgb(rgb, torch.zeros(128, 3, 3, 3), torch.zeros(128)),
                 lambda: hip.conv3x3_rgb(rgb, torch.zeros(64, 3, 1, 1), torch.zeros(64)),
                 lambda: hip.conv3x3_rgb_input_grad(torch.zeros(1, 32, 4, 4), w),
                 lambda: hip.conv3x3_rgb_input_grad(torch.zeros(1, 64, 4, 4), torch.zeros(64, 4, 3, 3))):
        with pytest.raises(ValueError):
            call()
