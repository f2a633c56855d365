"""The perceptual network on the device (rw_percept.hip, rewriting_amd/perceptual.py): the streaming kernels bit for bit
against torch on the host, the first layer and its adjoint against float64 with the bound of a chain of rounded
operations, the whole network's features and the input gradient of the loss term against a float64 twin (bar: 8 times the
float32 twin's own error, DESIGN section 8.1's margin), and ``all_weights_insert`` with this network.  Figures go to
perceptual.json in the directory RW_REPORT_DIR names (default: test_reports/, which git ignores); DESIGN section 8.6 copies
them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import generator_gradient_checks as C
from tests import perceptual_checks as P
from tests.conftest import build_stylegan, oracle_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TRUNCATION = 0.7
MARGIN = 8                          # d_hip <= MARGIN * d_ref
D_REF_MAX = 1e-5                    # the condition on the reference alone
EPS = 2.0 ** -24

# (2,64,8,8): 16-byte form, several planes; (1,16,2,2): one window per plane; (2,3,5,7): odd sizes -- the floor, the scalar
# form; (1,32,6,10): w % 4 != 0; the last one is laid at a 4-byte offset: the unaligned pointer that takes the scalar form
POOL_SHAPES = [((2, 64, 8, 8), 0), ((1, 16, 2, 2), 0), ((2, 3, 5, 7), 0), ((1, 32, 6, 10), 0), ((1, 8, 4, 12), 1)]
NETWORK_SHAPES = [(2, 3, 32, 32), (1, 3, 20, 28)]


@functools.lru_cache(maxsize=None)
def weights():
    return P.random_state_dict(0)


@functools.lru_cache(maxsize=None)
def network():
    from rewriting_amd import perceptual
    return perceptual.from_state_dict(weights()).to(DEV)


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def on_device(t, offset=0):
    """t on the device, `offset` floats past an allocation's start (a contiguous view: the wrappers read it in place)"""
    flat = torch.empty(t.numel() + offset, device=DEV, dtype=t.dtype)
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * offset
    return view


def planted(shape, seed):
    """a map with windows of four equal values above the bias, windows that stay at or below zero after it, a window whose
    first and third positions tie, and noise elsewhere; bias of std 0.1"""
    x, bias = randn(shape, seed), 0.1 * randn(shape[1:2], seed + 1)
    h, w = shape[2] // 2 * 2, shape[3] // 2 * 2
    x[:, :, 0:2, 0:2] = 2.0
    x[:, :, h - 2:h, w - 2:w] = -2.0
    if w >= 4:
        x[:, :, 0:2, 2:4] = torch.tensor([[1.5, -1.0], [1.5, 0.25]])
    if h >= 4:
        x[:, :, 2:4, 0:2] = torch.tensor([[-3.0, 0.75], [0.5, 0.75]])
    return x, bias


# ------------------------------------------------------------------------------------------ bias + ReLU (+ pool)
@pytest.mark.parametrize('shape,offset', POOL_SHAPES)
def test_bias_relu_pool_is_exact(shape, offset):
    """one rounded add and maxima on both sides: torch.equal; y null, pooled null, y aliasing x"""
    from rewriting_amd import hip
    x, bias = planted(shape, 3 + shape[1])
    want_y = F.relu(x + bias[None, :, None, None])
    want_p = F.max_pool2d(want_y, 2, 2)
    bd = bias.to(DEV)
    xd = on_device(x, offset)
    y, pooled = hip.bias_relu_pool(xd, bd, pool=True)
    assert torch.equal(y.cpu(), want_y) and torch.equal(pooled.cpu(), want_p)
    assert tuple(pooled.shape) == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
    y, pooled = hip.bias_relu_pool(xd, bd, pool=True, keep=False)
    assert y is None and torch.equal(pooled.cpu(), want_p)
    y, pooled = hip.bias_relu_pool(xd, bd)
    assert pooled is None and torch.equal(y.cpu(), want_y)
    assert torch.equal(xd.cpu(), x)                                     # the input was only read so far
    for pool in (False, True):
        alias = on_device(x, offset)
        y, pooled = hip.bias_relu_pool(alias, bd, pool=pool, out=alias)
        assert y.data_ptr() == alias.data_ptr() and torch.equal(alias.cpu(), want_y)
        assert pooled is None if not pool else torch.equal(pooled.cpu(), want_p)


@pytest.mark.parametrize('shape,offset', POOL_SHAPES)
def test_bias_relu_pool_grad_routes_as_autograd_does(shape, offset):
    """the kernel only routes values: torch.equal against autograd through relu and max_pool2d on the host -- four equal
    positive values send to the top-left, an all-zero window sends nothing, an odd last row and column get zero"""
    from rewriting_amd import hip
    x, bias = planted(shape, 3 + shape[1])
    y = F.relu(x + bias[None, :, None, None])
    yd = on_device(y, offset)
    for pooled in (False, True):
        leaf = x.clone().requires_grad_(True)
        out = F.relu(leaf + bias[None, :, None, None])
        out = F.max_pool2d(out, 2, 2) if pooled else out
        g = randn(out.shape, 17 + pooled)
        out.backward(g)
        got = hip.bias_relu_pool_grad(on_device(g, offset), yd, pooled=pooled)
        assert torch.equal(got.cpu(), leaf.grad), (shape, pooled)
        if pooled:
            h, w = shape[2] // 2 * 2, shape[3] // 2 * 2
            if h > 2:                                   # (at 2 x 2 the one window is the all-zero one)
                assert torch.equal(got[:, :, 0:2, 0:2].cpu().flatten(2), g[:, :, 0, 0, None] * torch.tensor([1.0, 0, 0, 0]))
            assert not got[:, :, h - 2:h, w - 2:w].any() and not got[:, :, h:].any() and not got[:, :, :, w:].any()


# ------------------------------------------------------------------------------------------ the first layer
# batch 2 at 8 x 8; odd sizes (scalar stores); one more than the 16 x 64 pixel tile each way (2 x 2 tiles, three of them edges)
RGB_SHAPES = [(2, 3, 8, 8), (1, 3, 5, 7), (1, 3, 17, 65)]


@pytest.mark.parametrize('shape', RGB_SHAPES)
def test_conv3x3_rgb_and_its_adjoint_against_float64(shape):
    """|err| <= 1.01 * 28 * 2^-24 * (sum |w x| + |b|) forward (27 multiply-adds and the bias; ReLU does not widen it),
    <= 1.01 * 9 * out_ch * 2^-24 * sum |g w| for the adjoint: a chain of that many rounded operations in any order
    (tests/test_gpu_key_response.py's form).  Each twice, bit for bit."""
    from rewriting_amd import hip
    sd = weights()
    w, bias = sd['0.weight'], sd['0.bias']
    out_ch = w.shape[0]
    x = randn(shape, 21 + shape[3])
    want = F.relu(F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    bound = 1.01 * 28 * EPS * (F.conv2d(x.double().abs(), w.double().abs(), padding=1) + bias.double().abs()[None, :, None, None])
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    got = hip.conv3x3_rgb(xd, wd, bd)
    assert torch.equal(got, hip.conv3x3_rgb(xd, wd, bd))
    err = (got.cpu().double() - want).abs()
    print('conv3x3_rgb %s: worst err / bound %.3f' % (shape, (err / bound).max().item()))
    assert bool((err <= bound).all()), (err / bound).max().item()
    g = randn((shape[0], out_ch) + shape[2:], 22 + shape[3]) * (want > 0)
    want_g = F.conv_transpose2d(g.double(), w.double(), padding=1)
    bound_g = 1.01 * 9 * out_ch * EPS * F.conv_transpose2d(g.double().abs(), w.double().abs(), padding=1)
    gd = g.to(DEV)
    got_g = hip.conv3x3_rgb_input_grad(gd, wd)
    assert tuple(got_g.shape) == shape and torch.equal(got_g, hip.conv3x3_rgb_input_grad(gd, wd))
    err_g = (got_g.cpu().double() - want_g).abs()
    print('conv3x3_rgb_input_grad %s: worst err / bound %.3f' % (shape, (err_g / bound_g).max().item()))
    assert bool((err_g <= bound_g).all()), (err_g / bound_g).max().item()
    P.report('perceptual.json', 'rgb_layer_%dx%dx%d' % (shape[0], shape[2], shape[3]),
             dict(forward_err_over_bound=(err / bound).max().item(), adjoint_err_over_bound=(err_g / bound_g).max().item()))


def test_wrappers_refuse_on_the_device():
    from rewriting_amd import hip
    x, b = torch.zeros(1, 4, 4, 4, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match='fp32 only'):
        hip.bias_relu_pool(x.double(), b)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.bias_relu_pool_grad(x.cpu(), x)
    with pytest.raises(ValueError):
        hip.bias_relu_pool_grad(x, x, pooled=True)
    with pytest.raises(ValueError, match='RW_ERR_UNSUPPORTED'):
        hip.conv3x3_rgb(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(128, 3, 3, 3, device=DEV), torch.zeros(128, device=DEV))
    with pytest.raises(RuntimeError, match='fp32 only'):
        network()(torch.zeros(1, 3, 8, 8, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        network()(torch.zeros(1, 3, 8, 8))


# ------------------------------------------------------------------------------------------ the whole network
@pytest.fixture
def launches(monkeypatch):
    from tests import route_spy
    log = []
    route_spy.install_spies(monkeypatch, log)
    return log


def routes(log):
    names = [call.split()[0] for call in log]
    return names.count('conv3x3_wino'), names.count('conv3x3'), names.count('conv3x3_rgb'), names.count('conv3x3_rgb_input_grad')


@functools.lru_cache(maxsize=None)
def twin_features(shape):
    """(x, block outputs in float64, in float32) of the twin on the host: computed once, shared, never changed"""
    x = randn(shape, 31 + shape[3])
    out64, out32 = [], []
    P.twin(weights(), x, torch.float64, outputs=out64)
    P.twin(weights(), x, torch.float32, outputs=out32)
    return x, out64, out32


@pytest.mark.parametrize('shape', NETWORK_SHAPES)
def test_features_against_the_float64_twin(shape, launches):
    """32^2 reaches the F(2x2) forms for w % 32, w == 16 and the whole 8 x 8 and 4 x 4 maps; 20 x 28 gives maps of 20 x 28,
    10 x 14, 5 x 7 and 2 x 3: the direct route and the floor of the pooling.  Per block output and for the final features:
    d_hip <= 8 d_ref, d_ref < 1e-5 (the float32 twin against the float64 one)."""
    from rewriting_amd import perceptual
    x, out64, out32 = twin_features(shape)
    net = network()
    trace = []
    with torch.no_grad():
        got = net(x.to(DEV), trace=trace)
        again = net(x.to(DEV))
    assert torch.equal(got, again)
    wino, direct, rgb, _ = routes(launches)
    assert rgb == 2 and (wino, direct) == ((16, 0) if shape[2] == 32 else (0, 16)), launches
    outputs = [F.max_pool2d(y.cpu(), 2, 2) if pool else y.cpu() for y, (_, _, _, pool) in zip(trace, perceptual.LAYERS)]
    assert torch.equal(outputs[-1], got.cpu())
    rows, bad = [], []
    for n, (o, o64, o32) in enumerate(zip(outputs, out64, out32)):
        d_hip, d_ref = P.rel(o, o64), P.rel(o32, o64)
        rows.append(dict(block=perceptual.LAYERS[n][0], d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref))
        print('features %s block %2d: d_hip %.3e d_ref %.3e ratio %.2f' % (shape, perceptual.LAYERS[n][0], d_hip, d_ref,
                                                                         d_hip / d_ref))
        if not (d_ref < D_REF_MAX and d_hip <= MARGIN * d_ref):
            bad.append(rows[-1])
    P.report('perceptual.json', 'features_%dx%dx%d' % (shape[0], shape[2], shape[3]), rows)
    assert not bad, bad


@pytest.mark.parametrize('shape', NETWORK_SHAPES)
def test_input_gradient_of_the_loss_term(shape, launches):
    """d (1e-2 mse(VF(gt), VF(pred))) / d pred.  The device's ReLU and pool decisions are read from trace= and both host
    twins are forced onto them (a decision within rounding of a tie flips a gradient by far more than rounding);
    d_hip <= 8 d_ref on pred.grad, d_ref < 1e-5.  The share of decisions that differ from the float64 twin's own is
    reported, not asserted.  gt receives no gradient."""
    sd = weights()
    net = network()
    gt, pred = randn(shape, 41 + shape[3]), randn(shape, 42 + shape[3])
    gtd, predd = gt.to(DEV), pred.clone().to(DEV).requires_grad_(True)
    trace = []
    loss = 1e-2 * F.mse_loss(net(gtd), net(predd, trace=trace))
    loss.backward()
    wino, direct, rgb, rgb_grad = routes(launches)
    assert (rgb, rgb_grad) == (2, 1) and (wino, direct) == ((24, 0) if shape[2] == 32 else (0, 24)), launches
    assert gtd.grad is None and predd.grad is not None
    forced, own = P.decisions(trace), []
    P.twin(sd, pred, torch.float64, own=own)
    grads, losses = {}, {}
    for dtype in (torch.float64, torch.float32):
        leaf = pred.clone().to(dtype).requires_grad_(True)
        value = 1e-2 * F.mse_loss(P.twin(sd, gt, dtype), P.twin(sd, leaf, dtype, forced=forced))
        value.backward()
        grads[dtype], losses[dtype] = leaf.grad, value.item()
    d_hip, d_ref = P.rel(predd.grad.cpu(), grads[torch.float64]), P.rel(grads[torch.float32], grads[torch.float64])
    relu_share, pool_share = P.differing_share(forced, own)
    print('input gradient %s: d_hip %.3e d_ref %.3e ratio %.2f; decisions differing from float64: relu %.2e pool %.2e'
          % (shape, d_hip, d_ref, d_hip / d_ref, relu_share, pool_share))
    P.report('perceptual.json', 'input_gradient_%dx%dx%d' % (shape[0], shape[2], shape[3]),
             dict(d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref, loss=loss.item(), loss_float64=losses[torch.float64],
                  relu_decisions_differing=relu_share, pool_decisions_differing=pool_share))
    assert abs(loss.item() - losses[torch.float64]) <= 1e-5 * abs(losses[torch.float64])
    assert d_ref < D_REF_MAX and d_hip <= MARGIN * d_ref, (d_hip, d_ref)


# ------------------------------------------------------------------------------------------ the overfit loop
@pytest.mark.parametrize('default', [False, True], ids=['feature_net', 'RW_VGG16_WEIGHTS'])
def test_all_weights_insert_with_the_perceptual_network(default, tmp_path, monkeypatch):
    """size 32, crop (8, 8, 24, 24), one iteration: the loss reported at iteration 0 within 1e-5 of the float64 restatement's
    with the float64 twin as feature_net (scenario D), every parameter moved; once with the network handed
    in and once built from the file RW_VGG16_WEIGHTS names."""
    from rewriting_amd import perceptual
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    size, bounds = 32, (8, 8, 24, 24)
    model = build_stylegan(size, TRUNCATION, device=DEV)
    gw = ganrewrite.SeqStyleGanRewriter(model, zdataset.z_dataset_for_model(model, size=4), 6, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    before = oracle_state_dict(gw.model)
    want = C.overfit_loss(before, x.cpu(), z.cpu(), bounds, size, TRUNCATION, P.Twin(weights()))
    if default:
        path = tmp_path / 'vgg16.pth'
        torch.save(P.torchvision_style(weights()), str(path))
        monkeypatch.setenv(perceptual.WEIGHTS_ENV, str(path))
        net = None
    else:
        monkeypatch.delenv(perceptual.WEIGHTS_ENV, raising=False)
        with pytest.raises(NotImplementedError, match='feature_net.*RW_VGG16_WEIGHTS'):
            gw.all_weights_insert(x, z, bounds=bounds, niter=1)
        net = network()
    losses = []
    gw.all_weights_insert(x, z, bounds=bounds, niter=1, lr=0.01, feature_net=net,
                          update_callback=lambda it, loss: losses.append(loss.item()))
    print('all_weights_insert (%s): loss %.8f, float64 %.8f' % ('default' if default else 'feature_net', losses[0], want))
    P.report('perceptual.json', 'all_weights_insert_%s' % ('default' if default else 'feature_net'),
             dict(loss=losses[0], loss_float64=want, rel=abs(losses[0] - want) / abs(want)))
    assert len(losses) == 1 and abs(losses[0] - want) <= 1e-5 * abs(want), (losses, want)
    after = gw.model.state_dict()
    still = [name for name, _ in gw.model.named_parameters() if torch.equal(after[name].cpu(), before[name])]
    assert not still, 'parameters that did not move: %s' % still
    if default:
        built = gw._feature_net(None)
        assert isinstance(built, perceptual.VGG16Features) and next(built.parameters()).device == x.device
        # the request path with no feature_net at all: the same network, handed on.  The selection is a 16 x 20 box (the
        # recorded UI masks cover 4 x 8 pixels at this size, which three pools reduce to nothing)
        box = torch.zeros(size, size)
        box[6:22, 4:24] = 1
        monkeypatch.setattr(gw, '_mask_on', lambda mask, shape: box)
        handed, inner = {}, gw.all_weights_insert
        monkeypatch.setattr(gw, 'all_weights_insert', lambda x, z, **kw: handed.update(kw) or inner(x, z, **kw))
        del losses[:]
        gw.apply_overfit({'object': [2, None], 'paste': [3, None]}, niter=1, lr=0.01,
                         update_callback=lambda it, loss: losses.append(loss.item()))
        t, l, b, r = handed['bounds']
        assert handed['feature_net'] is built and (b - t, r - l) == (16, 20)
        assert len(losses) == 1 and 0 < losses[0] < float('inf')
