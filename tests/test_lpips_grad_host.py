"""LPIPS as a loss on the host (rewriting_amd/lpips.py: adjoint_table, LPIPS.target, LPIPS.loss, OverfitTerm; the perceptual=
argument of all_weights_insert): the walk of the one autograd node on the emulated kernels against the twin's autograd
(tests/lpips_grad_checks.py), the value against ``forward``'s, the ranges of the adjoint tables, every refusal, and the two
entries of the C ABI."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import _lib, hip, lpips
from tests import lpips_checks as L
from tests import lpips_grad_checks as LG

ENTRIES = ('rw_lpips_tap_grad_f32', 'rw_lpips_combine_grad_f32')
ADJOINT_CONVS = ('conv3x3', 'conv3x3_wino', 'conv3x3_rgb_input_grad')


@pytest.fixture
def emulated(emulated_hip, monkeypatch):
    log = []
    LG.install(monkeypatch, log)
    for name in ('conv3x3', 'conv3x3_wino'):                    # the emulation's own: logged too

        def call(*args, _name=name, _fn=getattr(hip, name), **kwargs):
            log.append((_name, args, kwargs))
            return _fn(*args, **kwargs)
        monkeypatch.setattr(hip, name, call)
    return log


@pytest.fixture(scope='module')
def net():
    return lpips.from_state_dicts(*L.weights())


def names(log):
    return [name for name, _, _ in log]


# (w: the mask, none; spatial; im1 of batch 1)
FORMS = [('masked', True, False), ('unmasked', True, False), ('masked', False, False), ('unmasked', False, False),
         ('masked', True, True)]


@pytest.mark.parametrize('shape', L.SHAPES)
def test_the_walk_against_the_twins_autograd(emulated, net, shape):
    """d (sum_b u_b loss_b) / d im0 with a random upstream u: within 1e-5 (2-norm, relative) of the float32 twin's autograd on
    the decisions the emulated forward took, and as close to the float64 twin's as that one (8 times its error); im1, the
    target and w receive nothing; one combine adjoint (spatial), five tap adjoints, thirteen adjoint convolutions."""
    im0, im1 = L.pair(shape, 'box')
    mask = L.mask(shape)
    up = torch.rand(shape[0], generator=torch.Generator().manual_seed(5)) + 0.5
    for which, spatial, one in FORMS:
        if one and shape[0] == 1:
            continue
        w = mask if which == 'masked' else None
        other = im1[:1] if one else im1
        leaf = im0.clone().requires_grad_(True)
        del emulated[:]
        trace = []
        value = net.loss(leaf, other, w=w, spatial=spatial, trace=trace)
        assert tuple(value.shape) == (shape[0],) and len(trace) == 13
        forward_calls = len(emulated)
        (value * up).sum().backward()
        back = names(emulated[forward_calls:])
        assert back.count('lpips_combine_grad') == (1 if spatial else 5 + (w is not None)), back
        assert back.count('lpips_tap_grad') == 5 and back.count('bias_relu_pool_grad') == 12
        assert sum(back.count(n) for n in ADJOINT_CONVS) == 13 and back.count('conv3x3_rgb_input_grad') == 1
        assert not set(back) & {'lpips_tap', 'lpips_combine', 'bias_relu_pool', 'conv3x3_rgb'}
        forced = LG.decisions(trace)
        full = other.expand(*shape)
        v64, g64 = LG.twin_gradient(im0, full, torch.float64, forced, w=w, spatial=spatial, upstream=up)
        v32, g32 = LG.twin_gradient(im0, full, torch.float32, forced, w=w, spatial=spatial, upstream=up)
        d32, d_hip, d_ref = L.rel(leaf.grad, g32), L.rel(leaf.grad, g64), L.rel(g32, g64)
        print('%s %s spatial=%s im1 batch %d: to the float32 twin %.3e; to float64 %.3e, the float32 twin %.3e'
              % (shape, which, spatial, other.shape[0], d32, d_hip, d_ref))
        assert tuple(leaf.grad.shape) == shape and d32 <= 1e-5 and d_hip <= LG.MARGIN * d_ref
        assert L.rel(value, v64) <= 1e-5


def test_nothing_but_im0_receives_a_gradient(emulated, net):
    shape = (1, 3, 16, 16)
    im0, im1 = L.pair(shape, 'independent')
    leaf, w = im0.clone().requires_grad_(True), L.mask(shape)
    target = net.target(im1)
    assert isinstance(target, lpips.Target) and target.size == (16, 16) and target.batch == 1
    assert [tuple(t.shape) for t in target.taps] == [(1, c, 16 >> k, 16 >> k) for k, c in enumerate(lpips.CHANNELS)]
    assert not any(t.requires_grad for t in target.taps)
    net.loss(leaf, target, w=w).sum().backward()
    assert leaf.grad is not None and im1.grad is None and w.grad is None
    assert all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize('shape', L.SHAPES)
def test_the_value_is_forwards(emulated, net, shape):
    """bit for bit: masked, unmasked (a weight of ones) and spatial=False, with im1 and with a reused target, recording a
    gradient and under no_grad -- where nothing is saved -- and unchanged by a second backward"""
    im0, im1 = L.pair(shape, 'near')
    w = L.mask(shape)
    b = shape[0]
    target = net.target(im1)
    want = {('masked', True): net(im0, im1, w=w), ('unmasked', True): net(im0, im1, w=torch.ones_like(w)),
            ('masked', False): net(im0, im1, w=w, spatial=False), ('unmasked', False): net(im0, im1, spatial=False).view(b)}
    for (which, spatial), value in want.items():
        wt = w if which == 'masked' else None
        leaf = im0.clone().requires_grad_(True)
        got = net.loss(leaf, im1, w=wt, spatial=spatial)
        reused = net.loss(leaf, target, w=wt, spatial=spatial)
        assert got.requires_grad and torch.equal(got, value) and torch.equal(reused, value), (which, spatial)
        got.sum().backward(retain_graph=True)
        first = leaf.grad.clone()
        leaf.grad = None
        got.sum().backward()
        assert torch.equal(leaf.grad, first) and torch.equal(got, value)
        leaf.grad = None
        reused.sum().backward()
        assert torch.equal(leaf.grad, first)
        with torch.no_grad():
            quiet = net.loss(leaf, target, w=wt, spatial=spatial)
        plain = net.loss(im0, target, w=wt, spatial=spatial)
        assert not quiet.requires_grad and not plain.requires_grad and torch.equal(quiet, value) and torch.equal(plain, value)


def test_under_no_grad_nothing_is_saved(emulated, net, monkeypatch):
    im0, im1 = L.pair((1, 3, 16, 16), 'box')
    kept = []
    inner = lpips._evaluate
    monkeypatch.setattr(lpips, '_evaluate', lambda *a, **kw: kept.append(kw['keep']) or inner(*a, **kw))
    with torch.no_grad():
        net.loss(im0.clone().requires_grad_(True), im1)
    net.loss(im0, im1)
    net.loss(im0.clone().requires_grad_(True), im1)
    assert kept == [False, False, True]


# ------------------------------------------------------------------------------------------ adjoint_table
def test_adjoint_table_ranges_cover_exactly_the_outputs_that_read_an_input():
    for n_in in range(1, 10):
        for n_out in range(n_in, 41):
            i0, i1, _ = lpips.upsample_table(n_in, n_out)
            lo, hi = lpips.adjoint_table(n_in, n_out)
            assert lo.shape == hi.shape == (n_in,) and lo.dtype.name == hi.dtype.name == 'int32'
            assert not lo.flags.writeable and not hi.flags.writeable
            for i in range(n_in):
                touching = [o for o in range(n_out) if i0[o] == i or i1[o] == i]
                assert touching == list(range(lo[i], hi[i])), (n_in, n_out, i)
    assert lpips.adjoint_table(3, 7) is lpips.adjoint_table(3, 7)
    lo, hi = lpips.adjoint_table(7, 3)                          # fewer outputs than inputs: some inputs are read by none
    i0, i1, _ = lpips.upsample_table(7, 3)
    for i in range(7):
        assert [o for o in range(3) if i0[o] == i or i1[o] == i] == list(range(lo[i], hi[i]))
    flat = lpips.device_adjoint_tables(((5, 7), (2, 3)), (20, 28), 'cpu')
    assert flat.dtype == torch.int32 and tuple(flat.shape) == (2 * (5 + 7 + 2 + 3),)
    assert flat[:5].tolist() == lpips.adjoint_table(5, 20)[0].tolist() and flat[17:24].tolist() == lpips.adjoint_table(7, 28)[1].tolist()
    assert flat[24:26].tolist() == lpips.adjoint_table(2, 20)[0].tolist()
    assert lpips.device_adjoint_tables(((5, 7), (2, 3)), (20, 28), 'cpu') is flat


@pytest.mark.parametrize('tap,size', [((5, 7), (20, 28)), ((1, 1), (16, 16)), ((4, 4), (4, 4)), ((3, 9), (17, 40))])
def test_the_adjoint_stand_in_is_the_transpose(tap, size):
    """<up(d), G> == <d, up^T(G)> in float64, up = F.interpolate and up^T the gather over the ranges"""
    gen = torch.Generator().manual_seed(tap[0] + size[1])
    d = torch.rand(2, *tap, generator=gen, dtype=torch.float64)
    g = torch.rand(2, 1, *size, generator=gen, dtype=torch.float64)
    idx, lam = lpips.device_tables((tap,), size, 'cpu')
    back, = LG.lpips_combine_grad((tap,), (idx, lam.double()), lpips.device_adjoint_tables((tap,), size, 'cpu'), size,
                                  torch.ones(2, dtype=torch.float64), weight=g)
    # the gather, written out over the ranges
    (ylo, yhi), (xlo, xhi) = lpips.adjoint_table(tap[0], size[0]), lpips.adjoint_table(tap[1], size[1])
    my, mx = LG.axis_matrix(tap[0], size[0], lam=lam[0, :size[0]]), LG.axis_matrix(tap[1], size[1], lam=lam[0, size[0]:])
    gathered = torch.zeros_like(d)
    for i in range(tap[0]):
        for j in range(tap[1]):
            window = g[:, 0, ylo[i]:yhi[i], xlo[j]:xhi[j]]
            gathered[:, i, j] = torch.einsum('o,bop,p->b', my[ylo[i]:yhi[i], i], window, mx[xlo[j]:xhi[j], j])
    assert (gathered - back).abs().max().item() <= 1e-13
    # against torch's own operator (float64 tables there: lam rounds to float32 on the way to the device)
    up = F.interpolate(d[:, None], size=size, mode='bilinear', align_corners=False)
    lhs, rhs = (up * g).sum().item(), (d * back).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)
    exact, = LG.lpips_combine_grad((tap,), (idx, torch.from_numpy(
        __import__('numpy').concatenate([lpips.upsample_table(tap[0], size[0])[2], lpips.upsample_table(tap[1], size[1])[2]]))[None]),
        lpips.device_adjoint_tables((tap,), size, 'cpu'), size, torch.ones(2, dtype=torch.float64), weight=g)
    assert abs(lhs - (d * exact).sum().item()) <= 1e-12 * abs(lhs)


# ------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_loss(emulated, net, monkeypatch):
    im = torch.zeros(2, 3, 16, 16)
    leaf = im.clone().requires_grad_(True)
    net.loss(leaf, im)
    with pytest.raises(RuntimeError, match='the target requires a gradient'):
        net.loss(leaf, im.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='the weight requires a gradient'):
        net.loss(leaf, im, w=torch.ones(2, 1, 16, 16, requires_grad=True))
    with torch.no_grad():
        net.loss(leaf, im.clone().requires_grad_(True))
    for bad in (torch.ones(2, 16, 16), torch.ones(3, 1, 16, 16), torch.ones(2, 1, 16, 8)):
        with pytest.raises(ValueError, match=r'\(B or 1, 1, H, W\)'):
            net.loss(leaf, im, w=bad)
    with pytest.raises(ValueError, match='at least 16 x 16'):
        net.loss(leaf[:, :, :15], im[:, :, :15])
    with pytest.raises(ValueError, match='at least 16 x 16'):
        net.target(im[:, :, :, :15])
    with pytest.raises(ValueError, match='sizes must match'):
        net.loss(leaf, net.target(torch.zeros(2, 3, 16, 20)))
    with pytest.raises(ValueError, match='sizes must match'):
        net.loss(leaf, net.target(torch.zeros(3, 3, 16, 16)))
    with pytest.raises(RuntimeError, match='fp32 only'):
        net.loss(leaf.double(), im)
    net.lins[2].requires_grad_(True)
    try:
        with pytest.raises(RuntimeError, match='lins.2 requires a gradient'):
            net.loss(leaf, im)
    finally:
        net.lins[2].requires_grad_(False)
    with pytest.raises(TypeError, match='lpips.LPIPS'):
        lpips.OverfitTerm(torch.nn.Identity())
    # forward is as before: a metric that refuses gradients
    with pytest.raises(RuntimeError, match='forward only'):
        net(leaf, im)
    monkeypatch.setattr(hip, 'on_device', lambda t: bool(t.is_cuda))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.loss(leaf, im)


def test_the_wrappers_refuse_before_any_call(monkeypatch):
    def no_call():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(hip, 'lib', no_call)
    f, lin, gd = torch.zeros(2, 4, 3, 3), torch.zeros(4), torch.zeros(2, 3, 3)
    tables = lpips.device_tables(((3, 3),), (6, 6), 'cpu')
    ranges = lpips.device_adjoint_tables(((3, 3),), (6, 6), 'cpu')
    scale = torch.ones(2)
    for call in (lambda: hip.lpips_tap_grad(f, f, lin, gd), lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges, (6, 6), scale)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))      # past the device check, on the host
    for call in (lambda: hip.lpips_tap_grad(f.double(), f, lin, gd), lambda: hip.lpips_tap_grad(f, f, lin, gd.double()),
                 lambda: hip.lpips_tap_grad(f, f, lin, gd, acc=f.half()), lambda: hip.lpips_tap_grad(f, f, lin, gd, out=f.double()),
                 lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges, (6, 6), scale.double()),
                 lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges, (6, 6), scale, weight=torch.ones(2, 1, 6, 6).double())):
        with pytest.raises(RuntimeError, match='fp32 only'):
            call()
    with pytest.raises(RuntimeError, match='takes torch.int32'):
        hip.lpips_combine_grad(((3, 3),), tables, ranges.long(), (6, 6), scale)
    with pytest.raises(RuntimeError, match='contiguous'):
        hip.lpips_tap_grad(f, f, lin, gd, acc=f.transpose(2, 3))
    for call in (lambda: hip.lpips_tap_grad(f, torch.zeros(3, 4, 3, 3), lin, gd), lambda: hip.lpips_tap_grad(f, f, torch.zeros(5), gd),
                 lambda: hip.lpips_tap_grad(f, f, lin, torch.zeros(2, 1, 3, 3)), lambda: hip.lpips_tap_grad(f, f, lin, gd[:1]),
                 lambda: hip.lpips_tap_grad(f, f, lin, gd, acc=f[:1]), lambda: hip.lpips_tap_grad(f, f, lin, gd, out=f[:, :2].contiguous()),
                 lambda: hip.lpips_combine_grad((), tables, ranges, (6, 6), scale),
                 lambda: hip.lpips_combine_grad(((3, 3),) * 9, tables, ranges, (6, 6), scale),
                 lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges, (6, 7), scale),
                 lambda: hip.lpips_combine_grad(((3, 4),), tables, ranges, (6, 6), scale),
                 lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges[:-1], (6, 6), scale),
                 lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges, (6, 6), torch.ones(2, 1)),
                 lambda: hip.lpips_combine_grad(((3, 3),), tables, ranges, (6, 6), scale, weight=torch.ones(3, 1, 6, 6))):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------ all_weights_insert
def test_all_weights_insert_takes_a_perceptual_term_and_is_unchanged_without(emulated, net, monkeypatch):
    from rewriting_amd import perceptual
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    from tests import grad_emulation
    from tests.conftest import build_stylegan
    grad_emulation.install(monkeypatch)                 # ToRGB's adjoints (the generator's backward)
    model = build_stylegan(32, 0.5)
    gw = ganrewrite.SeqStyleGanRewriter(model, zdataset.z_dataset_for_model(model, size=4), 6, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    monkeypatch.delenv(perceptual.WEIGHTS_ENV, raising=False)
    with pytest.raises(NotImplementedError, match='feature_net.*RW_VGG16_WEIGHTS'):          # as before
        gw.all_weights_insert(x, z, niter=1)
    with pytest.raises(TypeError, match='callable'):
        gw.all_weights_insert(x, z, niter=1, perceptual=0.5)
    with pytest.raises(TypeError, match='callable'):
        gw.apply_overfit({'object': [2, None], 'paste': [3, None]}, niter=1, perceptual='lpips')
    term = lpips.OverfitTerm(net, weight=0.5)
    built = []
    inner = net.target
    monkeypatch.setattr(net, 'target', lambda im: built.append(tuple(im.shape)) or inner(im))
    losses, bounds = [], (8, 8, 24, 24)
    before = {k: v.detach().clone() for k, v in gw.model.state_dict().items()}
    with torch.no_grad():
        pred = gw.model(z)[:, :, 8:24, 8:24]
        want = F.l1_loss(x[:, :, 8:24, 8:24], pred) + 0.5 * net(pred, x[:, :, 8:24, 8:24], spatial=False).mean()
    gw.all_weights_insert(x, z, bounds=bounds, niter=2, lr=0.01, perceptual=term,
                          update_callback=lambda it, loss: losses.append(loss.item()))
    assert built == [(1, 3, 16, 16)] and len(losses) == 2               # the constant side ran once, no feature_net was resolved
    assert abs(losses[0] - want.item()) <= 1e-6 * abs(want.item()) and losses[1] != losses[0]
    after = gw.model.state_dict()
    assert not [name for name, _ in gw.model.named_parameters() if torch.equal(after[name], before[name])]


# ------------------------------------------------------------------------------------------ the ABI
def test_the_entries_are_bound_and_exported():
    assert _lib.ABI_VERSION == 11
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert not name.endswith('_supported') and not name.startswith('rw_packed_')
    assert ctypes.sizeof(_lib.LpipsGradMaps) == ctypes.sizeof(_lib.LpipsMaps)
    load = _lib.load()
    null = ctypes.c_void_p(0)
    assert load.rw_lpips_tap_grad_f32(null, null, null, null, null, null, 1, 1, 1, 1, 0, null) != 0
    assert load.rw_lpips_combine_grad_f32(None, null, null, null, null, 0, null, 1, 1, 1, null) != 0
