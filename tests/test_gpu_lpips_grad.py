"""LPIPS as a loss on the device (rw_lpips.hip: rw_lpips_tap_grad_f32, rw_lpips_combine_grad_f32; rewriting_amd/lpips.py:
LPIPS.loss, OverfitTerm): the tap adjoint against float64 autograd of the formula (bar: 8 times the float32 autograd's own
error, DESIGN section 8.1's margin), the combine adjoint against float64 autograd within the bound of its summation order, the
whole node against the twin of tests/lpips_grad_checks.py on the device's own ReLU and pool decisions, and all_weights_insert
with the LPIPS term.  Every kernel twice, bit for bit.  Figures go to lpips_grad.json in the directory RW_REPORT_DIR names
(default: test_reports/, which git ignores); DESIGN section 8.8 copies them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_checks as L
from tests import lpips_grad_checks as LG

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN, D_REF_MAX = LG.MARGIN, LG.D_REF_MAX
EPS = L.EPS


randn, on_device = L.randn, L.on_device


# ------------------------------------------------------------------------------------------ the tap adjoint: the forward's cases
def tap_inputs(shape, f1_batch, kind, seed):
    """(f0, f1, lin, gd, dead): ReLU outputs (about half of f0's elements are 0); with more than two pixels, pixel (0, 0) is
    zero in both maps, (0, 1) in f0 only and the last one in f1 only; dead: the pixels whose f0 is all zero"""
    lin = torch.rand(shape[1], generator=torch.Generator().manual_seed(seed)) * (randn(shape[1:2], seed + 1) < 0.5)
    f0 = F.relu(randn(shape, seed + 2))
    f1_shape = (f1_batch,) + shape[1:]
    f1 = F.relu(randn(f1_shape, seed + 3)) if kind == 'independent' else F.relu(f0[:f1_batch] + 1e-3 * randn(f1_shape, seed + 4))
    if shape[2] * shape[3] > 2:
        f0[:, :, 0, 0] = 0
        f1[:, :, 0, 0] = 0
        f0[:, :, 0, 1] = 0
        f1[:, :, -1, -1] = 0
    gd = torch.rand(shape[0], *shape[2:], generator=torch.Generator().manual_seed(seed + 5)) + 0.1
    return f0, f1, lin, gd, (f0 ** 2).sum(1) == 0


def tap_autograd(f0, f1, lin, gd, dead, dtype):
    """d (sum gd d) / d f0 of the zero-safe formula in `dtype`; at a dead pixel the kernel's rule: exactly 0 (the formula has
    a 1 / 1e-10 spike there)"""
    leaf = f0.clone().to(dtype).requires_grad_(True)
    (LG.tap_distance(leaf, f1, lin, dtype)[:, 0] * gd.to(dtype)).sum().backward()
    return leaf.grad * ~dead[:, None]


@pytest.mark.parametrize('shape,f1_batch,offset', L.TAP_CASES)
def test_tap_adjoint_against_float64_autograd(shape, f1_batch, offset):
    """d_hip <= 8 d_ref (2-norm; d_ref the float32 autograd's error, below 1e-5 on the independent maps up to 512 channels);
    dead pixels exactly 0, a pixel zero in f1 only finite and inside the bar; acc is added exactly, out may be acc, relu_mask
    leaves acc where f0 <= 0 and changes nothing else; twice, bit for bit."""
    from rewriting_amd import hip
    seed = 11 + shape[1] + 7 * f1_batch + offset
    rows = {}
    for kind in ('independent', 'near'):
        f0, f1, lin, gd, dead = tap_inputs(shape, f1_batch, kind, seed)
        want, ref = (tap_autograd(f0, f1, lin, gd, dead, dtype) for dtype in (torch.float64, torch.float32))
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(ref).all())
        f0d, f1d, lind, gdd = on_device(f0, offset), on_device(f1), lin.to(DEV), gd.to(DEV)
        got = hip.lpips_tap_grad(f0d, f1d, lind, gdd)
        assert tuple(got.shape) == shape and torch.equal(got, hip.lpips_tap_grad(f0d, f1d, lind, gdd))
        assert bool(torch.isfinite(got).all()) and not got.cpu()[dead[:, None].expand(*shape)].any()
        d_hip, d_ref = L.rel(got.cpu(), want), L.rel(ref, want)
        rows[kind] = dict(d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref)
        print('tap adjoint %s f1 batch %d offset %d %s: d_hip %.3e d_ref %.3e ratio %.2f'
              % (shape, f1_batch, offset, kind, d_hip, d_ref, d_hip / d_ref))
        assert d_hip <= MARGIN * d_ref, (kind, d_hip, d_ref)
        assert d_ref < D_REF_MAX or kind == 'near' or shape[1] > 512, (kind, d_ref)
        if shape[2] * shape[3] > 2:                         # the pixel that is zero in f1 only, by itself
            last = (got.cpu()[:, :, -1, -1], want[:, :, -1, -1], ref[:, :, -1, -1])
            assert L.rel(last[0], last[1]) <= MARGIN * max(L.rel(last[2], last[1]), EPS)
        acc = on_device(randn(shape, seed + 6), offset)
        summed = hip.lpips_tap_grad(f0d, f1d, lind, gdd, acc=acc)
        assert torch.equal(summed, acc + got)
        alias = acc.clone()
        assert hip.lpips_tap_grad(f0d, f1d, lind, gdd, acc=alias, out=alias).data_ptr() == alias.data_ptr() and torch.equal(alias, summed)
        masked = hip.lpips_tap_grad(f0d, f1d, lind, gdd, acc=acc, relu_mask=True)
        assert torch.equal(masked, torch.where(f0d > 0, summed, acc))
        assert torch.equal(hip.lpips_tap_grad(f0d, f1d, lind, gdd, relu_mask=True), torch.where(f0d > 0, got, torch.zeros_like(got)))
    LG.report('tap_%s_f1b%d_off%d' % ('x'.join(map(str, shape)), f1_batch, offset), rows)


# ------------------------------------------------------------------------------------------ the combine adjoint
# (tap sizes, output size): the pyramid of a 32 x 32 image; of a 20 x 28 one (the floors of the pools); one tap at its own size
# (spatial=False's form); one 1 x 1 tap under a 16 x 16 weight
COMBINE_CASES = [(((32, 32), (16, 16), (8, 8), (4, 4), (2, 2)), (32, 32)), (((20, 28), (10, 14), (5, 7), (2, 3), (1, 1)), (20, 28)),
                 (((5, 7),), (5, 7)), (((1, 1),), (16, 16))]


@pytest.mark.parametrize('sizes,size', COMBINE_CASES)
def test_combine_adjoint_against_float64_autograd(sizes, size):
    """Per element |err| <= 1.01 (|R_x| + |R_y| + 4) 2^-24 sum |term|: a term passes through |R_x| additions along its row and
    |R_y| across the rows (rw_lpips.hip: a row's columns first, then the rows; each a fused multiply-add), the roundings of its
    two weights 1 - lam and the product with gscale -- |R_x| + |R_y| + 3 roundings, derived, not measured.  The reference is
    float64 autograd of lpips_checks.apply_tables on the tables the device reads.  weight of batch B, of batch 1 and none."""
    from rewriting_amd import hip, lpips
    batch = 2
    tables = lpips.device_tables(sizes, size, DEV)
    ranges = lpips.device_adjoint_tables(sizes, size, DEV)
    idx, lam = (t.cpu() for t in tables)
    gscale = torch.rand(batch, generator=torch.Generator().manual_seed(2)) + 0.5
    weights = {'per image': randn((batch, 1) + size, 3), 'batch 1': (torch.rand(1, 1, *size, generator=torch.Generator().manual_seed(4)) > 0.3).float(),
               'none': None}
    figures = {}
    for name, w in weights.items():
        w64 = torch.ones(batch, *size, dtype=torch.float64) if w is None else w.double()[:, 0].expand(batch, *size)
        wants, bounds = [], []
        for k, (hk, wk) in enumerate(sizes):
            for magnitude in (False, True):
                leaf = torch.zeros(batch, hk, wk, dtype=torch.float64, requires_grad=True)
                up = L.apply_tables(leaf, idx[k], lam[k], size)
                (up * (w64.abs() if magnitude else w64) * gscale.double()[:, None, None]).sum().backward()
                (bounds if magnitude else wants).append(leaf.grad)
            (ylo, yhi), (xlo, xhi) = lpips.adjoint_table(hk, size[0]), lpips.adjoint_table(wk, size[1])
            chain = torch.from_numpy((yhi - ylo).copy())[:, None] + torch.from_numpy((xhi - xlo).copy())[None, :] + 4
            bounds[-1] = 1.01 * chain.double() * EPS * bounds[-1]
        wd = None if w is None else w.to(DEV)
        got = hip.lpips_combine_grad(sizes, tables, ranges, size, gscale.to(DEV), weight=wd)
        again = hip.lpips_combine_grad(sizes, tables, ranges, size, gscale.to(DEV), weight=wd)
        worst = 0.0
        for g, g2, want, bound, (hk, wk) in zip(got, again, wants, bounds, sizes):
            assert tuple(g.shape) == (batch, hk, wk) and torch.equal(g, g2)
            err = (g.cpu().double() - want).abs()
            worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
            assert bool((err <= bound).all()), (name, (hk, wk), (err / bound.clamp_min(1e-300)).max().item())
        print('combine adjoint %s -> %s, w %s: worst err / bound %.3f' % (sizes, size, name, worst))
        figures['err_over_bound_w_' + name.replace(' ', '_')] = worst
    LG.report('combine_%s_to_%dx%d' % ('_'.join('%dx%d' % s for s in sizes), size[0], size[1]), figures)


def test_combine_adjoint_clamps_wrong_tables():
    """ranges and indices far outside give a wrong picture, never an access outside a map: the result stays finite and bounded by
    the weights' sum"""
    from rewriting_amd import hip, lpips
    sizes, size = ((3, 3),), (6, 6)
    idx, lam = lpips.device_tables(sizes, size, DEV)
    ranges = lpips.device_adjoint_tables(sizes, size, DEV)
    wrong_ranges = ranges.clone()
    wrong_ranges[::2] = -(1 << 20)
    wrong_ranges[1::2] = 1 << 20
    wrong_idx = idx.clone()
    wrong_idx[:, ::2] = 1 << 20
    w = torch.rand(1, 1, 6, 6, generator=torch.Generator().manual_seed(9)).to(DEV)
    one = torch.ones(1, device=DEV)
    for tables, rng in (((idx, lam), wrong_ranges), ((wrong_idx, lam), ranges), ((wrong_idx, lam), wrong_ranges)):
        got, = hip.lpips_combine_grad(sizes, tables, rng, size, one, weight=w)
        assert bool(torch.isfinite(got).all()) and bool((got >= 0).all()) and got.max().item() <= w.sum().item() * (1 + 64 * EPS)


def test_wrappers_refuse_on_the_device():
    from rewriting_amd import hip, lpips
    f, lin, gd = torch.zeros(1, 4, 3, 3, device=DEV), torch.zeros(4, device=DEV), torch.zeros(1, 3, 3, device=DEV)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.lpips_tap_grad(f, f, lin, gd.cpu())
    with pytest.raises(RuntimeError, match='fp32 only'):
        hip.lpips_tap_grad(f, f.double(), lin, gd)
    with pytest.raises(ValueError):
        hip.lpips_tap_grad(f, f, lin, gd[:, :2].contiguous())
    with pytest.raises(ValueError):
        hip.lpips_tap_grad(f, f, lin, gd, acc=f[:, :2].contiguous())
    sizes = ((3, 3),)
    tables, ranges = lpips.device_tables(sizes, (6, 6), DEV), lpips.device_adjoint_tables(sizes, (6, 6), DEV)
    scale = torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.lpips_combine_grad(sizes, tables, ranges, (6, 6), scale.cpu())
    with pytest.raises(RuntimeError, match='fp32 only'):
        hip.lpips_combine_grad(sizes, tables, ranges, (6, 6), scale.double())
    with pytest.raises(ValueError):
        hip.lpips_combine_grad(sizes, tables, ranges[:-1].contiguous(), (6, 6), scale)
    with pytest.raises(ValueError, match='1 .. %d tap maps' % hip.LPIPS_MAX_TAPS):
        hip.lpips_combine_grad(sizes * (hip.LPIPS_MAX_TAPS + 1), tables, ranges, (6, 6), scale)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        network().loss(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


# ------------------------------------------------------------------------------------------ the whole node
@functools.lru_cache(maxsize=None)
def network():
    from rewriting_amd import lpips
    return lpips.from_state_dicts(*L.weights()).to(DEV)


def module_gradient(shape, kind, w, spatial, tag):
    """One form of the loss on pair(shape, kind): the value against forward's, bit for bit; a reused target, bit for bit; the
    gradient against the twins on the device's decisions.  Returns the row of figures."""
    net = network()
    im0, im1 = L.pair(shape, kind)
    im0d, im1d = im0.to(DEV), im1.to(DEV)
    wd = None if w is None else w.to(DEV)
    with torch.no_grad():
        if spatial:
            value = net(im0d, im1d, w=wd if wd is not None else torch.ones(shape[0], 1, *shape[2:], device=DEV))
        else:
            value = net(im0d, im1d, w=wd, spatial=False).view(shape[0])
    leaf = im0d.clone().requires_grad_(True)
    trace = []
    got = net.loss(leaf, im1d, w=wd, spatial=spatial, trace=trace)
    assert tuple(got.shape) == (shape[0],) and torch.equal(got, value) and len(trace) == 13
    got.sum().backward()
    assert tuple(leaf.grad.shape) == shape and im1d.grad is None
    again = im0d.clone().requires_grad_(True)
    reused = net.loss(again, net.target(im1d), w=wd, spatial=spatial)
    reused.sum().backward()
    assert torch.equal(reused, value) and torch.equal(again.grad, leaf.grad)
    forced, own = LG.decisions(trace), []
    v64, g64 = LG.twin_gradient(im0, im1, torch.float64, forced, w=w, spatial=spatial)
    _, g32 = LG.twin_gradient(im0, im1, torch.float32, forced, w=w, spatial=spatial)
    LG.tap_features(L.weights()[0], im0, torch.float64, own=own)
    relu_share, pool_share = LG.P.differing_share(forced, own)
    d_hip, d_ref = L.rel(leaf.grad.cpu(), g64), L.rel(g32, g64)
    print('lpips loss %s %s %s: d_hip %.3e d_ref %.3e ratio %.2f; value rel %.2e; decisions differing from float64: relu %.2e '
          'pool %.2e' % (shape, kind, tag, d_hip, d_ref, d_hip / d_ref, L.rel(got.cpu(), v64), relu_share, pool_share))
    return dict(d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref, value_rel=L.rel(got.cpu(), v64),
                relu_decisions_differing=relu_share, pool_decisions_differing=pool_share)


@pytest.mark.parametrize('kind', L.KINDS)
@pytest.mark.parametrize('shape', L.SHAPES)
def test_loss_gradient_against_the_float64_twin(shape, kind):
    """d (masked scalar) / d im0, the device's ReLU and pool decisions forced on both twins: independent and box
    d_ref < 1e-5 and d_hip <= 8 d_ref; near d_hip <= 8 d_ref alone, both figures recorded -- the metric amplifies rounding by
    1 / |n0 - n1| there, and the float32 twin itself is outside the cap (1.5e-5 .. 2.4e-5 on the host)."""
    row = module_gradient(shape, kind, L.mask(shape), True, 'masked')
    LG.report('loss_%dx%dx%d_%s' % (shape[0], shape[2], shape[3], kind), row)
    assert row['d_hip'] <= MARGIN * row['d_ref'], row
    assert kind == 'near' or row['d_ref'] < D_REF_MAX, row


@pytest.mark.parametrize('spatial', [True, False], ids=['unmasked', 'spatial_false'])
def test_loss_gradient_of_the_unweighted_forms(spatial):
    shape = (2, 3, 32, 32)
    row = module_gradient(shape, 'independent', None, spatial, 'unmasked' if spatial else 'spatial=False')
    LG.report('loss_2x32x32_independent_%s' % ('unmasked' if spatial else 'spatial_false'), row)
    assert row['d_ref'] < D_REF_MAX and row['d_hip'] <= MARGIN * row['d_ref'], row


# ------------------------------------------------------------------------------------------ the overfit loop
def overfit_loss(sd, x, z, bounds, size, truncation, weight=1.0):
    """all_weights_insert's loss with perceptual=OverfitTerm(net, weight) of the float64 restatement at the state `sd`
    (modelled on generator_gradient_checks.overfit_loss): l1 + weight * the twin's LPIPS, spatial=False, mean over the batch"""
    from oracle import restatement as R
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    vgg, lins = L.weights()
    t, l, b, r = bounds
    with torch.no_grad():
        out = R.generator_forward(sd, z.double(), size, truncation=truncation)
        gt, pred = x.double()[:, :, t:b, l:r], out[:, :, t:b, l:r]
        return (F.l1_loss(gt, pred) + weight * L.twin(vgg, lins, pred, gt, torch.float64, spatial=False).mean()).item()


def test_all_weights_insert_with_the_lpips_term(monkeypatch):
    """size 32, crop (8, 8, 24, 24), two iterations, no feature_net and no RW_VGG16_WEIGHTS: the loss reported at iteration 0
    within 1e-5 of the float64 restatement's l1 + twin LPIPS (the bar generator_gradient_checks.overfit_loss's users hold),
    every parameter moved, the target built once."""
    from rewriting_amd import lpips, perceptual
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    from tests.conftest import build_stylegan, oracle_state_dict
    size, bounds, truncation = 32, (8, 8, 24, 24), 0.5
    model = build_stylegan(size, truncation, device=DEV)
    gw = ganrewrite.SeqStyleGanRewriter(model, zdataset.z_dataset_for_model(model, size=4), 6, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    before = oracle_state_dict(gw.model)
    want = overfit_loss(before, x.cpu(), z.cpu(), bounds, size, truncation)
    monkeypatch.delenv(perceptual.WEIGHTS_ENV, raising=False)
    net = network()
    built, inner = [], net.target
    monkeypatch.setattr(net, 'target', lambda im: built.append(tuple(im.shape)) or inner(im))
    losses = []
    gw.all_weights_insert(x, z, bounds=bounds, niter=2, lr=0.01, feature_net=None, perceptual=lpips.OverfitTerm(net),
                          update_callback=lambda it, loss: losses.append(loss.item()))
    print('all_weights_insert (LPIPS term): loss %.8f, float64 %.8f' % (losses[0], want))
    LG.report('all_weights_insert_lpips', dict(loss=losses[0], loss_float64=want, rel=abs(losses[0] - want) / abs(want)))
    assert len(losses) == 2 and abs(losses[0] - want) <= 1e-5 * abs(want), (losses, want)
    assert built == [(1, 3, 16, 16)]
    after = gw.model.state_dict()
    still = [name for name, _ in gw.model.named_parameters() if torch.equal(after[name].cpu(), before[name])]
    assert not still, 'parameters that did not move: %s' % still
