"""LPIPS on the device (rw_lpips.hip, rewriting_amd/lpips.py, rewriting_amd/distances.py): the tap kernel against the float64
formula (bar: 8 times the float32 torch formula's own error, DESIGN section 8.1's margin -- on nearly equal maps an expanded,
cancelling form misses it by orders of magnitude), the combine kernel and the masked L1 against float64 with the bounds of
their chains of rounded operations, the whole module against the float64 twin of tests/lpips_checks.py, and edit_distance in its
three modes.  Every kernel twice, bit for bit.  Figures go to lpips.json in the directory RW_REPORT_DIR names (default:
test_reports/, which git ignores); DESIGN section 8.7 copies them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_checks as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 8                          # d_hip <= MARGIN * d_ref
D_REF_MAP, D_REF_TAP = 2e-5, 5e-5   # the conditions on the reference alone (tests/test_lpips_host.py asserts them on the host)
EPS = L.EPS


randn, on_device = L.randn, L.on_device


# ------------------------------------------------------------------------------------------ the tap kernel
@pytest.mark.parametrize('shape,f1_batch,offset', L.TAP_CASES)
def test_tap_kernel_against_the_float64_formula(shape, f1_batch, offset):
    """maps as taps are (ReLU outputs); independent, near (f1 = f0 + 1e-3 noise), a pixel all-zero in both maps (exactly 0), a
    pixel zero in one map only.  d_hip <= 8 d_ref, 2-norm, d_ref the float32 torch formula's error."""
    from rewriting_amd import hip
    seed = 11 + shape[1] + 7 * f1_batch + offset
    lin = torch.rand(shape[1], generator=torch.Generator().manual_seed(seed)) * (randn(shape[1:2], seed + 1) < 0.5)
    f0 = F.relu(randn(shape, seed + 2)) + 0.01
    f1_shape = (f1_batch,) + shape[1:]
    inputs = {'independent': F.relu(randn(f1_shape, seed + 3)),
              'near': F.relu(f0[:f1_batch] + 1e-3 * randn(f1_shape, seed + 4))}
    rows = {}
    for kind, f1 in inputs.items():
        a, b = f0.clone(), f1.clone()
        several = shape[2] * shape[3] > 1                   # (a map of one pixel keeps it: all-zero, there is nothing to compare)
        if several:
            a[:, :, 0, 0] = 0
            b[:, :, 0, 0] = 0                               # a pixel all-zero in both maps
            b[:, :, -1, -1] = 0                             # and one that is zero in one map only
        want = L.tap_distance(a, b, lin, torch.float64)[:, 0]
        ref = L.tap_distance(a, b, lin, torch.float32)[:, 0]
        ad, bd, lind = on_device(a, offset), on_device(b), lin.to(DEV)
        got = hip.lpips_tap(ad, bd, lind)
        assert tuple(got.shape) == (shape[0],) + shape[2:] and torch.equal(got, hip.lpips_tap(ad, bd, lind))
        assert not (several and got[:, 0, 0].any()) and bool(torch.isfinite(got).all())
        d_hip, d_ref = L.rel(got.cpu(), want), L.rel(ref, want)
        print('tap %s f1 batch %d offset %d %s: d_hip %.3e d_ref %.3e ratio %.2f' % (shape, f1_batch, offset, kind, d_hip, d_ref,
                                                                                    d_hip / d_ref))
        rows[kind] = dict(d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref)
        assert d_hip <= MARGIN * d_ref, (kind, d_hip, d_ref)
    L.report('tap_%s_f1b%d_off%d' % ('x'.join(map(str, shape)), f1_batch, offset), rows)


# ------------------------------------------------------------------------------------------ the combine kernel
def pyramid(size, batch, seed):
    """nonnegative tap maps of an image of `size`: sizes H >> k, W >> k, k = 0 .. 4"""
    return [torch.rand(batch, size[0] >> k, size[1] >> k, generator=torch.Generator().manual_seed(seed + k)) * (k + 1)
            for k in range(5)]


def corner_bound(taps, size):
    """sum_k (largest of the four corner values of tap k), gathered with the host tables: (B, H, W) float64"""
    from rewriting_amd import lpips
    total = 0
    for d in taps:
        y0, y1, _ = (torch.from_numpy(t.copy()).long() for t in lpips.upsample_table(d.shape[1], size[0]))
        x0, x1, _ = (torch.from_numpy(t.copy()).long() for t in lpips.upsample_table(d.shape[2], size[1]))
        d = d.double()
        corners = torch.stack([d[:, y0][:, :, x0], d[:, y0][:, :, x1], d[:, y1][:, :, x0], d[:, y1][:, :, x1]])
        total = total + corners.max(dim=0).values
    return total


@pytest.mark.parametrize('size', [(20, 28), (32, 32)])
def test_combine_kernel_against_float64(size):
    """the map: |err| <= 1.01 * 32 * 2^-24 * sum_k (largest corner value of tap k), elementwise (nonnegative inputs: whatever the
    form of the four-term sum).  The sums: |err| <= (n + 32) 2^-24 value with n = 62, the longest chain of additions a term passes
    through in rw_lpips.hip's reduction (28 per thread + 6 + 3 in the workgroup, 16 + 6 + 3 in the finishing one; here 1 + 9 +
    1 + 9).  The null-map and null-sums forms, w of batch 1 and no w, the spatial=False form; each twice, bit for bit."""
    from rewriting_amd import hip, lpips
    batch = 2
    taps = pyramid(size, batch, 5 + size[0])
    assert [tuple(d.shape[1:]) for d in taps] == ([(20, 28), (10, 14), (5, 7), (2, 3), (1, 1)] if size[0] == 20 else
                                                  [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)])
    want = sum(F.interpolate(d.double()[:, None], size=size, mode='bilinear', align_corners=False) for d in taps)
    bound = 1.01 * 32 * EPS * corner_bound(taps, size)[:, None]
    tapsd = [d.to(DEV) for d in taps]
    tables = lpips.device_tables([d.shape[1:] for d in taps], size, DEV)
    out, sums = hip.lpips_combine(tapsd, tables, size)
    assert sums is None and tuple(out.shape) == (batch, 1) + size
    err = (out.cpu().double() - want).abs()
    print('combine %s: worst err / bound %.3f' % (size, (err / bound).max().item()))
    assert bool((err <= bound).all()), (err / bound).max().item()
    figures = dict(map_err_over_bound=(err / bound).max().item())
    weights = {'per image': torch.rand(batch, 1, *size, generator=torch.Generator().manual_seed(3)),
               'batch 1': (torch.rand(1, 1, *size, generator=torch.Generator().manual_seed(4)) > 0.3).float(), 'none': None}
    for name, w in weights.items():
        wd = None if w is None else w.to(DEV)
        both = hip.lpips_combine(tapsd, tables, size, weight=wd, want_sums=True)
        only = hip.lpips_combine(tapsd, tables, size, weight=wd, want_map=False, want_sums=True)
        assert only[0] is None and torch.equal(both[0], out) and torch.equal(both[1], only[1])
        assert torch.equal(only[1], hip.lpips_combine(tapsd, tables, size, weight=wd, want_map=False, want_sums=True)[1])
        w64 = torch.ones(batch, 1, *size, dtype=torch.float64) if w is None else w.double().expand(batch, 1, *size)
        value = torch.stack([(want * w64).sum((1, 2, 3)), w64.sum((1, 2, 3))], dim=1)
        err_s = (only[1].cpu().double() - value).abs() / ((L.CHAIN + 32) * EPS * value)
        print('combine %s sums, w %s: worst err / bound %.3f' % (size, name, err_s.max().item()))
        figures['sums_err_over_bound_w_' + name.replace(' ', '_')] = err_s.max().item()
        assert bool((err_s <= 1).all()), err_s
    # spatial=False: the entry at a tap's own size -- (sum d_k, pixels)
    for d, dd in zip(taps, tapsd):
        own = tuple(d.shape[1:])
        _, s = hip.lpips_combine([dd], lpips.device_tables((own,), own, DEV), own, want_map=False, want_sums=True)
        total = d.double().sum((1, 2))
        assert torch.equal(s[:, 1].cpu(), torch.full((batch,), float(own[0] * own[1])))
        assert bool(((s[:, 0].cpu().double() - total).abs() <= (L.CHAIN + 32) * EPS * total).all())
    L.report('combine_%dx%d' % size, figures)


def test_combine_clamps_a_wrong_table():
    """indices far outside the tap's map give a wrong picture, never a read outside it: the result is made of the tap's values"""
    from rewriting_amd import hip, lpips
    d = torch.rand(1, 3, 3, generator=torch.Generator().manual_seed(9)) + 1
    idx, lam = lpips.device_tables(((3, 3),), (6, 6), DEV)
    wrong = idx.clone()
    wrong[:, ::2] = 1 << 20
    wrong[:, 1::2] = -(1 << 20)
    out, _ = hip.lpips_combine([d.to(DEV)], (wrong, lam), (6, 6))
    assert bool((out.cpu() >= d.min()).all()) and bool((out.cpu() <= d.max() * (1 + 4 * EPS)).all())


# ------------------------------------------------------------------------------------------ masked L1
@pytest.mark.parametrize('shape,mask_batch', [((2, 3, 20, 28), 2), ((3, 3, 32, 32), 1), ((1, 3, 5, 7), 1)])
def test_masked_l1_against_float64(shape, mask_batch):
    """|err| <= (n + 3) 2^-24 value, n = 62 (the chain of the reduction; + 3: the differences, their sum and the product with the
    mask); the mask's sum exact.  Twice, bit for bit."""
    from rewriting_amd import hip
    a, b = randn(shape, 1), randn(shape, 2)
    mask = (torch.rand(mask_batch, *shape[2:], generator=torch.Generator().manual_seed(3)) > 0.4).float()
    got = hip.masked_l1(a.to(DEV), b.to(DEV), mask.to(DEV))
    assert tuple(got.shape) == (shape[0], 2) and torch.equal(got, hip.masked_l1(a.to(DEV), b.to(DEV), mask.to(DEV)))
    m64 = mask.double().expand(shape[0], *shape[2:])
    want = ((a.double() - b.double()).abs().sum(1) * m64).sum((1, 2))
    assert torch.equal(got[:, 1].cpu().double(), m64.sum((1, 2)))
    err = (got[:, 0].cpu().double() - want).abs() / ((L.CHAIN + 3) * EPS * want)
    print('masked_l1 %s: worst err / bound %.3f' % (shape, err.max().item()))
    assert bool((err <= 1).all()), err


def test_wrappers_refuse_on_the_device():
    from rewriting_amd import hip
    f, lin = torch.zeros(1, 4, 3, 3, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match='fp32 only'):
        hip.lpips_tap(f.double(), f, lin)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.lpips_tap(f, f.cpu(), lin)
    with pytest.raises(ValueError):
        hip.lpips_tap(f, f, lin[:3])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        network()(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match='at least 16 x 16'):
        network()(torch.zeros(1, 3, 8, 16, device=DEV), torch.zeros(1, 3, 8, 16, device=DEV))


# ------------------------------------------------------------------------------------------ the whole module
@functools.lru_cache(maxsize=None)
def network():
    from rewriting_amd import lpips
    return lpips.from_state_dicts(*L.weights()).to(DEV)


@pytest.fixture
def launches(monkeypatch):
    from tests import route_spy
    log = []
    route_spy.install_spies(monkeypatch, log)
    return log


@pytest.mark.parametrize('kind', L.KINDS)
@pytest.mark.parametrize('shape', L.SHAPES)
def test_module_against_the_float64_twin(shape, kind, launches):
    """the spatial map and every d_k: d_hip <= 8 d_ref with d_ref < 2e-5 (map) / 5e-5 (tap), the float32 twin against the
    float64 one; the masked scalar within 8 times the float32 twin's own relative error; 24 MFMA convolutions + 2 RGB per pair.
    32^2 reaches the F(2x2) form at 32 x 32 and the split-K direct sum below; 20 x 28 the floor of every pool; 16^2 the 1 x 1
    last tap.  Measured on the MI355X: map ratios 0.55 - 1.6, taps 0.12 - 3.9, masked scalars 0.03 - 1.45.  (With the maps below
    32 wide on the routes their shapes take by themselves -- F(2x2) and the serial direct sum, both about twice as far from
    float64 per layer -- the one-number last tap of the 16 x 16 near pair missed the bar at 8.25; it is at 2.23.)"""
    ref64, ref32 = L.reference(shape, kind)[torch.float64], L.reference(shape, kind)[torch.float32]
    im0, im1 = (t.to(DEV) for t in L.pair(shape, kind))
    net = network()
    taps = []
    got = net(im0, im1, taps=taps)
    names = [call.split()[0] for call in launches]
    assert names.count('conv3x3_wino') + names.count('conv3x3') == 24 and names.count('conv3x3_rgb') == 2, launches
    assert torch.equal(got, net(im0, im1)) and not got.requires_grad
    rows, bad = [], []
    pairs = [('map', got.cpu(), ref64[0], ref32[0], D_REF_MAP)]
    pairs += [('d%d' % k, d.cpu()[:, None], ref64[1][k], ref32[1][k], D_REF_TAP) for k, d in enumerate(taps)]
    for name, mine, want, want32, d_ref_max in pairs:
        d_hip, d_ref = L.rel(mine, want), L.rel(want32, want)
        rows.append(dict(what=name, d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref))
        print('lpips %s %s %s: d_hip %.3e d_ref %.3e ratio %.2f' % (shape, kind, name, d_hip, d_ref, d_hip / d_ref))
        if not (d_ref < d_ref_max and d_hip <= MARGIN * d_ref):
            bad.append(rows[-1])
    scalar = net(im0, im1, w=L.mask(shape).to(DEV))
    assert tuple(scalar.shape) == (shape[0],) and torch.equal(scalar, net(im0, im1, w=L.mask(shape).to(DEV)))
    s_hip, s_ref = L.rel(scalar.cpu(), ref64[2]), L.rel(ref32[2], ref64[2])
    print('lpips %s %s masked scalar: hip %.3e float32 twin %.3e ratio %.2f' % (shape, kind, s_hip, s_ref, s_hip / max(s_ref, 1e-300)))
    rows.append(dict(what='masked scalar', d_hip=s_hip, d_ref=s_ref))
    L.report('module_%dx%dx%d_%s' % (shape[0], shape[2], shape[3], kind), rows)
    assert not bad, bad
    assert s_hip <= MARGIN * s_ref, (s_hip, s_ref)


def test_module_broadcasts_im1_and_takes_spatial_false():
    sd, lins = L.weights()
    shape = (2, 3, 32, 32)
    im0, im1 = L.pair(shape, 'independent')
    net = network()
    got = net(im0.to(DEV), im1[:1].to(DEV))
    want = L.twin(sd, lins, im0, im1[:1].expand(*shape), torch.float64)
    want32 = L.twin(sd, lins, im0, im1[:1].expand(*shape), torch.float32)
    assert L.rel(got.cpu(), want) <= MARGIN * L.rel(want32, want)
    flat = net(im0.to(DEV), im1.to(DEV), spatial=False)
    want = L.twin(sd, lins, im0, im1, torch.float64, spatial=False)
    want32 = L.twin(sd, lins, im0, im1, torch.float32, spatial=False)
    print('spatial=False: hip %.3e float32 twin %.3e' % (L.rel(flat.cpu(), want), L.rel(want32, want)))
    # two float32 numbers: the twin's own error of them can fall below the rounding of the format (9.6e-9 here, a sixth of
    # 2^-24), which no float32 result is held to -- d_ref is at least 2^-24
    assert tuple(flat.shape) == (2, 1, 1, 1) and L.rel(flat.cpu(), want) <= MARGIN * max(L.rel(want32, want), EPS)


@pytest.mark.parametrize('mode', ['lpips', 'mask_lpips', 'pixel'])
def test_edit_distance_on_a_four_image_set(mode):
    """against the reference's loop on the float64 twin (tests/test_lpips_host.py restates it): the LPIPS modes' four values
    within 8 times the float32 twin's own error (2-norm over the set), the pixel mode within the chain bound of masked_l1"""
    from rewriting_amd import distances
    sd, lins = L.weights()
    before, after, seg = L.edit_set()
    src = (1, 2)
    values, counts = distances.edit_distance(before.to(DEV), after.to(DEV), seg.to(DEV), src, mode, network())
    mask = distances.mask_of(seg, src)
    if mode == 'pixel':
        want = ((after.double() - before.double()).abs().sum(1) * mask.double()).sum((1, 2))
        assert torch.equal(counts.cpu().double(), mask.double().sum((1, 2)))
        assert bool(((values.cpu().double() - want).abs() <= (L.CHAIN + 3) * EPS * want).all())
        return
    w = mask[:, None] if mode == 'lpips' else torch.ones(4, 1, 32, 32)
    want = L.twin(sd, lins, before, after, torch.float64, w=w)
    want32 = L.twin(sd, lins, before, after, torch.float32, w=w)
    d_hip, d_ref = L.rel(values.cpu(), want), L.rel(want32, want)
    print('edit_distance %s: d_hip %.3e d_ref %.3e' % (mode, d_hip, d_ref))
    assert torch.equal(counts.cpu(), torch.ones(4)) and d_hip <= MARGIN * d_ref, (d_hip, d_ref)
