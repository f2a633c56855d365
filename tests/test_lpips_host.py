"""rewriting_amd/lpips.py and rewriting_amd/distances.py on the host: the up-sampling tables against F.interpolate in float64,
the state dicts, every refusal, the broadcasting of im1 and w, the module on the emulated kernels against the float32 twin
(tests/lpips_checks.py), edit_distance against the reference's loop restated here, the condition on the reference of the
device test, and the entries of the C ABI."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import _lib, distances, hip, lpips, perceptual
from tests import lpips_checks as L

MARGIN = 8                          # d <= MARGIN * d_ref (DESIGN section 8.1's margin)
ENTRIES = ('rw_lpips_tap_f32', 'rw_lpips_reduce_scratch_elems', 'rw_lpips_combine_f32', 'rw_masked_l1_rgb_f32')


@pytest.fixture
def emulated(emulated_hip, monkeypatch):
    log = []
    L.install(monkeypatch, log)
    return log


@pytest.fixture(scope='module')
def net():
    sd, lins = L.weights()
    return lpips.from_state_dicts(sd, lins)


@pytest.mark.parametrize('n_in,n_out', [(1, 16), (2, 20), (3, 28), (5, 20), (7, 28), (16, 32), (64, 1024)])
def test_upsample_table_is_interpolate_in_float64(n_in, n_out):
    i0, i1, lam = lpips.upsample_table(n_in, n_out)
    assert i0.shape == i1.shape == lam.shape == (n_out,) and lam.dtype.name == 'float64'
    assert i0.min() >= 0 and i1.min() >= 0 and i0.max() <= n_in - 1 and i1.max() <= n_in - 1
    assert (lam >= 0).all() and (lam < 1).all()
    eye = torch.eye(n_in, dtype=torch.float64)
    got = torch.zeros(n_out, n_in, dtype=torch.float64)
    rows = torch.arange(n_out)
    got.index_put_((rows, torch.from_numpy(i0.copy()).long()), 1 - torch.from_numpy(lam.copy()), accumulate=True)
    got.index_put_((rows, torch.from_numpy(i1.copy()).long()), torch.from_numpy(lam.copy()), accumulate=True)
    # channel c of the input is column c of the identity along H: out[0, c, o, 0] = M[o, c]
    want = F.interpolate(eye.view(1, n_in, n_in, 1), size=(n_out, 1), mode='bilinear', align_corners=False)[0, :, :, 0].t()
    assert (got - want).abs().max().item() <= 1e-12
    idx, lam32 = lpips.device_tables(((n_in, n_in),), (n_out, n_out), 'cpu')
    assert tuple(idx.shape) == (1, 4 * n_out) and tuple(lam32.shape) == (1, 2 * n_out) and lam32.dtype == torch.float32
    assert torch.equal(idx[0, :n_out], idx[0, 2 * n_out:3 * n_out]) and torch.equal(idx[0, n_out:2 * n_out], idx[0, 3 * n_out:])
    with pytest.raises(ValueError, match='positive'):
        lpips.upsample_table(0, 4)


def test_state_dicts_bare_prefixed_and_from_files(tmp_path, monkeypatch):
    sd, lins = L.weights()
    net = lpips.from_state_dicts(sd, lins)
    assert [(i, b.in_ch, b.out_ch, b.pool) for i, b in net.blocks()] == [tuple(row) for row in L.ALL_LAYERS]
    assert isinstance(net.features, perceptual.VGG16Features) and not any(p.requires_grad for p in net.parameters())
    for index, block in net.blocks():
        assert torch.equal(block.weight, sd['%d.weight' % index]) and torch.equal(block.bias, sd['%d.bias' % index])
    for p, want in zip(net.lins, L.lin_list(lins)):
        assert torch.equal(p, want)
    whole = {'features.' + k: v for k, v in sd.items()}
    whole['classifier.0.weight'] = torch.zeros(4, 4)
    bare_lins = {'lin%d' % k: v for k, v in enumerate(L.lin_list(lins))}
    other = lpips.from_state_dicts(whole, bare_lins)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), net.state_dict().values()))
    # perceptual's own loader is as before: the layers past 20 are ignored there
    assert sorted(perceptual.from_state_dict(whole).state_dict()) == sorted(perceptual.from_state_dict(P_head(sd)).state_dict())
    vgg_path, lin_path = tmp_path / 'vgg16.pth', tmp_path / 'lin.pth'
    torch.save(whole, str(vgg_path))
    torch.save(lins, str(lin_path))
    loaded = lpips.lpips_vgg(str(vgg_path), str(lin_path))
    assert all(torch.equal(a, b) and a.device.type == 'cpu' for a, b in zip(loaded.state_dict().values(), net.state_dict().values()))
    monkeypatch.delenv(perceptual.WEIGHTS_ENV, raising=False)
    monkeypatch.delenv(lpips.WEIGHTS_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match='RW_VGG16_WEIGHTS.*RW_LPIPS_WEIGHTS'):
        lpips.lpips_vgg()
    monkeypatch.setenv(perceptual.WEIGHTS_ENV, str(vgg_path))
    with pytest.raises(FileNotFoundError, match='RW_LPIPS_WEIGHTS'):
        lpips.lpips_vgg()
    monkeypatch.setenv(lpips.WEIGHTS_ENV, str(lin_path))
    assert torch.equal(lpips.lpips_vgg().lins[4], net.lins[4])
    with pytest.raises(KeyError, match='lacks 28.bias'):
        lpips.from_state_dicts({k: v for k, v in sd.items() if k != '28.bias'}, lins)
    with pytest.raises(KeyError, match='lacks 19.bias'):
        lpips.from_state_dicts({k: v for k, v in sd.items() if k != '19.bias'}, lins)
    with pytest.raises(ValueError, match='24.weight'):
        lpips.from_state_dicts(dict(sd, **{'24.weight': torch.zeros(512, 256, 3, 3)}), lins)
    with pytest.raises(KeyError, match='30.weight'):
        lpips.from_state_dicts(dict(sd, **{'30.weight': torch.zeros(1)}), lins)
    with pytest.raises(KeyError, match='lin3'):
        lpips.from_state_dicts(sd, {k: v for k, v in lins.items() if not k.startswith('lin3')})
    with pytest.raises(ValueError, match='lin1'):
        lpips.from_state_dicts(sd, dict(lins, **{'lin1.model.1.weight': torch.zeros(1, 64, 1, 1)}))
    with pytest.raises(TypeError, match='VGG16Features'):
        lpips.LPIPS(torch.nn.Identity())


def P_head(sd):
    return {k: v for k, v in sd.items() if int(k.split('.')[0]) <= perceptual.LAST_LAYER}


def test_every_refusal(emulated, net, monkeypatch):
    im = torch.zeros(2, 3, 16, 16)
    net(im, im)
    with pytest.raises(RuntimeError, match='fp32 only'):
        net(im.double(), im)
    with pytest.raises(RuntimeError, match='fp32 only'):
        net(im, im.half())
    with pytest.raises(RuntimeError, match='fp32 only'):
        net(im, im, w=torch.ones(2, 1, 16, 16, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='forward only'):
        net(im.clone().requires_grad_(True), im)
    with torch.no_grad():
        net(im.clone().requires_grad_(True), im)
    with pytest.raises(ValueError, match=r'\(B, 3, H, W\)'):
        net(im[:, :2], im)
    with pytest.raises(ValueError, match='sizes must match'):
        net(im, torch.zeros(2, 3, 16, 20))
    with pytest.raises(ValueError, match='sizes must match'):
        net(im, torch.zeros(3, 3, 16, 16))
    for bad in (torch.ones(2, 16, 16), torch.ones(2, 3, 16, 16), torch.ones(3, 1, 16, 16), torch.ones(2, 1, 16, 8)):
        with pytest.raises(ValueError, match=r'\(B or 1, 1, H, W\)'):
            net(im, im, w=bad)
    with pytest.raises(ValueError, match='at least 16 x 16'):
        net(im[:, :, :15], im[:, :, :15])
    net.lins[2].requires_grad_(True)
    try:
        with pytest.raises(RuntimeError, match='lins.2 requires a gradient'):
            net(im, im)
    finally:
        net.lins[2].requires_grad_(False)
    monkeypatch.setattr(hip, 'on_device', lambda t: bool(t.is_cuda))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(im, im)


def test_the_wrappers_refuse_before_any_call(monkeypatch):
    def no_call():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(hip, 'lib', no_call)
    f, lin, d = torch.zeros(2, 4, 3, 3), torch.zeros(4), torch.zeros(2, 3, 3)
    tables = lpips.device_tables(((3, 3),), (6, 6), 'cpu')
    rgb, m = torch.zeros(2, 3, 4, 4), torch.ones(2, 4, 4)
    for call in (lambda: hip.lpips_tap(f, f, lin), lambda: hip.lpips_combine([d], tables, (6, 6)), lambda: hip.masked_l1(rgb, rgb, m)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))      # past the device check, on the host
    for call in (lambda: hip.lpips_tap(f.double(), f, lin), lambda: hip.lpips_tap(f, f, lin.half()),
                 lambda: hip.lpips_combine([d.double()], tables, (6, 6)), lambda: hip.masked_l1(rgb, rgb.double(), m),
                 lambda: hip.masked_l1(rgb, rgb, m.long())):
        with pytest.raises(RuntimeError, match='fp32 only'):
            call()
    with pytest.raises(RuntimeError, match='contiguous'):
        hip.lpips_tap(f.transpose(2, 3), f, lin)
    for call in (lambda: hip.lpips_tap(f, torch.zeros(2, 3, 3, 3), lin), lambda: hip.lpips_tap(f, torch.zeros(3, 4, 3, 3), lin),
                 lambda: hip.lpips_tap(f, f, torch.zeros(5)), lambda: hip.lpips_tap(f[0], f[0], lin),
                 lambda: hip.lpips_combine([], tables, (6, 6)), lambda: hip.lpips_combine([d] * 9, tables, (6, 6)),
                 lambda: hip.lpips_combine([d], tables, (6, 6), want_map=False),
                 lambda: hip.lpips_combine([d], tables, (6, 7)), lambda: hip.lpips_combine([d, d], tables, (6, 6)),
                 lambda: hip.lpips_combine([d], tables, (6, 6), weight=torch.ones(3, 1, 6, 6)),
                 lambda: hip.masked_l1(rgb, rgb[:1], m), lambda: hip.masked_l1(f, f, m), lambda: hip.masked_l1(rgb, rgb, torch.ones(2, 3, 4))):
        with pytest.raises(ValueError):
            call()


def test_im1_and_w_broadcast(emulated, net):
    im0, im1 = L.pair((2, 3, 32, 32), 'independent')
    w = L.mask((2, 3, 32, 32))
    whole = net(im0, im1[:1].expand(2, 3, 32, 32).contiguous(), w=w[:1].expand(2, 1, 32, 32).contiguous())
    del emulated[:]
    got = net(im0, im1[:1], w=w[:1])
    # (the host's convolutions round differently at batch 1 and batch 2: to rounding, not to the bit)
    assert tuple(got.shape) == (2,) and L.rel(got, whole) < 1e-6
    # im1's network ran once: every convolution saw batch 2 and batch 1
    batches = [args[0].shape[0] for name, args, _ in emulated if name == 'conv3x3_rgb']
    assert batches == [2, 1]
    taps = [(args[0].shape[0], args[1].shape[0]) for name, args, _ in emulated if name == 'lpips_tap']
    assert taps == [(2, 1)] * 5
    combine = [kw for name, _, kw in emulated if name == 'lpips_combine']
    assert len(combine) == 1 and combine[0]['want_map'] is False and combine[0]['want_sums'] is True     # the map is never written


@pytest.mark.parametrize('shape', L.SHAPES)
def test_the_module_on_the_emulation_is_the_float32_twin(emulated, net, shape):
    sd, lins = L.weights()
    im0, im1 = L.pair(shape, 'box')
    ref, ref32 = L.reference(shape, 'box')[torch.float64], L.reference(shape, 'box')[torch.float32]
    taps = []
    got = net(im0, im1, taps=taps)
    b, _, h, w = shape
    assert tuple(got.shape) == (b, 1, h, w)
    assert [tuple(d.shape) for d in taps] == [(b, h >> k, w >> k) for k in range(5)]
    # the emulated kernels are the float32 arithmetic in another order (the F(2x2,3x3) transforms included): the device test's bar
    assert L.rel(got, ref[0]) <= MARGIN * L.rel(ref32[0], ref[0])
    for d, want, want32 in zip(taps, ref[1], ref32[1]):
        assert L.rel(d[:, None], want) <= MARGIN * L.rel(want32, want)
    scalar = net(im0, im1, w=L.mask(shape))
    assert tuple(scalar.shape) == (b,) and L.rel(scalar, ref[2]) <= MARGIN * L.rel(ref32[0], ref[0])
    flat = net(im0, im1, spatial=False)
    want = L.twin(sd, lins, im0, im1, torch.float64, spatial=False)
    assert tuple(flat.shape) == (b, 1, 1, 1) and L.rel(flat, want) <= MARGIN * L.rel(ref32[0], ref[0])
    flat_w = net(im0, im1, w=L.mask(shape), spatial=False)
    assert tuple(flat_w.shape) == (b,) and L.rel(flat_w, want.view(b)) <= MARGIN * L.rel(ref32[0], ref[0])
    assert not got.requires_grad


def test_the_reference_alone_meets_its_condition():
    """the float32 twin against the float64 twin, on the device test's inputs: < 2e-5 on the spatial map, < 5e-5 per tap"""
    worst_map = worst_tap = 0.0
    for shape in L.SHAPES:
        for kind in L.KINDS:
            ref = L.reference(shape, kind)
            d_map = L.rel(ref[torch.float32][0], ref[torch.float64][0])
            d_taps = [L.rel(a, b) for a, b in zip(ref[torch.float32][1], ref[torch.float64][1])]
            print('%s %s: d_ref map %.3e taps %s' % (shape, kind, d_map, ' '.join('%.3e' % d for d in d_taps)))
            worst_map, worst_tap = max(worst_map, d_map), max([worst_tap] + d_taps)
    assert worst_map < 2e-5 and worst_tap < 5e-5, (worst_map, worst_tap)


def reference_loop(before, after, seg, src, mode, sd, lins):
    """metrics/distances.py:101-133 restated on the float64 twin: image by image for the two LPIPS modes"""
    masks = torch.ones_like(seg)
    for index in src:
        masks = masks * (seg != index).long()
    total, count = 0.0, 0
    if mode in ('lpips', 'mask_lpips'):
        for b, a, m in zip(before, after, masks):
            b, a, m = b.unsqueeze(0), a.unsqueeze(0), m.unsqueeze(0).unsqueeze(0)
            total += L.twin(sd, lins, b, a, torch.float64, w=m if mode == 'lpips' else torch.ones_like(m)).item()
            count += 1
    else:
        differences = (after.double() - before.double()).abs().sum(dim=1)
        total += (differences * masks).sum().item()
        count += masks.long().sum().item()
    return total, count


@pytest.mark.parametrize('mode', distances.MODES)
def test_edit_distance_against_the_reference_loop(emulated, net, mode):
    sd, lins = L.weights()
    before, after, seg = L.edit_set()
    values, counts = distances.edit_distance(before, after, seg, (1, 2), mode, net)
    want_total, want_count = reference_loop(before, after, seg, (1, 2), mode, sd, lins)
    assert tuple(values.shape) == tuple(counts.shape) == (4,)
    assert counts.sum().item() == want_count
    assert abs(values.double().sum().item() - want_total) <= 2e-5 * want_total
    if mode == 'pixel':
        unmasked, n = distances.edit_distance(before, after, None, (), mode)
        assert n.sum().item() == 4 * 32 * 32 and unmasked.sum().item() > values.sum().item()
    else:
        with pytest.raises(ValueError, match='needs net'):
            distances.edit_distance(before, after, seg, (1, 2), mode)
    with pytest.raises(ValueError, match='mode is one of'):
        distances.edit_distance(before, after, seg, (1, 2), 'l2', net)
    with pytest.raises(ValueError, match=r'\(B, H, W\)'):
        distances.edit_distance(before, after, seg[:2], (1, 2), mode, net)


def test_compute_dl_over_png_directories(emulated, net, tmp_path, monkeypatch):
    import numpy
    import PIL.Image
    sd, lins = L.weights()
    before, after, seg = L.edit_set()
    dirs = {}
    for name, images in (('before', before), ('after', after)):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        for k, im in enumerate(images):
            data = ((im.permute(1, 2, 0) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
            PIL.Image.fromarray(numpy.ascontiguousarray(data)).save(str(dirs[name] / ('%d.png' % k)))
    dirs['seg'] = tmp_path / 'seg'
    dirs['seg'].mkdir()
    for k in range(4):
        torch.save(torch.stack([torch.zeros_like(seg[k]), seg[k]]), str(dirs['seg'] / ('%d.pth' % k)))
    quant = lambda x: (((x + 1) * 127.5).round().clamp(0, 255) / 255 - 0.5) / 0.5
    for mode in distances.MODES:
        total, count = distances.compute_dl(str(dirs['before']), str(dirs['after']), str(dirs['seg']), [0, 1, 3], src=(1, 2), srcc=1,
                                            mode=mode, batch_size=2, net=net, device='cpu')
        pick = torch.tensor([0, 1, 3])
        want_total, want_count = reference_loop(quant(before)[pick], quant(after)[pick], seg[pick], (1, 2), mode, sd, lins)
        assert count == want_count and abs(total - want_total) <= 2e-5 * want_total, (mode, total, want_total)


def test_the_entries_are_bound_and_exported():
    assert _lib.ABI_VERSION == 11 and hip.LPIPS_MAX_TAPS == 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.LpipsMaps) == 8 * 8 + 8 * 4 + 8 * 4 + 4 + 4       # 8 pointers, 2 x 8 ints, n, padding
    scratch = _lib.load().rw_lpips_reduce_scratch_elems
    assert scratch(1, 1) == 2 and scratch(2, 1024 * 1024) == 2 * 2 * 4096 and scratch(1, 1024 * 1024 + 1) == 2 * 2049
    assert scratch(0, 4) == -1 and scratch(1, 0) == -1 and scratch(1, 256 * 28 * 4096 + 1) == -1
    assert scratch(1, 256 * 28 * 4096) == 2 * 4096
