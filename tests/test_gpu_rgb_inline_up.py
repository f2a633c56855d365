"""The running RGB image upsampled inside its consumers (hip.HalfSkip: rw_rgb_combine_up_f32 and the F(4x4) ToRGB epilogues,
rw_up2k4_row4 in csrc/rw_common.h) against the same consumers fed the image that the existing upsampling op materialises
(Upsample: upfirdn2d up 2, pads 2 / 1, upfirdn2d_up2k4_kernel).  The two must agree bit for bit -- same taps in the same
order, added at the same place of the sum -- so every comparison is torch.equal, at the smallest shapes the kernels take:
every tile of them touches a border of the image.  Two FIRs: the generator's, and one that is no outer product and not
symmetric, so that a transposed, unflipped or row/column-swapped tap shows."""
import functools
import math

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FIRS = ['generator', 'skew']


@functools.lru_cache(maxsize=None)
def _fir(which):
    if which == 'generator':
        k1 = torch.tensor([1., 3., 3., 1.])
        k = k1[:, None] * k1[None, :]
    else:
        rs = numpy.random.RandomState(2101)
        k = torch.tensor([1., 2., 3., 4.])[:, None] * torch.tensor([1., 3., 5., 7.])[None, :]
        k = k + torch.from_numpy(rs.uniform(0.1, 0.9, (4, 4)).astype('float32'))
    return (k / k.sum() * 4).contiguous()


def _upsampled(half, fir):
    from rewriting_amd.utils.stylegan2 import op
    return op.upfirdn2d(half, fir, up=2, down=1, pad=(2, 1))


@pytest.mark.parametrize('which', FIRS)
@pytest.mark.parametrize('size', [(8, 8), (8, 16), (12, 20), (64, 64)], ids=str)
@pytest.mark.parametrize('n_part', [1, 2, 4])
def test_rgb_combine_half_size_skip_equals_materialised_skip(n_part, size, which):
    from rewriting_amd import hip
    h, w = size
    rs = numpy.random.RandomState(2102)
    part = torch.from_numpy(rs.randn(n_part, 2, 3, h, w).astype('float32')).to(DEV)
    bias = torch.from_numpy(rs.randn(3).astype('float32')).to(DEV)
    half = torch.from_numpy(rs.randn(2, 3, h // 2, w // 2).astype('float32')).to(DEV)
    fir = _fir(which).to(DEV)
    full = _upsampled(half, fir)
    assert tuple(full.shape) == (2, 3, h, w)
    for b in (bias, None):
        want = hip.rgb_combine(part, b, full)
        got = hip.rgb_combine(part, b, hip.HalfSkip(half, fir))
        assert torch.equal(got, want), (n_part, size, which, b is not None, (got - want).abs().max().item())
    # the upsampled term alone: zero partial sums, no bias
    got = hip.rgb_combine(torch.zeros_like(part), None, hip.HalfSkip(half, fir))
    assert torch.equal(got, full + 0.0)


def test_half_size_skip_shapes_are_checked():
    from rewriting_amd import hip
    part = torch.zeros(1, 2, 3, 8, 8, device=DEV)
    fir = _fir('generator').to(DEV)
    with pytest.raises(ValueError):
        hip.rgb_combine(part, None, hip.HalfSkip(torch.zeros(2, 3, 8, 8, device=DEV), fir))
    with pytest.raises(ValueError):
        hip.rgb_combine(part, None, hip.HalfSkip(torch.zeros(2, 3, 4, 4, device=DEV), fir[:3]))


@functools.lru_cache(maxsize=None)
def _conv_inputs(case):
    b, i, o, h, w = case
    rs = numpy.random.RandomState(2103)
    f = lambda *shape: torch.from_numpy(rs.randn(*shape).astype('float32'))
    return dict(x=f(b, i, h, w), wt=f(1, o, i, 3, 3), style=1 + 0.5 * f(b, i), noise=f(b, h * w), bias=f(o),
                wrgb=f(3, o), srgb=1 + 0.3 * f(b, o), brgb=f(3), half=f(b, 3, h // 2, w // 2))


@pytest.mark.parametrize('which', FIRS)
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('mm', ['f32', 'split', 'split-ps'])
@pytest.mark.parametrize('case', [(2, 8, 32, 8, 64), (2, 32, 32, 8, 64), (2, 8, 32, 16, 128), (2, 32, 32, 16, 128)], ids=str)
def test_final_wino4_to_rgb_half_size_skip_equals_materialised_skip(case, mm, with_bias, which, monkeypatch):
    from rewriting_amd import hip
    b, i, o, h, w = case
    assert hip.wino4_to_rgb_supported(o, i, h, w)
    if mm != 'f32':
        monkeypatch.setenv('RW_W4H_PS', '1' if mm == 'split-ps' else '0')
    t = {k: v.to(DEV) for k, v in _conv_inputs(case).items()}
    fir = _fir(which).to(DEV)
    s = 1 / math.sqrt(i * 9)
    dm = hip.demod(hip.weight_sqsum(t['wt'], s), t['style'])
    uf = hip.pack_conv_weight_wino4(t['wt'], split=mm != 'f32')
    args = dict(style=t['style'], demod=dm, noise=t['noise'], noise_w=torch.tensor([0.2], device=DEV), bias=t['bias'], act=True)
    brgb = t['brgb'] if with_bias else None
    full = _upsampled(t['half'], fir)
    _, want = hip.conv3x3_wino4_to_rgb(t['x'], uf, o, s, t['wrgb'], t['srgb'], brgb, full, 1 / math.sqrt(o), **args)
    y, got = hip.conv3x3_wino4_to_rgb(t['x'], uf, o, s, t['wrgb'], t['srgb'], brgb, hip.HalfSkip(t['half'], fir),
                                      1 / math.sqrt(o), **args)
    assert y is None and torch.isfinite(want).all()
    assert torch.equal(got, want), (case, mm, with_bias, which, (got - want).abs().max().item())
    # the skip matters: without one the image differs
    _, bare = hip.conv3x3_wino4_to_rgb(t['x'], uf, o, s, t['wrgb'], t['srgb'], brgb, None, 1 / math.sqrt(o), **args)
    assert not torch.equal(bare, want)


def test_generator_image_is_the_same_with_the_switch_off(monkeypatch):
    """A 128^2 generator: to_rgb at 64^2 and at 128^2 are two chained rgb_combine launches, each with the image one level
    down as its skip.  The switch on must really take that path, off must not, and the images must be equal."""
    from rewriting_amd import hip
    from tests.conftest import build_stylegan
    for name in ('RW_RGB_INLINE_UP', 'RW_RGB_PARTIAL', 'RW_RGB_STREAM', 'RW_FUSE', 'RW_MICRO_BATCH'):
        monkeypatch.delenv(name, raising=False)
    g = build_stylegan(128, 0.7, device=DEV)
    z = torch.randn(2, 512, generator=torch.Generator().manual_seed(11)).to(DEV)
    seen = []
    combine = hip.rgb_combine
    monkeypatch.setattr(hip, 'rgb_combine', lambda p, b, s: (seen.append(type(s).__name__), combine(p, b, s))[1])
    with torch.no_grad():
        on = g(z)
        halves, seen[:] = seen.count('HalfSkip'), []
        monkeypatch.setenv('RW_RGB_INLINE_UP', '0')
        off = g(z)
    torch.cuda.synchronize()
    assert halves >= 2 and seen and 'HalfSkip' not in seen, (halves, seen)
    assert tuple(on.shape) == (2, 3, 128, 128) and torch.isfinite(on).all()
    assert torch.equal(on, off), (on - off).abs().max().item()
    # a forward hook of torch's on any step may look into the bags: it sees the running image as a tensor, as before
    monkeypatch.delenv('RW_RGB_INLINE_UP')
    outputs = []
    handle = g.up_rgb3.register_forward_hook(lambda m, i, o: outputs.append(o['output']))
    seen[:] = []
    with torch.no_grad():
        hooked = g(z)
    handle.remove()
    assert torch.is_tensor(outputs[0]) and tuple(outputs[0].shape) == (2, 3, 32, 32) and 'HalfSkip' not in seen
    assert torch.equal(hooked, on)
