"""The input window of the F(4x4,3x3) kernels (rw_wino4.hip, conv_wino36b_body) as it arrives in 16-byte items from
16-byte aligned addresses -- rows y0 - 1 .., columns x0 - 4 .. x0 + 67, three overlapping one-wave pieces per channel --
at the smallest shapes where the loader can go wrong: one weight tap at a time (a window that is off by a row or a column
is an O(1) error in that tap's output, and the outer two rows and columns of the map prove the zero padding), full 3x3
weights, the upsampling mode and ToRGB in the epilogue; on fp32 MFMAs, on the 16-bit pipe and there with the point split.
The reference is float64; the bars are the F(4x4,3x3) test's (test_gpu_kernels.py): 1e-5 relative (Frobenius) and 1e-4
of the output range for a map, and for the image 2e-6 (1e-5 without bias and skip) against ToRGB of the kernel's own map.
(Measured worst cases, MI355X: 1.6e-5 of the range and 2.9e-6 relative for a stride-1 map, 6.9e-6 / 1.5e-6 for the
upsampling map, 1.0e-7 / 1.5e-7 for the images; every case prints its figures.)"""
import functools
import math

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (b, in, out, h, w).  8 x 64: one tile group, all four image edges in one workgroup, two intervals: the ring of three is
# used only partly.  16 x 128: seams between groups in x and y, eight intervals (the ring wraps), the batch stride.
# 8 x 192: in_ch no power of two, a run longer than one group.
CONV_CASES = [(1, 8, 32, 8, 64), (2, 32, 32, 16, 128), (1, 24, 64, 8, 192)]
UP_CASE = (1, 16, 8, 8, 64)
RGB_CASE = (2, 32, 32, 16, 128)
# one non-zero tap (ky, kx) of the 3x3 kernel, all nine, then all taps at once
WEIGHTS = [(ky, kx) for ky in range(3) for kx in range(3)] + ['full']
MODES = ['f32', 'split', 'split-ps']


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """made once per shape and never changed"""
    b, i, o, h, w = case
    rs = numpy.random.RandomState(1801)
    x = torch.from_numpy(rs.randn(b, i, h, w).astype('float32'))
    wt = torch.from_numpy(rs.randn(1, o, i, 3, 3).astype('float32'))
    style = torch.from_numpy((1 + 0.5 * rs.randn(b, i)).astype('float32'))
    return x, wt, style


@functools.lru_cache(maxsize=None)
def _epilogue(case, up):
    b, i, o, h, w = case
    rs = numpy.random.RandomState(1802)
    n = 4 * h * w if up else h * w
    return (torch.from_numpy(rs.randn(b, n).astype('float32')), torch.tensor([0.2]),
            torch.from_numpy(rs.randn(o).astype('float32')))


@functools.lru_cache(maxsize=None)
def _weights(case, which):
    wt = _inputs(case)[1]
    if which == 'full':
        return wt
    one = torch.zeros_like(wt)
    one[..., which[0], which[1]] = wt[..., which[0], which[1]]
    return one


def _act64(v, noise, nw, bias):
    v = v + nw.double() * noise.double().view(v.shape[0], 1, v.shape[2], v.shape[3]) + bias.double().view(1, -1, 1, 1)
    return torch.where(v > 0, v, 0.2 * v) * math.sqrt(2.0)


@functools.lru_cache(maxsize=None)
def _reference(case, which, up):
    """float64: (the demodulated convolution of the styled input, the same through noise, bias and leaky ReLU)"""
    from oracle import restatement as R
    x, _, style = _inputs(case)
    wt = _weights(case, which).double()
    key = (style[:, :, None, None] * x).double()
    conv = R.demod_conv(key, style.double(), wt, upsample=up)
    if up:
        k1 = torch.tensor([1., 3., 3., 1.], dtype=torch.float64)
        k4 = k1[:, None] * k1[None, :]
        conv = R.upfirdn2d(conv, k4 / k4.sum() * 4, pad=(1, 1))
    return conv, _act64(conv, *_epilogue(case, up))


def _mode(monkeypatch, mm):
    if mm != 'f32':
        monkeypatch.setenv('RW_W4H_PS', '1' if mm == 'split-ps' else '0')
    return mm != 'f32'


def _check_map(what, got, ref):
    assert torch.isfinite(got).all()
    scale = ref.abs().max().item()
    linf = (got.cpu().double() - ref).abs().max().item()
    e = rel(got, ref)
    print('wino4 window %s: linf / range %.3g, rel %.3g' % (what, linf / scale, e))
    assert linf < 1e-4 * scale, (what, linf / scale)
    assert e < 1e-5, (what, e)


@pytest.mark.parametrize('mm', MODES)
@pytest.mark.parametrize('which', WEIGHTS, ids=str)
@pytest.mark.parametrize('case', CONV_CASES, ids=str)
def test_stride1_window_single_taps_and_full_weights(case, which, mm, monkeypatch):
    from rewriting_amd import hip
    b, i, o, h, w = case
    split = _mode(monkeypatch, mm)
    x, _, style = _inputs(case)
    wt = _weights(case, which)
    noise, nw, bias = _epilogue(case, False)
    s = 1 / math.sqrt(i * 9)
    dm = hip.demod(hip.weight_sqsum(wt.to(DEV), s), style.to(DEV))
    uf = hip.pack_conv_weight_wino4(wt.to(DEV), split=split)
    plain_ref, act_ref = _reference(case, which, False)
    plain = hip.conv3x3_wino4(x.to(DEV), uf, o, s, style=style.to(DEV), demod=dm)
    _check_map('%s %s %s plain' % (case, which, mm), plain, plain_ref)
    got = hip.conv3x3_wino4(x.to(DEV), uf, o, s, style=style.to(DEV), demod=dm, noise=noise.to(DEV), noise_w=nw.to(DEV),
                            bias=bias.to(DEV), act=True)
    _check_map('%s %s %s epilogue' % (case, which, mm), got, act_ref)


@pytest.mark.parametrize('mm', MODES)
@pytest.mark.parametrize('which', WEIGHTS, ids=str)
def test_upsampling_window_single_taps_and_full_weights(which, mm, monkeypatch):
    from rewriting_amd import hip
    case = UP_CASE
    b, i, o, h, w = case
    assert hip.conv_transpose_blur_wino4_supported(o, i, h, w)
    split = _mode(monkeypatch, mm)
    x, _, style = _inputs(case)
    wt = _weights(case, which)
    noise, nw, bias = _epilogue(case, True)
    s = 1 / math.sqrt(i * 9)
    k1 = torch.tensor([1., 3., 3., 1.])
    k4 = k1[:, None] * k1[None, :]
    k4 = (k4 / k4.sum() * 4).to(DEV)
    dm = hip.demod(hip.weight_sqsum(wt.to(DEV), s), style.to(DEV))
    uf = hip.pack_conv_transpose_blur_weight_wino4(wt.to(DEV), k4, split=split)
    plain_ref, act_ref = _reference(case, which, True)
    plain = hip.conv_transpose3x3s2_blur_wino4(x.to(DEV), uf, o, s, style=style.to(DEV), demod=dm)
    assert plain.shape == (b, o, 2 * h, 2 * w)
    _check_map('up %s %s %s plain' % (case, which, mm), plain, plain_ref)
    got = hip.conv_transpose3x3s2_blur_wino4(x.to(DEV), uf, o, s, style=style.to(DEV), demod=dm,
                                             noise=noise.view(b, 1, 2 * h, 2 * w).to(DEV), noise_w=nw.to(DEV),
                                             bias=bias.to(DEV), act=True)
    _check_map('up %s %s %s epilogue' % (case, which, mm), got, act_ref)


@pytest.mark.parametrize('mm', MODES)
@pytest.mark.parametrize('which', WEIGHTS, ids=str)
def test_to_rgb_window_single_taps_and_full_weights(which, mm, monkeypatch):
    from rewriting_amd import hip
    case = RGB_CASE
    b, i, o, h, w = case
    assert hip.wino4_to_rgb_supported(o, i, h, w)
    split = _mode(monkeypatch, mm)
    x, _, style = _inputs(case)
    wt = _weights(case, which)
    noise, nw, bias = _epilogue(case, False)
    rs = numpy.random.RandomState(1803)
    wrgb = torch.from_numpy(rs.randn(3, o).astype('float32')).to(DEV)
    srgb = torch.from_numpy((1 + 0.3 * rs.randn(b, o)).astype('float32')).to(DEV)
    brgb = torch.from_numpy(rs.randn(3).astype('float32')).to(DEV)
    skip = torch.from_numpy(rs.randn(b, 3, h, w).astype('float32')).to(DEV)
    s = 1 / math.sqrt(i * 9)
    dm = hip.demod(hip.weight_sqsum(wt.to(DEV), s), style.to(DEV))
    uf = hip.pack_conv_weight_wino4(wt.to(DEV), split=split)
    args = dict(style=style.to(DEV), demod=dm, noise=noise.to(DEV), noise_w=nw.to(DEV), bias=bias.to(DEV), act=True)
    # the map this image is made of, held to float64 ...
    fmap = hip.conv3x3_wino4(x.to(DEV), uf, o, s, **args)
    _check_map('rgb %s %s %s map' % (case, which, mm), fmap, _reference(case, which, False)[1])
    # ... and the image to ToRGB of that map
    want = hip.to_rgb(fmap, wrgb, srgb, brgb, skip, 1 / math.sqrt(o))
    y, rgb = hip.conv3x3_wino4_to_rgb(x.to(DEV), uf, o, s, wrgb, srgb, brgb, skip, 1 / math.sqrt(o), **args)
    e = rel(rgb, want)
    _, rgb2 = hip.conv3x3_wino4_to_rgb(x.to(DEV), uf, o, s, wrgb, srgb, None, None, 1 / math.sqrt(o), **args)
    e2 = rel(rgb2, want - skip - brgb.view(1, 3, 1, 1))
    print('wino4 window rgb %s %s %s: image rel %.3g, without bias and skip %.3g' % (case, which, mm, e, e2))
    assert y is None and torch.isfinite(rgb).all()
    assert e < 2e-6, e
    assert e2 < 1e-5, e2
