"""The direct-sum kernels (rw_dconv.hip) with the taps (2, 0) and (2, 1) sharing their Vh Ul instruction, at the smallest
shapes where the pairing can go wrong: one weight tap at a time (a wrong or missing partner of a tap is a relative error
of about 2^-11 in that tap's output, far outside the bars), full 3x3 weights, and the upsampling mode (its composed phase
kernels are 3x3 too).  The bars are the direct kernels' own (test_gpu_kernels.py: max-abs below 2e-5 of the direct fp32
kernel's maximum, relative l2 below 3e-6), the reference is float64 conv2d of the styled input."""
import functools
import math

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (form, (b, in, out, h, w)): one-role = RW_DCONV_V=1; the specialised kernel takes in_ch >= 32, out_ch % 64 == 0, w % 64 == 0
CASES = [('one-role', (1, 16, 32, 16, 32)), ('one-role', (2, 32, 64, 16, 32)),
         ('specialised', (1, 32, 64, 16, 64)), ('specialised', (1, 48, 64, 16, 64)), ('specialised', (3, 32, 64, 16, 128))]
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """x (randn x exp(1.5 randn) per channel), full weights, style -- made once per shape and never changed"""
    b, i, o, h, w = case
    rs = numpy.random.RandomState(901)
    x = torch.from_numpy(rs.randn(b, i, h, w).astype('float32'))
    wt = torch.from_numpy(rs.randn(1, o, i, 3, 3).astype('float32'))
    style = torch.from_numpy((1 + 0.5 * rs.randn(b, i)).astype('float32'))
    x = x * torch.from_numpy(numpy.exp(1.5 * rs.randn(1, i, 1, 1)).astype('float32'))
    return x, wt, style


def _env(monkeypatch, form, case):
    monkeypatch.setenv('RW_DCONV_V', '1' if form == 'one-role' else '2')
    if form == 'specialised' and case[0] == 3:
        monkeypatch.setenv('RW_DCONV_GRID', '5')               # runs of several tiles, across images, ragged


def _check(case, wt):
    from rewriting_amd import hip
    b, i, o, h, w = case
    x, _, style = _inputs(case)
    s = 1 / math.sqrt(i * 9)
    dm = hip.demod(hip.weight_sqsum(wt.to(DEV), s), style.to(DEV))
    pk = hip.pack_conv_weight_direct16(wt.to(DEV))
    got = hip.conv3x3_direct16(x.to(DEV), pk, o, s, style=style.to(DEV), demod=dm)
    direct = hip.conv3x3(x.to(DEV), hip.pack_conv_weight(wt.to(DEV), 0), o, s, style=style.to(DEV), demod=dm, impl=0)
    scale = direct.abs().max().item()
    key = (style[:, :, None, None] * x).double()
    ref = torch.nn.functional.conv2d(key, wt[0].double(), padding=1) * s * dm.cpu().double()[:, :, None, None]
    linf = (got.cpu().double() - ref).abs().max().item()
    e = rel(got, ref)
    print('dconv pairs %s: linf / scale %.3g, rel %.3g' % (case, linf / scale, e))
    assert torch.isfinite(got).all()
    assert linf < 2e-5 * scale, linf / scale
    assert e < 3e-6, e


@pytest.mark.parametrize('tap', TAPS)
@pytest.mark.parametrize('form,case', CASES)
def test_direct16_conv_with_one_weight_tap_matches_float64(form, case, tap, monkeypatch):
    """The weight is non-zero at one tap (ky, kx) only: the output is that tap's three piece products and nothing else."""
    from rewriting_amd import hip
    assert hip.dconv_supported(case[2], case[1], case[3], case[4])
    _env(monkeypatch, form, case)
    full = _inputs(case)[1]
    wt = torch.zeros_like(full)
    wt[..., tap[0], tap[1]] = full[..., tap[0], tap[1]]
    _check(case, wt)


@pytest.mark.parametrize('form,case', CASES)
def test_direct16_conv_with_full_weights_matches_float64(form, case, monkeypatch):
    _env(monkeypatch, form, case)
    _check(case, _inputs(case)[1])


@pytest.mark.parametrize('ver', ['one-role', 'specialised'])
def test_direct16_upsampling_conv_matches_conv_then_blur(ver, monkeypatch):
    """The upsampling mode (four output-parity phases, each a 3x3 direct sum) against the two-pass route of the same library
    (direct transposed convolution, then blur + noise + bias + leaky ReLU), as test_gpu_kernels.py's UP_DIRECT16_CASES."""
    from rewriting_amd import hip
    case = (2, 16, 16, 8, 32)
    b, i, o, h, w = case
    assert hip.dconv_transpose_blur_supported(o, i, h, w)
    monkeypatch.setenv('RW_DCONV_V', '1' if ver == 'one-role' else '2')
    monkeypatch.setenv('RW_DCONV_GRID', '7')
    rs = numpy.random.RandomState(902)
    x = torch.from_numpy(rs.randn(b, i, h, w).astype('float32'))
    wt = torch.from_numpy(rs.randn(1, o, i, 3, 3).astype('float32'))
    style = torch.from_numpy((1 + 0.5 * rs.randn(b, i)).astype('float32'))
    x = x * torch.from_numpy(numpy.exp(1.0 * rs.randn(1, i, 1, 1)).astype('float32'))
    s = 1 / math.sqrt(i * 9)
    k1 = torch.tensor([1., 3., 3., 1.])
    k4 = k1[:, None] * k1[None, :]
    k4 = (k4 / k4.sum() * 4).to(DEV)
    noise = torch.from_numpy(rs.randn(b, 1, 2 * h, 2 * w).astype('float32')).to(DEV)
    nw = torch.tensor([0.37], device=DEV)
    bias = torch.from_numpy(rs.randn(o).astype('float32')).to(DEV)
    dm = hip.demod(hip.weight_sqsum(wt.to(DEV), s), style.to(DEV))
    wide = hip.conv_transpose3x3s2(x.to(DEV), hip.pack_conv_weight(wt.to(DEV), 1), o, s, style=style.to(DEV), demod=dm,
                                   impl=0 if i % 16 == 0 and o % 32 == 0 else 1)
    pk = hip.pack_conv_transpose_blur_weight_direct16(wt.to(DEV), k4)
    for kw in (dict(noise=noise, noise_w=nw, bias=bias, act=True), dict()):
        want = hip.blur_noise_act(wide, k4, kw.get('noise'), kw.get('noise_w'), kw.get('bias'), None)
        got = hip.conv_transpose3x3s2_blur_direct16(x.to(DEV), pk, o, s, style=style.to(DEV), demod=dm, **kw)
        assert got.shape == want.shape == (b, o, 2 * h, 2 * w)
        scale = want.abs().max().item()
        linf = (got - want).abs().max().item()
        print('dconv pairs up %s: linf / scale %.3g, rel %.3g' % (sorted(kw), linf / scale, rel(got, want)))
        assert linf < 2e-5 * scale, linf / scale
        assert rel(got, want) < 3e-6, rel(got, want)
