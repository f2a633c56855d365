"""The float64 forward on the device: every _f64 kernel against torch in double on the host, a .double() generator
against oracle/restatement.py stage by stage, the double image as the oracle of the fp32 one, and the refusals.

Bar of every double comparison (tests/f64_common.py): max |got - want| <= 1e-9 max(1, max |want|), both sides on the same
double inputs.
"""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import hip, synthetic
from rewriting_amd.utils import nethook, zdataset
from rewriting_amd.utils.stylegan2 import models
from tests import f64_common as f64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0) if torch.cuda.is_available() else None
D = torch.float64


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=D)


def uni(gen, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=gen, dtype=D)


def close(got, want, what=''):
    err = f64.assert_close(got, want, what)
    print('%s: %.3e' % (what, err))


# ---------------------------------------------------------------------------------------------- 1. per kernel
STRIDE1 = [(2, 16, 16, 4, 4),       # one MFMA tile
           (1, 24, 40, 5, 7),       # the one-thread-per-output kernel, odd sizes
           (1, 64, 32, 33, 17),     # edges inside MFMA tiles, several tiles
           (1, 512, 512, 8, 8),     # the deepest K
           (3, 4, 16, 16, 16)]      # the smallest MFMA K step
TRANSPOSED = [(2, 16, 16, 4, 4), (1, 32, 16, 5, 3), (1, 64, 64, 16, 16),
              (1, 20, 12, 3, 6)]    # the one-thread-per-output kernel


def _conv_case(shape, seed):
    b, cin, cout, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    return (rnd(gen, b, cin, h, w), rnd(gen, cout, cin, 3, 3), uni(gen, 0.5, 1.5, b, cin), uni(gen, 0.5, 2.0, b, cout),
            1 / math.sqrt(9 * cin))


@pytest.mark.parametrize('shape', STRIDE1, ids=lambda s: '%dx%d-%d_%dx%d' % s)
def test_conv3x3_f64(shape):
    x, wt, style, demod, scale = _conv_case(shape, 11)
    for with_style, with_demod in itertools.product((False, True), repeat=2):
        xs = x * style[:, :, None, None] if with_style else x
        want = F.conv2d(xs, scale * wt, padding=1)
        if with_demod:
            want = want * demod[:, :, None, None]
        got = hip.conv3x3_f64(x.to(DEV), wt.to(DEV), scale, style=style.to(DEV) if with_style else None,
                              demod=demod.to(DEV) if with_demod else None)
        close(got, want, 'conv3x3_f64 %s style=%s demod=%s' % (shape, with_style, with_demod))


@pytest.mark.parametrize('shape', TRANSPOSED, ids=lambda s: '%dx%d-%d_%dx%d' % s)
def test_conv_transpose3x3s2_f64(shape):
    x, wt, style, demod, scale = _conv_case(shape, 12)
    b, cin, cout, h, w = shape
    for with_style, with_demod in itertools.product((False, True), repeat=2):
        xs = x * style[:, :, None, None] if with_style else x
        want = F.conv_transpose2d(xs, scale * wt.transpose(0, 1), stride=2)
        if with_demod:
            want = want * demod[:, :, None, None]
        assert tuple(want.shape) == (b, cout, 2 * h + 1, 2 * w + 1)
        got = hip.conv_transpose3x3s2_f64(x.to(DEV), wt.to(DEV), scale, style=style.to(DEV) if with_style else None,
                                          demod=demod.to(DEV) if with_demod else None)
        close(got, want, 'conv_transpose3x3s2_f64 %s style=%s demod=%s' % (shape, with_style, with_demod))
        # output row 2H and column 2W, which only the last input row / column reach
        close(got[:, :, -1], want[:, :, -1], 'row 2H')
        close(got[:, :, :, -1], want[:, :, :, -1], 'column 2W')


@pytest.mark.parametrize('c,h,w', [(32, 4, 4), (32, 33, 17), (512, 4, 4), (512, 33, 17)])
def test_to_rgb_f64(c, h, w):
    gen = torch.Generator().manual_seed(13)
    b = 2
    x, wt, style = rnd(gen, b, c, h, w), rnd(gen, 3, c), uni(gen, 0.5, 1.5, b, c)
    bias, skip = rnd(gen, 3), rnd(gen, b, 3, h, w)
    scale = 1 / math.sqrt(c)
    for with_bias, with_skip in itertools.product((False, True), repeat=2):
        want = torch.einsum('bci,bihw->bchw', scale * wt[None] * style[:, None, :], x)
        if with_bias:
            want = want + bias.view(1, 3, 1, 1)
        if with_skip:
            want = want + skip
        got = hip.to_rgb_f64(x.to(DEV), wt.to(DEV), style.to(DEV), bias.to(DEV) if with_bias else None,
                             skip.to(DEV) if with_skip else None, scale)
        close(got, want, 'to_rgb_f64 C=%d hw=%d bias=%s skip=%s' % (c, h * w, with_bias, with_skip))


@pytest.mark.parametrize('out_dim', [512, 32])
def test_equal_linear_f64(out_dim):
    gen = torch.Generator().manual_seed(14)
    b, n_latent = 5, 8
    latent = rnd(gen, b, n_latent, 512)
    wt, bias = rnd(gen, out_dim, 512) / 0.01, rnd(gen, out_dim)
    scale, lr_mul = 0.01 / math.sqrt(512), 0.01
    lat_dev = latent.to(DEV)
    for act in (False, True):
        for view_h, view_d in ((latent[:, 3], lat_dev[:, 3]), (latent[:, 0].contiguous(), lat_dev[:, 0].contiguous())):
            want = F.linear(view_h, wt * scale) + bias * lr_mul
            if act:
                want = F.leaky_relu(want, 0.2) * 2 ** 0.5
            got = hip.equal_linear_f64(view_d, wt.to(DEV), bias.to(DEV), scale, lr_mul, act=act)
            close(got, want, 'equal_linear_f64 512->%d act=%s stride=%d' % (out_dim, act, view_d.stride(0)))
    got = hip.equal_linear_f64(lat_dev[:, 3], wt.to(DEV), None, scale, lr_mul)
    close(got, F.linear(latent[:, 3], wt * scale), 'equal_linear_f64 without bias')


def test_pixel_norm_adjust_latent_style_mul_noise_add_f64():
    gen = torch.Generator().manual_seed(15)
    z = rnd(gen, 5, 512)
    close(hip.pixel_norm_f64(z.to(DEV)), z * torch.rsqrt(torch.mean(z ** 2, dim=1, keepdim=True) + 1e-8), 'pixel_norm_f64')
    avg = rnd(gen, 512)
    close(hip.adjust_latent_f64(z.to(DEV), avg.to(DEV), 6, 0.5), (avg + 0.5 * (z - avg)).unsqueeze(1).repeat(1, 6, 1),
          'adjust_latent_f64 with avg')
    close(hip.adjust_latent_f64(z.to(DEV), None, 6, 0.5), z.unsqueeze(1).repeat(1, 6, 1), 'adjust_latent_f64 without avg')
    for b, c, h, w in ((2, 24, 5, 7), (3, 16, 8, 8)):
        x, style, noise, nw = rnd(gen, b, c, h, w), uni(gen, 0.5, 1.5, b, c), rnd(gen, b, h * w), rnd(gen, 1)
        close(hip.style_mul_f64(x.to(DEV), style.to(DEV)), style[:, :, None, None] * x, 'style_mul_f64')
        close(hip.noise_add_f64(x.to(DEV), noise.to(DEV), nw.to(DEV)), x + nw * noise.view(b, 1, h, w), 'noise_add_f64')


@pytest.mark.parametrize('b,cin,cout', [(2, 24, 40), (3, 512, 512)])
def test_weight_sqsum_and_demod_f64(b, cin, cout):
    gen = torch.Generator().manual_seed(16)
    wt, style = rnd(gen, 1, cout, cin, 3, 3), uni(gen, 0.5, 1.5, b, cin)
    scale = 1 / math.sqrt(9 * cin)
    temp = scale * wt * style.view(b, 1, cin, 1, 1)                     # models.py:320-328
    want = torch.rsqrt(temp.pow(2).sum([2, 3, 4]) + 1e-8)
    wsq = hip.weight_sqsum_f64(wt.to(DEV), scale)
    close(wsq, ((scale * wt[0]) ** 2).sum((2, 3)), 'weight_sqsum_f64')
    close(hip.demod_f64(wsq, style.to(DEV)), want, 'demod_f64')


# ---------------------------------------------------------------------------------------------- 2. model
_cache = {}


def case(size, batch, cm=2, mconv='seq'):
    """(generator on the device, its float64 state dict, z, the restatement's image and stages), computed once."""
    key = (size, batch, cm, mconv)
    if key not in _cache:
        g, sd, z = f64.double_generator(size, batch, channel_multiplier=cm, mconv=mconv, device=DEV)
        _cache[key] = (g, sd, z) + f64.truth(sd, z, size)
    return _cache[key]


@pytest.mark.parametrize('size,batch,cm', [(32, 3, 2), (64, 2, 1)])
def test_double_generator_matches_the_restatement_at_every_stage(size, batch, cm):
    g, sd, z, want, stages = case(size, batch, cm)
    img, got = f64.run_hooked(g, z.to(DEV), stages)
    close(img, want, 'size %d image' % size)
    for name in stages:
        close(got[name], stages[name], 'size %d %s' % (size, name))
    with torch.no_grad():
        bag = nethook.subsequence(g, upto_layer='latents')(z.to(DEV))
        full = nethook.subsequence(g, last_layer='to_rgb%d' % (int(math.log2(size)) - 1))(z.to(DEV))
    assert bag.latent.dtype == D
    for field in ('latent', 'style', 'fmap', 'output'):
        assert full[field].dtype == D, field


def test_double_generator_with_the_plain_modulated_convolution():
    g, sd, z, want, _ = case(32, 3, mconv=None)
    with torch.no_grad():
        img = g(z.to(DEV))
    close(img, want, 'mconv=None image')


def test_sliced_and_hooked_double_models():
    g, sd, z, want, stages = case(32, 3)
    with torch.no_grad():
        # upto_layer is exclusive: the slice up to ...adain ends on the map ApplyStyle reads (and its style), the slice up to
        # ...dconv -- the rewriter's context model -- on the key map
        before = nethook.subsequence(g, upto_layer='layer5.sconv.mconv.adain', share_weights=True)(z.to(DEV))
        key = nethook.subsequence(g, upto_layer='layer5.sconv.mconv.dconv', share_weights=True)(z.to(DEV))
        plain = g(z.to(DEV))
        with nethook.InstrumentedModel(g) as inst:
            inst.retain_layer('layer4.sconv.mconv.dconv', detach=False)
            hooked = inst(z.to(DEV))
            assert inst.retained_layer('layer4.sconv.mconv.dconv').fmap.dtype == D
    close(before.fmap, stages['layer4.sconv.activate'], 'the map in front of ApplyStyle, from a slice')
    close(before.style, stages['layer5.sconv.style'], 'the style of a slice')
    close(key.fmap, stages['layer5.sconv.adain'], 'the key map of a slice')
    assert key.output.dtype == D and key.latent.dtype == D and key.style.dtype == D
    assert torch.equal(plain, hooked)


# ---------------------------------------------------------------------------------------------- 3. oracle of the fp32 forward
def test_the_double_image_is_the_oracle_of_the_fp32_image_at_256():
    """The project's own image bar (BASELINE.json: images within 1e-3 L-inf), with the float64 forward of the same
    weights as the truth."""
    g = models.SeqStyleGAN2(256, 512, 8, truncation=0.5, mconv='seq')
    synthetic.randomize_(g, seed=0)
    g = g.eval().to(DEV)
    z = zdataset.standard_z_sample(1, 512, seed=1).to(DEV)
    with torch.no_grad():
        img32 = g(z)
        img64 = g.double()(z.double())
    assert img32.dtype == torch.float32 and img64.dtype == D
    err = (img32.double() - img64).abs().max().item()
    print('size 256: max |img_fp32 - img_f64| = %.3e (image magnitude %.2f)' % (err, img64.abs().max().item()))
    assert err < 1e-3, err


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_name_their_reason():
    from rewriting_amd.rewrite import ganrewrite
    g, sd, z, _, _ = case(32, 3)
    zd = z.to(DEV)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r'torch\.float32.*torch\.float64'):
            g(zd.float())
    x = torch.zeros(1, 16, 4, 4, dtype=D, device=DEV)
    with pytest.raises(RuntimeError, match=r'weight is torch\.float32.*takes torch\.float64'):
        hip.conv3x3_f64(x, torch.zeros(16, 16, 3, 3, device=DEV), 1.0)
    with torch.enable_grad():
        assert g.layer3.sconv.mconv.dconv.weight.requires_grad
        with pytest.raises(NotImplementedError, match='forward only'):
            g(zd)
        with pytest.raises(NotImplementedError, match='forward only'):
            nethook.subsequence(g, first_layer='layer3.sconv.mconv.dconv', last_layer='layer3.sconv.mconv.dconv',
                                share_weights=True)(models.DataBag(fmap=x.new_zeros(1, 512, 4, 4),
                                                                   style=x.new_ones(1, 512)))
    with pytest.raises(RuntimeError, match='float32 only'):
        ganrewrite.SeqStyleGanRewriter(g, zd, 5)
