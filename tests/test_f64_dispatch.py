"""The float64 forward above the C ABI, without a GPU: the ten _f64 entries are exported and bound, their wrappers
refuse host tensors, and a .double() generator dispatches every module to them -- checked by replacing the wrappers
with torch-double stand-ins defined here and comparing the size-32 image and stages with oracle/restatement.py."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from rewriting_amd import _lib, hip
from rewriting_amd.utils.stylegan2 import models
from tests import f64_common as f64

F64_ENTRIES = ['rw_pixel_norm_f64', 'rw_equal_linear_f64', 'rw_adjust_latent_f64', 'rw_style_mul_f64',
               'rw_weight_sqsum_f64', 'rw_demod_f64', 'rw_noise_add_f64', 'rw_to_rgb_f64', 'rw_conv3x3_f64',
               'rw_conv_transpose3x3s2_f64']
F64_WRAPPERS = [n[3:] for n in F64_ENTRIES]
# what the fp32 forward calls for the same modules (and its packing / fused forms): none may run for a double model
F32_WRAPPERS = ['pixel_norm', 'equal_linear', 'adjust_latent', 'style_mul', 'weight_sqsum', 'demod', 'noise_add', 'to_rgb',
                'conv3x3', 'conv_transpose3x3s2', 'pack_conv_weight', 'pack_conv_weight_wino', 'conv3x3_wino',
                'pack_conv_weight_wino4', 'conv3x3_wino4', 'conv_transpose3x3s2_wino', 'blur_noise_act',
                'conv3x3_direct16', 'conv_transpose3x3s2_blur_fused', 'fused_bias_act', 'upfirdn2d_major', 'absmax']


def test_the_f64_entries_are_exported_and_bound():
    assert os.path.isfile(_lib.LIB_PATH), 'run __graft_entry__.build() first'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in F64_ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
        assert ctypes.c_float not in _lib.SIGNATURES[name][1], name         # every scalar is a double
    for name in F64_WRAPPERS:
        assert callable(getattr(hip, name)), name


def test_abi_version_covers_the_f64_entries():
    """The version that introduced the _f64 forward (10: the library stood at 9 before it), so that the loader calls a
    library without these symbols stale."""
    assert _lib.load().rw_abi_version() == _lib.ABI_VERSION == 11


def test_f64_wrappers_refuse_host_tensors_device_first():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.pixel_norm_f64(torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # the device is checked before the dtype
        hip.pixel_norm_f64(torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.conv3x3_f64(torch.zeros(1, 4, 4, 4, dtype=torch.float64), torch.zeros(16, 4, 3, 3, dtype=torch.float64), 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.equal_linear_f64(torch.zeros(2, 8), torch.zeros(4, 8, dtype=torch.float64), None, 1.0, 1.0)


# ---- torch-double stand-ins with the wrappers' interfaces
def _all_double(*tensors):
    for t in tensors:
        assert t is None or t.dtype == torch.float64, t.dtype


def pixel_norm_f64(x, eps=1e-8):
    _all_double(x)
    return x * torch.rsqrt(torch.mean(x ** 2, dim=1, keepdim=True) + eps)


def equal_linear_f64(x, weight, bias, w_scale, b_scale, act=False, alpha=0.2, act_scale=2 ** 0.5):
    _all_double(x, weight, bias)
    x, weight = x.detach(), weight.detach()
    if act:
        return R.fused_leaky_relu(F.linear(x, weight * w_scale), bias.detach() * b_scale, alpha, act_scale)
    return F.linear(x, weight * w_scale, bias=None if bias is None else bias.detach() * b_scale)


def adjust_latent_f64(w, avg, n_latent, psi):
    _all_double(w, avg)
    if avg is not None:
        w = avg + psi * (w - avg)
    return w.unsqueeze(1).repeat(1, n_latent, 1)


def style_mul_f64(x, style):
    _all_double(x, style)
    return style.detach()[:, :, None, None] * x.detach()


def weight_sqsum_f64(weight, w_scale):
    _all_double(weight)
    w = weight.detach().reshape(weight.shape[-4], weight.shape[-3], -1)
    return ((w * w_scale) ** 2).sum(-1)


def demod_f64(wsq, style, eps=1e-8):
    _all_double(wsq, style)
    return torch.rsqrt((style.detach() ** 2) @ wsq.t() + eps)


def _mod(x, style, demod, conv):
    _all_double(x, style, demod)
    x = x.detach()
    if style is not None:
        x = x * style.detach()[:, :, None, None]
    y = conv(x)
    return y if demod is None else y * demod[:, :, None, None]


def conv3x3_f64(x, weight, w_scale, style=None, demod=None):
    _all_double(weight)
    assert weight.ndim == 4
    return _mod(x, style, demod, lambda v: F.conv2d(v, w_scale * weight.detach(), padding=1))


def conv_transpose3x3s2_f64(x, weight, w_scale, style=None, demod=None):
    _all_double(weight)
    assert weight.ndim == 4
    return _mod(x, style, demod, lambda v: F.conv_transpose2d(v, w_scale * weight.detach().transpose(0, 1), stride=2))


def noise_add_f64(x, noise, noise_w):
    _all_double(x, noise, noise_w)
    b, _, h, w = x.shape
    return x.detach() + noise_w.detach() * noise.reshape(b, 1, h, w)


def to_rgb_f64(x, weight, style, bias, skip, w_scale):
    _all_double(x, weight, style, bias, skip)
    wmod = w_scale * weight.detach()[None] * style.detach()[:, None, :]
    out = torch.einsum('bci,bihw->bchw', wmod, x.detach())
    if bias is not None:
        out = out + bias.detach().view(1, 3, 1, 1)
    return out if skip is None else out + skip


@pytest.fixture
def double_stand_ins(monkeypatch):
    called = set()

    def counted(name, fn):
        def run(*a, **k):
            called.add(name)
            return fn(*a, **k)
        return run

    def refuses(name):
        def run(*a, **k):
            raise AssertionError('the fp32 wrapper hip.%s ran for a double model' % name)
        return run
    for name in F64_WRAPPERS:
        monkeypatch.setattr(hip, name, counted(name, globals()[name]))
    for name in F32_WRAPPERS:
        monkeypatch.setattr(hip, name, refuses(name))
    # the two native ops took double before this path existed; their stand-ins are the restatement's
    monkeypatch.setattr(hip, 'fused_bias_act_f64',
                        lambda x, b, ref, act, grad, alpha, scale: R.fused_bias_act(
                            x.detach(), None if b is None else b.detach(), ref, act, grad, alpha, scale))
    monkeypatch.setattr(hip, 'upfirdn2d_major_f64', lambda x, k, *a: R.upfirdn2d_major(x.detach(), k.detach(), *a))
    return called


def test_a_double_model_runs_on_the_f64_wrappers_and_on_nothing_else(double_stand_ins):
    g, sd, z = f64.double_generator(32, 3)
    want, stages = f64.truth(sd, z, 32)
    img, got = f64.run_hooked(g, z, stages)
    f64.assert_close(img, want, 'image')
    for name in stages:
        f64.assert_close(got[name], stages[name], name)
    assert double_stand_ins == set(F64_WRAPPERS)            # every one of the ten ran


def test_the_plain_modulated_convolution_takes_the_same_dispatch(double_stand_ins):
    g, sd, z = f64.double_generator(32, 3, mconv=None)
    want, _ = f64.truth(sd, z, 32)
    with torch.no_grad():
        img = g(z)
    f64.assert_close(img, want, 'image')


def test_mixed_dtypes_grad_mode_and_the_rewriter_are_refused(double_stand_ins):
    from rewriting_amd.rewrite import ganrewrite
    g, _, z = f64.double_generator(32, 3)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r'torch\.float32.*torch\.float64'):
            g(z.float())
        with pytest.raises(RuntimeError, match=r'torch\.float64.*torch\.float32'):
            g.float()(z)
        g = g.double()
        with pytest.raises(RuntimeError, match=r'torch\.float64.*noise torch\.float32'):      # a float32 noise in the bag
            models.NoiseInjectionF().double()(models.DataBag(fmap=torch.zeros(1, 2, 4, 4, dtype=torch.float64),
                                                             noise=torch.zeros(1, 1, 4, 4)))
    with torch.enable_grad():
        assert g.layer3.sconv.mconv.dconv.weight.requires_grad
        with pytest.raises(NotImplementedError, match='forward only'):
            g(z)
    with pytest.raises(RuntimeError, match='float32 only'):
        ganrewrite.SeqStyleGanRewriter(g, z, 5)
    assert not double_stand_ins                                 # nothing ran
