"""The RANGE of the split-operand kernels on the device (DESIGN.md section 4.1 "Range"): every kernel that runs a 3x3
convolution on the 16-bit matrix pipe with exact f16 operand pairs scales its input by ONE power of two per image, read
off (bound of the whole map and batch) x (the image's largest |style|).  Three things are checked that well-conditioned
data and a global error measure cannot see:

 1. far field / batch neighbour -- one pixel of image 0 raised to 2^k times the map's former maximum; on the outputs that
    pixel cannot reach (geometry only: split_model.far_field), and on image 1 alone, the kernel must BE the model of the
    documented arithmetic (split_model.model: f16 denormals kept, headroom 14 / 8 / 12, per-image smax with fabs; float64
    from the rounding on)
    up to fp32 accumulation: || got - model || <= 4 || sibling - ref ||, sibling = the family's own fp32 kernel, ref = the
    float64 convolution.  One bit of headroom too few, or a flushed denormal, is ~50x that at k = 20.
 2. powers of two leave exactly -- kernel(x 2^a, pack(w 2^b)) == ldexp(kernel(x, pack(w)), a + b) bit for bit, the
    reported bound included, image 1's style 2^5 times image 0's; the fp32 siblings owe the same.
 3. signs and zeros -- a style whose largest entry is negative, a zero style row, a zero map, zero weights, a zero input
    channel and a zero filter: every place the exponent is read off a zero.

Which environment value reaches which kernel body (and with it each site that reads the exponent): split_model.FORMS.
The fused upsampling kernel's two persistent bodies take 32 input channels and up, so they run at (2, 32, 16, 16, 32).
Nothing here is compared with a number fitted to the kernels: the bars are the families' own (split_model.BARS)."""
import functools
import math

import pytest
import torch

from tests import split_model as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FORM_IDS = [f[0] for f in S.FORMS]


def _k4():
    return S.blur_kernel().to(DEV)


def _demod(wt, style, shape):
    from rewriting_amd import hip
    return hip.demod(hip.weight_sqsum(wt.to(DEV), S.w_scale_of(shape)), style.to(DEV))


def _pack(kind, wt, split=True):
    """the packed weights of the split-operand kernel, or (split=False) of its fp32 sibling"""
    from rewriting_amd import hip
    wt = wt.to(DEV)
    if kind == 'direct':
        return hip.pack_conv_weight_direct16(wt) if split else hip.pack_conv_weight(wt, 0)
    if kind == 'tconv':
        return hip.pack_conv_weight_direct16(wt) if split else hip.pack_conv_weight(wt, 1)
    if kind == 'dconv_up':
        return hip.pack_conv_transpose_blur_weight_direct16(wt, _k4()) if split else hip.pack_conv_weight(wt, 1)
    if kind == 'wino4':
        return hip.pack_conv_weight_wino4(wt, split=split)
    if kind == 'wino4_up':
        return hip.pack_conv_transpose_blur_weight_wino4(wt, _k4(), split=split)
    return hip.pack_conv_transpose_weight_wino(wt, split=split)


def _run(kind, shape, x, pk, style, dm, y_amax=None):
    """the split-operand kernel: no noise, bias or activation; x_amax=None (the wrapper measures the bound)"""
    from rewriting_amd import hip
    o, s = shape[2], S.w_scale_of(shape)
    x, style = x.to(DEV), style.to(DEV)
    if kind == 'direct':
        return hip.conv3x3_direct16(x, pk, o, s, style=style, demod=dm, y_amax=y_amax)
    if kind == 'tconv':
        return hip.conv_transpose3x3s2_blur_fused(x, pk, _k4(), o, s, style=style, demod=dm, y_amax=y_amax)
    if kind == 'dconv_up':
        return hip.conv_transpose3x3s2_blur_direct16(x, pk, o, s, style=style, demod=dm, y_amax=y_amax)
    if kind == 'wino4':
        return hip.conv3x3_wino4(x, pk, o, s, style=style, demod=dm, y_amax=y_amax)
    if kind == 'wino4_up':
        return hip.conv_transpose3x3s2_blur_wino4(x, pk, o, s, style=style, demod=dm, y_amax=y_amax)
    assert y_amax is None                                  # the F(2,2) kernel reports no bound
    return hip.conv_transpose3x3s2_wino(x, pk, o, s, style=style, demod=dm)[:, :, :-1, :-1].contiguous()


def _sibling(kind, shape, x, pk, style, dm):
    """the family's own fp32 route on the same inputs (pk = _pack(..., split=False))"""
    from rewriting_amd import hip
    i, o, s = shape[1], shape[2], S.w_scale_of(shape)
    x, style = x.to(DEV), style.to(DEV)
    if kind == 'direct':
        return hip.conv3x3(x, pk, o, s, style=style, demod=dm, impl=0)
    if kind in ('tconv', 'dconv_up'):
        wide = hip.conv_transpose3x3s2(x, pk, o, s, style=style, demod=dm, impl=0 if i % 16 == 0 and o % 32 == 0 else 1)
        return hip.blur_noise_act(wide, _k4(), None, None, None)
    if kind == 'wino4':
        return hip.conv3x3_wino4(x, pk, o, s, style=style, demod=dm)
    if kind == 'wino4_up':
        return hip.conv_transpose3x3s2_blur_wino4(x, pk, o, s, style=style, demod=dm)
    return hip.conv_transpose3x3s2_wino(x, pk, o, s, style=style, demod=dm)[:, :, :-1, :-1].contiguous()


def _has_bound(kind):
    return kind != 'upwino'


def _new_bound(kind, shape):
    from rewriting_amd import hip
    b, _, o, h, w = shape
    n = b * o * h * w * (4 if kind in S.UPSAMPLING else 1)
    return hip.new_bound(n, DEV).fill_(3e38)             # poisoned: every slot the reduction reads must be written


def _within_bars(kind, got, ref):
    rel_bar, linf_bar = S.BARS[kind]
    got, ref = got.double().cpu(), ref.double().cpu()
    e, linf, scale = ((got - ref).norm() / ref.norm()).item(), (got - ref).abs().max().item(), ref.abs().max().item()
    assert torch.isfinite(got).all()
    assert e < rel_bar, e
    assert linf < linf_bar * scale, linf / scale


# ---- 1. far field and batch neighbour
@functools.lru_cache(maxsize=None)
def _far_case(kind, shape, k, point_split=False):
    """(x, demod, model, ref, sibling) of one problem: made once, shared by the forms that run it, never changed"""
    x0, wt, style = S.inputs(kind, shape)
    x = S.raise_pixel(kind, x0, k)
    dm = _demod(wt, style, shape)
    s, k4 = S.w_scale_of(shape), S.blur_kernel()
    model = S.model(kind, x, wt, style, dm, s, k4, point_split=point_split)
    ref = S.reference(kind, x, wt, style, dm, s, k4)
    sib = _sibling(kind, shape, x, _pack(kind, wt, split=False), style, dm).cpu()
    return x, dm, model, ref, sib


@pytest.mark.parametrize('k', S.KS)
@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_far_field_and_batch_neighbour_follow_the_model(form, k, monkeypatch):
    """Far from the raised pixel, and in the image beside it, the kernel is the float64 model up to fp32 accumulation.

    MEASURED (MI355X; || got - model || in units of || sibling - ref || over the far field of the batch; allowed: 4): every
    form holds it at every k with a ratio that does not move from k = 0 to k = 20 -- the direct sums 0.7 .. 1.3, F(4x4)
    1.0 .. 1.3, its upsampling phases 1.0 .. 1.7, F(2,2) 1.0 -- so f16 denormals survive the conversions and the matrix
    instruction, and the headroom and fabs are right.
    The transformed families round AFTER an fp32 input transform, so the model takes that transform in the kernels' own
    fp32 operation order (split_model.wino4_input_points / upwino_input_points).  With the transform in float64 -- or in
    fp32 in any other order, hip_emulation.py's included -- the same kernels come out at 5.6 .. 38 from k = 16 on: where the
    far field sits in f16's denormals the quantum q = 2^-25 2^-eV is far above the transform's fp32 error d, a value that d
    moves across a rounding boundary comes out one whole q away, and two evaluations differ by sqrt(d q), not d."""
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    _, wt, style = S.inputs(kind, shape)
    x, dm, model, ref, sib = _far_case(kind, shape, k, env.get('RW_W4H_PS') == '1')
    got = _run(kind, shape, x, _pack(kind, wt), style, dm).cpu()
    far = S.far_field(kind, shape)
    assert got.shape == model.shape == ref.shape == sib.shape
    assert torch.isfinite(got).all()
    print('split range %s k=%d: far field got %.3g model %.3g sibling %.3g | image 1 got %.3g model %.3g sibling %.3g | '
          'got - model %.3g of 4 (sibling - ref) %.3g'
          % (name, k, S.far_rel(got, ref, far), S.far_rel(model, ref, far), S.far_rel(sib, ref, far),
             S.far_rel(got, ref, far, 1), S.far_rel(model, ref, far, 1), S.far_rel(sib, ref, far, 1),
             S.far_norm(got, model, far), 4 * S.far_norm(sib, ref, far)))
    # inside the footprint (and everywhere else): the family's bar over the global maximum
    assert (got.double() - ref).abs().max().item() < S.BARS[kind][1] * ref.abs().max().item()
    for image in (None, 1):
        assert S.far_norm(got, model, far, image) <= 4 * S.far_norm(sib, ref, far, image), (name, k, image)


@pytest.mark.parametrize('k', S.KS)
@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_far_field_error_is_the_models(form, k, monkeypatch):
    """The SIZE of the far field's error against float64 is the model's: || got - ref || <= sqrt(2) || model - ref || +
    4 || sibling - ref ||.  Where the shared power of two has pushed the far field into f16's denormals the model's error is
    the rounding to the quantum 2^-25 2^-eV (rms: quantum / sqrt(12)); a kernel with one bit of headroom less has twice
    that, one that flushes denormals 2^10 times -- sqrt(2) is half way, in bits, between what is owed and the smallest
    fault.  Unlike the difference from the model, the size does not depend on WHICH of two neighbouring f16 numbers a value
    that the fp32 input transform has moved by less than a quantum is rounded to: it holds whatever order that transform
    is compiled to."""
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    _, wt, style = S.inputs(kind, shape)
    x, dm, model, ref, sib = _far_case(kind, shape, k, env.get('RW_W4H_PS') == '1')
    got = _run(kind, shape, x, _pack(kind, wt), style, dm).cpu()
    far = S.far_field(kind, shape)
    for image in (None, 1):
        assert S.far_norm(got, ref, far, image) <= (2 ** 0.5 * S.far_norm(model, ref, far, image)
                                                    + 4 * S.far_norm(sib, ref, far, image)), (name, k, image)


# ---- 2. powers of two leave exactly
SCALINGS = [(-40, 0), (40, 0), (0, -20), (0, 20), (-7, 20), (7, -20)]


def _pow2_inputs(kind, shape):
    x, wt, style = S.inputs(kind, shape)
    style = style.clone()
    style[1] = style[0] * 32.0                            # per-image smax: image 1's exponent is 5 above image 0's
    return x, wt, style


def _ldexp(t, n):
    return t * 2.0 ** n                                   # exact (torch.ldexp goes through pow on the device)


@pytest.mark.parametrize('ab', SCALINGS, ids=['x%+d,w%+d' % ab for ab in SCALINGS])
@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_powers_of_two_leave_exactly(form, ab, monkeypatch):
    """With demod and w_scale unchanged, scaling x by 2^a and w by 2^b scales the result -- and the reported bound -- by
    2^(a + b) bit for bit: the exponents stay 40 and more away from the +-100 clamp and every factor inside fp32's
    normal range."""
    from rewriting_amd import hip
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    a, b = ab
    x, wt, style = _pow2_inputs(kind, shape)
    dm = _demod(wt, style, shape)
    xa, wb = _ldexp(x, a), _ldexp(wt, b)
    bounds = [_new_bound(kind, shape), _new_bound(kind, shape)] if _has_bound(kind) else [None, None]
    base = _run(kind, shape, x, _pack(kind, wt), style, dm, y_amax=bounds[0])
    got = _run(kind, shape, xa, _pack(kind, wb), style, dm, y_amax=bounds[1])
    assert torch.isfinite(base).all() and base.abs().max().item() > 0
    assert torch.equal(got, _ldexp(base, a + b))
    if _has_bound(kind):
        assert hip.bound_value(bounds[0]) == base.abs().max().item()
        assert hip.bound_value(bounds[1]) == hip.bound_value(bounds[0]) * 2.0 ** (a + b)


@pytest.mark.parametrize('ab', SCALINGS, ids=['x%+d,w%+d' % ab for ab in SCALINGS])
@pytest.mark.parametrize('kind,shape', S.PROBLEMS)
def test_powers_of_two_leave_the_fp32_siblings_exactly(kind, shape, ab):
    """The same identity for the fp32 routes: they owe it too, which tells a kernel's fault from this test's."""
    a, b = ab
    x, wt, style = _pow2_inputs(kind, shape)
    dm = _demod(wt, style, shape)
    base = _sibling(kind, shape, x, _pack(kind, wt, split=False), style, dm)
    got = _sibling(kind, shape, _ldexp(x, a), _pack(kind, _ldexp(wt, b), split=False), style, dm)
    assert torch.isfinite(base).all() and base.abs().max().item() > 0
    assert torch.equal(got, _ldexp(base, a + b))


# ---- 3. signs and zeros
@functools.lru_cache(maxsize=None)
def _negative_style(kind, shape):
    """every row: entries in +-1, exact zeros, and -3.0 as the entry of largest magnitude"""
    b, i = shape[0], shape[1]
    g = torch.Generator().manual_seed(77 + i)
    style = torch.rand(b, i, generator=g) * 2 - 1
    style[:, 1::5] = 0.0
    style[0, 2] = style[1, i - 3] = -3.0
    assert (style.abs().amax(1) == 3.0).all() and (style.amin(1) == -3.0).all() and (style.amax(1) < 3.0).all()
    return style


@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_style_whose_largest_entry_is_negative(form, monkeypatch):
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    x, wt, _ = S.inputs(kind, shape)
    style = _negative_style(kind, shape)
    dm = _demod(wt, style, shape)
    got = _run(kind, shape, x, _pack(kind, wt), style, dm)
    _within_bars(kind, got, S.reference(kind, x, wt, style, dm, S.w_scale_of(shape), S.blur_kernel()))


@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_zero_style_row(form, monkeypatch):
    """Image 1's style is all zero (its exponent is read off 0): its output is exactly zero, image 0's does not move."""
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    x, wt, style = S.inputs(kind, shape)
    zeroed = style.clone()
    zeroed[1] = 0.0
    dm, dmz = _demod(wt, style, shape), _demod(wt, zeroed, shape)
    assert torch.equal(dm[0], dmz[0]) and torch.isfinite(dmz).all()
    pk = _pack(kind, wt)
    bound = _new_bound(kind, shape) if _has_bound(kind) else None
    before, got = _run(kind, shape, x, pk, style, dm), _run(kind, shape, x, pk, zeroed, dmz, y_amax=bound)
    assert torch.isfinite(got).all()
    assert (got[1] == 0.0).all()
    assert torch.equal(got[0], before[0]) and before[0].abs().max().item() > 0
    if bound is not None:
        from rewriting_amd import hip
        assert hip.bound_value(bound) == got.abs().max().item()


@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_zero_input_map(form, monkeypatch):
    from rewriting_amd import hip
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    x, wt, style = S.inputs(kind, shape)
    bound = _new_bound(kind, shape) if _has_bound(kind) else None
    got = _run(kind, shape, torch.zeros_like(x), _pack(kind, wt), style, _demod(wt, style, shape), y_amax=bound)
    assert torch.isfinite(got).all() and (got == 0.0).all()
    if bound is not None:
        assert hip.bound_value(bound) == 0.0


@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_zero_weight(form, monkeypatch):
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    x, wt, style = S.inputs(kind, shape)
    zero = torch.zeros_like(wt)
    pk = _pack(kind, zero)
    u_inv = float(pk.rw_u_inv)
    assert math.isfinite(u_inv) and u_inv > 0 and math.frexp(u_inv)[0] == 0.5         # a power of two
    dm = _demod(zero, style, shape)
    assert torch.isfinite(dm).all()
    got = _run(kind, shape, x, pk, style, dm)
    assert torch.isfinite(got).all() and (got == 0.0).all()


@pytest.mark.parametrize('form', S.FORMS, ids=FORM_IDS)
def test_zero_input_channel_and_zero_filter(form, monkeypatch):
    name, kind, shape, env = form
    S.set_env(monkeypatch, env)
    x, wt, style = S.inputs(kind, shape)
    x, wt = x.clone(), wt.clone()
    x[:, 2] = 0.0
    wt[0, 5] = 0.0
    dm = _demod(wt, style, shape)
    got = _run(kind, shape, x, _pack(kind, wt), style, dm)
    _within_bars(kind, got, S.reference(kind, x, wt, style, dm, S.w_scale_of(shape), S.blur_kernel()))
    assert (got[:, 5] == 0.0).all() and got[:, 4].abs().max().item() > 0
