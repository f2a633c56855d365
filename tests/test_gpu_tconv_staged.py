"""The STAGED forms of the fused upsampling kernel (csrc/rw_tconv.hip, round 12): a pre-pass (split_map_kernel) writes the
map once as the operand words the window buffer takes, and the convolution copies its windows from there into LDS where
the present form loads fp32, multiplies by the style, splits and writes them once per 16 (32) out-channels.  The pre-pass
runs the present form's arithmetic on the same inputs, so everything here is EQUALITY: the result and the reported bound
against the present form of the same shape (torch.equal: a padding -0 counts as +0 -- the present form multiplies its
padding zeros by the style), the words against a numpy model bit for bit.

The forms are forced with RW_TCONV_TY (8 / 16 / 32), RW_TCONV_STAGED (1 / 0) and RW_TCONV_STAGED_MIN_IN = 16; the scratch is
this file's own tensor, registered with rw_tconv_stage_buffer around the one launch that may use it -- filled with a NaN
pattern first, so that a staged launch shows (the words are there afterwards) and a word that is read but was never
written cannot pass.  Shapes (B, Cin, Cout, H, W): one tile and one chunk; 2 x 2 tiles of three chunks (both buffer
parities, an odd count), two out-channel tiles and two images; a tile with neighbours above and below; one with
neighbours left and right."""
import math

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 16, 16, 16, 32), (2, 48, 32, 32, 64), (1, 32, 16, 48, 32), (1, 32, 32, 16, 96)]
FORMS = [(shape, ty) for shape in SHAPES for ty in (16, 8, 32) if ty != 32 or shape[2] % 32 == 0]
OPTIONS = ('style', 'demod', 'noise', 'bias_act', 'post_scale')
PATTERN = 0xff            # bytes of the scratch before a launch: every half a NaN
_cache = {}


def _inputs(shape):
    """Everything a launch of `shape` takes, made once and left unchanged."""
    if shape not in _cache:
        from rewriting_amd import hip
        b, i, o, h, w = shape
        rs = numpy.random.RandomState(1200 + i + h)
        t = lambda a: torch.from_numpy(numpy.asarray(a, dtype='float32')).to(DEV)
        x = t(rs.randn(b, i, h, w) * numpy.exp(rs.randn(1, i, 1, 1)))
        wt = t(rs.randn(1, o, i, 3, 3))
        style = t(1 + 0.3 * rs.randn(b, i))
        s = 1 / math.sqrt(i * 9)
        k1 = torch.tensor([1., 3., 3., 1.])
        k4 = k1[:, None] * k1[None, :]
        _cache[shape] = dict(
            x=x, s=s, k4=(k4 / k4.sum() * 4).to(DEV), pk=hip.pack_conv_weight_direct16(wt), amax=hip.absmax(x),
            style=style, demod=hip.demod(hip.weight_sqsum(wt, s), style), noise=t(rs.randn(b, 1, 2 * h, 2 * w)),
            noise_w=torch.tensor([0.37], device=DEV), bias=t(rs.randn(o)), post_scale=t(1 + 0.3 * rs.randn(b, o)))
    return _cache[shape]


def _keywords(d, options):
    kw = {}
    for name in options:
        if name == 'noise':
            kw.update(noise=d['noise'], noise_w=d['noise_w'])
        elif name == 'bias_act':
            kw.update(bias=d['bias'], act=True)
        else:
            kw[name] = d[name]
    return kw


def _need(shape):
    b, i, _, h, w = shape
    return b * i * h * w * 4


def _scratch(nbytes):
    return torch.full((nbytes,), PATTERN, dtype=torch.uint8, device=DEV)


def _launch(monkeypatch, shape, ty, staged, scratch=None, x=None, x_amax=None, **kw):
    """(result, reported bound) of one launch of rw_tconv_blur_f32 in the form `ty`, with `scratch` (or nothing) registered
    for the stream while it is called -- what hip.conv_transpose3x3s2_blur_fused does, with the test's own buffer."""
    from rewriting_amd import hip
    d = _inputs(shape)
    b, i, o, h, w = shape
    monkeypatch.setenv('RW_TCONV_TY', str(ty))
    monkeypatch.setenv('RW_TCONV_STAGED', '1' if staged else '0')
    monkeypatch.setenv('RW_TCONV_STAGED_MIN_IN', '16')
    x = d['x'] if x is None else x
    assert hip.lib().rw_tconv_stage_bytes(b, i, o, h, w) == (_need(shape) if staged else 0)
    y = hip._out(x, o, up=2)
    ymax = hip.new_bound(y.numel(), DEV).fill_(3e38)
    if scratch is not None:
        hip.check(hip.lib().rw_tconv_stage_buffer(hip._stream(), hip._p(scratch), scratch.numel()))
    try:
        hip._conv('rw_tconv_blur_f32', x, hip._packed(d['pk'], o, i, hip._DIRECT16), o, d['s'],
                  hip._epilogue(kw.get('style'), kw.get('demod'), kw.get('noise'), kw.get('noise_w'), kw.get('bias'),
                                kw.get('act', False)),
                  x_amax=d['amax'] if x_amax is None else x_amax, k4=d['k4'], y=y,
                  post_scale=kw.get('post_scale'), y_amax=ymax)
    finally:
        hip.check(hip.lib().rw_tconv_stage_buffer(hip._stream(), None, 0))
    return y, hip.bound_value(ymax)


def _untouched(t):
    return bool((t == PATTERN).all())


@pytest.mark.parametrize('shape,ty', FORMS)
def test_staged_form_equals_the_present_form(shape, ty, monkeypatch):
    """Result and reported bound, for each option of the epilogue alone, none of them and all of them."""
    d = _inputs(shape)
    for options in [()] + [(name,) for name in OPTIONS] + [OPTIONS]:
        kw = _keywords(d, options)
        want, want_bound = _launch(monkeypatch, shape, ty, False, **kw)
        scratch = _scratch(_need(shape))
        got, got_bound = _launch(monkeypatch, shape, ty, True, scratch, **kw)
        assert not _untouched(scratch), 'the staged form did not run'
        assert torch.isfinite(got).all(), options
        assert torch.equal(got, want), (options, (got - want).abs().max().item())
        assert got_bound == want_bound == got.abs().max().item(), options


def _model_words(x, style, bound):
    """words[image][chunk][y][x][quad][8 halves] as uint16: float32 product with style * in_scale (rounded first), float16
    round-to-nearest, the exact float32 residual, float16 again."""
    b, i, h, w = x.shape
    out = numpy.empty((b, i // 16, h, w, 4, 8), dtype=numpy.uint16)
    for ib in range(b):
        am = numpy.float32(bound) * numpy.abs(style[ib]).max().astype(numpy.float32)
        e = int((am.view(numpy.uint32) >> 23) & 0xff) - 126
        e = min(max(e, -100), 100)
        sv = (style[ib] * numpy.float32(2.0 ** (14 - e))).astype(numpy.float32)
        v = (x[ib] * sv[:, None, None]).astype(numpy.float32)
        hi = v.astype(numpy.float16)
        lo = (v - hi.astype(numpy.float32)).astype(numpy.float16)
        for part, halves in ((0, hi), (4, lo)):
            q = halves.view(numpy.uint16).reshape(i // 16, 4, 4, h, w)             # chunk, quad, channel of the quad
            out[ib, :, :, :, :, part:part + 4] = q.transpose(0, 3, 4, 1, 2)
    return out


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_words_of_the_pre_pass_are_the_numpy_models(shape, monkeypatch):
    """Inputs in the normal range of both halves (|x| in [1/4, 1), |style| in [1/2, 1]: |V| >= 2^10, so a residual is 0 or at
    least 2^-13), signs mixed, and one more image that is all zeros (its words: the signed zeros of 0 x style)."""
    b, i, o, h, w = shape
    rs = numpy.random.RandomState(77 + i)
    x = (rs.uniform(0.25, 1.0, (b + 1, i, h, w)) * rs.choice([-1.0, 1.0], (b + 1, i, h, w))).astype('float32')
    x[b] = 0.0
    style = (rs.uniform(0.5, 1.0, (b + 1, i)) * rs.choice([-1.0, 1.0], (b + 1, i))).astype('float32')
    from rewriting_amd import hip
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(style).to(DEV)
    amax = hip.absmax(xd)
    big = (b + 1, i, o, h, w)
    _cache[big] = dict(_inputs(shape), x=xd, amax=amax)
    try:
        scratch = _scratch(_need(big))
        got, _ = _launch(monkeypatch, big, 16, True, scratch, style=sd)
        want, _ = _launch(monkeypatch, big, 16, False, style=sd)
    finally:
        del _cache[big]
    assert torch.equal(got, want)
    words = scratch.cpu().numpy().view(numpy.uint16).reshape(b + 1, i // 16, h, w, 4, 8)
    model = _model_words(x, style, hip.bound_value(amax))
    assert numpy.array_equal(words, model), int((words != model).sum())
    assert not numpy.isnan(words.view(numpy.float16)).any()


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_every_word_read_was_written_and_nothing_beyond(shape, monkeypatch):
    """A scratch 4 KB larger than needed, all NaN halves before the launch: the result is the present form's (a word read
    but not written would be NaN), no NaN pattern is left where the words are, the tail keeps its pattern."""
    d = _inputs(shape)
    kw = _keywords(d, OPTIONS)
    need = _need(shape)
    scratch = _scratch(need + 4096)
    got, got_bound = _launch(monkeypatch, shape, 16, True, scratch, **kw)
    want, want_bound = _launch(monkeypatch, shape, 16, False, **kw)
    assert torch.equal(got, want) and got_bound == want_bound
    halves = scratch[:need].view(torch.float16)
    assert not torch.isnan(halves).any()
    assert _untouched(scratch[need:])


@pytest.mark.parametrize('ty', (16, 8))
def test_loose_bound_and_negative_styles(ty, monkeypatch):
    """A bound 37 times too large (other scales, the same rule in both forms) and an image whose style row is negative."""
    shape = SHAPES[1]
    d = _inputs(shape)
    style = d['style'].clone()
    style[0] = -style[0].abs()
    kw = dict(_keywords(d, OPTIONS), style=style)
    loose = d['amax'] * 37.0
    got, got_bound = _launch(monkeypatch, shape, ty, True, _scratch(_need(shape)), x_amax=loose, **kw)
    want, want_bound = _launch(monkeypatch, shape, ty, False, x_amax=loose, **kw)
    assert torch.equal(got, want) and got_bound == want_bound


@pytest.mark.parametrize('scratch_bytes', (None, -16))
def test_without_a_large_enough_buffer_the_present_form_runs(scratch_bytes, monkeypatch):
    """No buffer registered, or one 16 bytes too small (which stays untouched): the result is the present form's."""
    shape = SHAPES[1]
    kw = _keywords(_inputs(shape), OPTIONS)
    scratch = None if scratch_bytes is None else _scratch(_need(shape) + scratch_bytes)
    got, got_bound = _launch(monkeypatch, shape, 16, True, scratch, **kw)
    want, want_bound = _launch(monkeypatch, shape, 16, False, **kw)
    assert torch.equal(got, want) and got_bound == want_bound
    assert scratch is None or _untouched(scratch)


def test_the_wrapper_stages_through_its_own_scratch(monkeypatch):
    """hip.conv_transpose3x3s2_blur_fused at 256 input channels, staged through the wrapper's own scratch: equal to
    RW_TCONV_STAGED = 0."""
    from rewriting_amd import hip
    shape = (1, 256, 16, 16, 32)
    d = _inputs(shape)
    kw = dict(_keywords(d, OPTIONS), x_amax=d['amax'])
    monkeypatch.setenv('RW_TCONV_TY', '16')
    monkeypatch.setenv('RW_TCONV_STAGED_MIN_IN', '16')
    monkeypatch.setenv('RW_TCONV_STAGED', '1')
    got = hip.conv_transpose3x3s2_blur_fused(d['x'], d['pk'], d['k4'], shape[2], d['s'], **kw)
    monkeypatch.setenv('RW_TCONV_STAGED', '0')
    want = hip.conv_transpose3x3s2_blur_fused(d['x'], d['pk'], d['k4'], shape[2], d['s'], **kw)
    assert torch.equal(got, want)
