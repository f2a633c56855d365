"""TEST INFRASTRUCTURE -- the documented arithmetic of the split-operand kernels (rw_dconv.hip, rw_tconv.hip, rw_wino4.hip,
rw_upwino.hip) evaluated in float64, and the inputs, references and geometry the range tests share
(test_split_model.py on the host, test_gpu_split_range.py on the device).

The model is hip_emulation.py's statement of these kernels with ONE thing kept from the device: the rounding of the scaled
operands to pairs of f16 numbers, with the kernels' exponent rule (rw_exp_above / rw_split_scales in csrc/rw_common.h:
((bits >> 23) & 0xff) - 126 of bound * smax in fp32, clamped to +-100, smax per image).  The style product is the kernels' fp32 product and so is what else precedes the
rounding -- the input transform of the F(4x4,3x3) and F(2,2) kernels, in their own operation order; every sum after the
rounding is float64, so what separates a kernel from the model is its fp32 accumulation -- nothing that depends on the
range of the data.  The code is hip_emulation's own (its functions take any dtype).
"""
import functools
import math

import numpy
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests import hip_emulation as E

# kind -> the headroom of its input scale: |V| < 2^top (direct sums 14; F(4x4,3x3), gain 100 < 2^7: 8; F(2,2), gain 4: 12)
TOP = {'direct': 14, 'dconv_up': 14, 'tconv': 14, 'wino4': 8, 'wino4_up': 8, 'upwino': 12}
UPSAMPLING = ('dconv_up', 'tconv', 'wino4_up', 'upwino')
# the bars the suite holds each family to against float64 (test_gpu_kernels.py, test_gpu_dconv_pairs.py):
# (relative l2, L-infinity over the global maximum)
BARS = {'direct': (3e-6, 2e-5), 'dconv_up': (3e-6, 2e-5), 'tconv': (3e-6, 2e-5), 'upwino': (3e-6, 2e-5),
        'wino4': (2e-5, 1e-4), 'wino4_up': (3e-5, 1e-4)}
KS = (0, 12, 16, 20)

# (name, kind, (batch, in, out, h, w), environment).  The exponent rule is written once, rw_exp_above() in rw_common.h:
# every kernel body reaches it through rw_split_scales<headroom>(bound * smax, ...), the host through rw_weight_scale_of().
# Which value reaches which body, each with its own bound * smax and headroom:
#   rw_dconv.hip   dconv_body              -- RW_DCONV_V=1 always; the upsampling mode below 32 input channels under both
#                  dconv_ws_body           -- RW_DCONV_V=2 with in >= 32, out % 64 == 0, w % 64 == 0
#   rw_tconv.hip   tconv_body              -- RW_TCONV_TY=8 / 16; unset outside 32 <= in <= 128; ANY value below 32 channels
#                  tconv_ws_body           -- RW_TCONV_TY=0 and unset with 32 <= in <= 128: needs in >= 32
#                  tconv_blur_pp_kernel    -- RW_TCONV_TY=2, in >= 32
#   rw_wino4.hip   conv_wino36b_body       -- one body for stride 1 and the upsampling phases; RW_W4H_PS=0 / 1 its two
#                                             ways of dealing the 36 points to the waves
#   rw_upwino.hip  conv_up_wino_body
#   rw_common.h    rw_weight_scale_of      -- every pack_* call (the zero-weight case reads it off a zero)
# The fused upsampling kernel's persistent bodies do not take 16 input channels, so they run at (2, 32, 16, 16, 32), the
# smallest shape they take.
FORMS = [
    ('direct16-one-role', 'direct', (2, 16, 32, 16, 32), {'RW_DCONV_V': '1'}),
    ('direct16-specialised', 'direct', (2, 32, 64, 16, 64), {'RW_DCONV_V': '2'}),
    ('up-direct16-v1', 'dconv_up', (2, 16, 16, 8, 32), {'RW_DCONV_V': '1'}),
    ('up-direct16-v2', 'dconv_up', (2, 16, 16, 8, 32), {'RW_DCONV_V': '2'}),
    ('up-fused-ty8', 'tconv', (2, 16, 16, 16, 32), {'RW_TCONV_TY': '8'}),
    ('up-fused-ty16', 'tconv', (2, 16, 16, 16, 32), {'RW_TCONV_TY': '16'}),
    ('up-fused-auto', 'tconv', (2, 16, 16, 16, 32), {'RW_TCONV_TY': None}),
    ('up-fused-persistent', 'tconv', (2, 32, 16, 16, 32), {'RW_TCONV_TY': '0'}),
    ('up-fused-pipelined', 'tconv', (2, 32, 16, 16, 32), {'RW_TCONV_TY': '2'}),
    ('up-fused-auto-persistent', 'tconv', (2, 32, 16, 16, 32), {'RW_TCONV_TY': None}),
    ('wino4-split', 'wino4', (2, 16, 32, 16, 64), {'RW_W4H_PS': '0'}),
    ('wino4-split-ps', 'wino4', (2, 16, 32, 16, 64), {'RW_W4H_PS': '1'}),
    ('up-wino4-split', 'wino4_up', (2, 16, 16, 8, 64), {}),
    ('up-f22-split', 'upwino', (2, 16, 32, 4, 32), {}),
]
PROBLEMS = sorted({(kind, shape) for _, kind, shape, _ in FORMS})


def set_env(monkeypatch, env):
    for name, value in env.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def blur_kernel():
    k1 = torch.tensor([1., 3., 3., 1.])
    k4 = k1[:, None] * k1[None, :]
    return k4 / k4.sum() * 4


@functools.lru_cache(maxsize=None)
def inputs(kind, shape):
    """x (randn x exp(randn) per channel), Gaussian weights, style 1 + 0.3 randn -- made once per problem, never changed"""
    b, i, o, h, w = shape
    rs = numpy.random.RandomState(4100 + sorted(TOP).index(kind) * 16 + i)
    x = torch.from_numpy(rs.randn(b, i, h, w).astype('float32'))
    wt = torch.from_numpy(rs.randn(1, o, i, 3, 3).astype('float32'))
    style = torch.from_numpy((1 + 0.3 * rs.randn(b, i)).astype('float32'))
    x = x * torch.from_numpy(numpy.exp(rs.randn(1, i, 1, 1)).astype('float32'))
    return x, wt, style


def raised_pixel(kind):
    """(channel, y, x) of the raised pixel: where it sits in TWO tiles per axis of the tiled forms"""
    return (3, 1, 5) if kind == 'upwino' else (3, 4, 12)


def raise_pixel(kind, x, k):
    """image 0: one pixel of one channel at 2^k times the former max |x|"""
    c, py, px = raised_pixel(kind)
    x = x.clone()
    x[0, c, py, px] = torch.ldexp(x.abs().max(), torch.tensor(k))
    return x


def _tiles(p, stride, lo, hi):
    """first and last tile t whose window [stride t + lo, stride t + hi] holds p"""
    return -((hi - p) // stride), (p - lo) // stride


def far_field(kind, shape):
    """The outputs the raised pixel cannot reach, from geometry alone: a bool mask (b, 1, H_out, W_out); all of image 1."""
    b, i, o, h, w = shape
    _, py, px = raised_pixel(kind)
    up = kind in UPSAMPLING
    hh, ww = (2 * h, 2 * w) if up else (h, w)

    def span(p):
        if kind == 'direct':
            return p - 1, p + 1                              # its 3x3 window
        if kind in ('dconv_up', 'tconv'):
            return 2 * p - 3, 2 * p + 4                      # the 8x8 output block around (2y, 2x)
        if kind in ('wino4', 'wino4_up'):                    # 6x6 input tiles of stride 4: input rows 4t - 1 .. 4t + 4
            t0, t1 = _tiles(p, 4, -1, 4)
            s = 2 if up else 1
            return min(4 * s * t0, s * p - 3 * (s - 1)), max(4 * s * t1 + 4 * s - 1, s * p + 4 * (s - 1))
        t0, t1 = _tiles(p, 2, -1, 1)                          # F(2,2): 3x3 input windows of stride 2 -> 4x4 quads
        return min(4 * t0, 2 * p), max(4 * t1 + 3, 2 * p + 2)
    (r0, r1), (c0, c1) = span(py), span(px)
    far = torch.ones(b, 1, hh, ww, dtype=torch.bool)
    far[0, :, max(r0, 0):min(r1, hh - 1) + 1, max(c0, 0):min(c1, ww - 1) + 1] = False
    return far


def excluded_share(kind, shape):
    far = far_field(kind, shape)
    return 1.0 - far[0].double().mean().item()


def styled(x, style):
    """the kernels' own fp32 product x * style, as float64"""
    return (x * style[:, :, None, None]).double()


def _scaled(z, w_scale, demod, repeat=1):
    dm = demod.detach().cpu().double()
    if repeat > 1:
        dm = dm.repeat_interleave(repeat, dim=1)
    return z * w_scale * dm[:, :, None, None]


def _fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 numbers is exact in float64)"""
    return (a.double() * b.double() + c.double()).float()


def wino4_input_points(x, style, point_split=False):
    """B^T d B of rw_wino4.hip's split kernels in THEIR fp32 operation order, as float64 (n, i, ty, tx, 6, 6): the column
    pass w4_bt2 (point_split: w4_bt2_rows) on d = x style, then w4_bt_row, with the contractions the compiler makes in
    each: which products of 5, and which style products, are fused into the addition or subtraction that consumes them
    (the two column passes differ).  Measured, not derived: of the candidate orders these are the ones the kernels'
    results follow to fp32 accumulation at every k; any other differs at k >= 16 by many times
    that, which is how a recompilation that contracts differently would show up in test_gpu_split_range.py."""
    sv = style[:, :, None, None, None]
    xr = F.pad(x, (1, 1, 1, 1)).unfold(2, 6, 4).unfold(3, 6, 4)
    xr = [xr[..., r, :] for r in range(6)]
    d0, d1, d2, d3, d4, d5 = (xi * sv for xi in xr)
    m5 = torch.tensor(-5.0)
    r, q = _fma(xr[4], sv, -d2), d3 - 4.0 * d1
    if point_split:
        t0, t5 = _fma(xr[4], sv, 4.0 * d0 - 5.0 * d2), _fma(xr[5], sv, 4.0 * d1 - 5.0 * d3)
        p, s = _fma(xr[4], sv, -4.0 * d2), 2.0 * (d3 - d1)
    else:
        t0, t5 = _fma(xr[4], sv, _fma(m5, d2, 4.0 * d0)), _fma(xr[5], sv, _fma(m5, d3, 4.0 * d1))
        p, s = d4 - 4.0 * d2, 2.0 * _fma(-xr[1], sv, d3)
    c = torch.stack([t0, p + q, p - q, r + s, r - s, t5], -2)
    e0, e1, e2, e3, e4, e5 = (c[..., k] for k in range(6))
    p, q, r, s = e4 - 4.0 * e2, e3 - 4.0 * e1, e4 - e2, e3 - e1
    return torch.stack([4.0 * e0 + _fma(m5, e2, e4), p + q, p - q, r + 2.0 * s, r - 2.0 * s,
                        4.0 * e1 + _fma(m5, e3, e5)], -1).double()


def upwino_input_points(x, style):
    """T[v][h] of rw_upwino.hip's split kernel in ITS fp32 operation order, as float64: d = x style, the vertical
    differences, then the horizontal ones, every difference of two style products as ONE fma x sv - d (the compiler's
    contraction; measured: the device's value bit for bit)."""
    sv = style[:, :, None, None]
    b, c, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    raw = [[xp[:, :, r:r + h:2, cc:cc + wd:2] for cc in range(3)] for r in range(3)]
    d = [[raw[r][cc] * sv for cc in range(3)] for r in range(3)]

    def sub(r0, c0, r1, c1):
        return _fma(raw[r0][c0], sv, -d[r1][c1])
    t = [[sub(0, cc, 1, cc) for cc in range(3)], d[1], [sub(2, cc, 1, cc) for cc in range(3)], d[2]]
    T = []
    for v in range(4):
        if v in (1, 3):
            r = (v + 1) // 2
            T.append([sub(r, 0, r, 1), t[v][1], sub(r, 2, r, 1), t[v][2]])
        else:
            T.append([t[v][0] - t[v][1], t[v][1], t[v][2] - t[v][1], t[v][2]])
    return [[e.double() for e in row] for row in T]


def model(kind, x, wt, style, demod, w_scale, k4=None, fault=None, point_split=False):
    """The documented arithmetic: what the split-operand kernel of this kind computes, up to fp32 accumulation.  The
    transformed families round AFTER an fp32 input transform, so theirs is taken in the kernels' own fp32 order
    (wino4_input_points -- point_split: RW_W4H_PS=1 -- and upwino_input_points); everything from the rounding on is float64.
    x_amax is the measured bound, as the wrappers take it with x_amax=None.
    fault: 'headroom' (the input scaled one bit lower than documented) or 'flush' (f16 denormals of the input pair read
    as zero) -- the two smallest ways a kernel can depart from the arithmetic, for test_split_model.py to show that the
    device tests would see them."""
    ev = E._input_exp(E.absmax(x), x, style, TOP[kind] - (fault == 'headroom'))
    fl = fault == 'flush'
    xs, w = styled(x, style), wt[0].double()
    o = w.shape[0]
    if kind == 'direct':
        return _scaled(E._direct16_sums(xs, w, ev, flush=fl), w_scale, demod)
    if kind == 'tconv':
        z = _scaled(E._direct16_sums(xs, w, ev, transposed=True, flush=fl), w_scale, demod)
        return R.upfirdn2d(z, k4.double(), pad=(1, 1))
    if kind == 'wino4':
        return _scaled(E._wino4_sums(xs, w, ev, flush=fl, V=wino4_input_points(x, style, point_split)), w_scale, demod)
    if kind == 'dconv_up':
        return E._pixel_shuffle_phases(_scaled(E._direct16_sums(xs, E._phase_weights(w, k4), ev, flush=fl), w_scale, demod, 4), o)
    if kind == 'wino4_up':
        return E._pixel_shuffle_phases(_scaled(E._wino4_sums(xs, E._phase_weights(w, k4), ev, flush=fl,
                                                                 V=wino4_input_points(x, style, point_split)), w_scale, demod, 4), o)
    assert kind == 'upwino'
    b, _, h, wd = x.shape
    y = torch.zeros(b, o, 2 * h + 1, 2 * wd + 1, dtype=torch.float64)
    E._upwino_quads(xs, w, y, ev, 15 - E._pow2_above(w.abs().max().reshape(1) * 4), flush=fl,
                    T=upwino_input_points(x, style))
    return _scaled(y[:, :, :-1, :-1], w_scale, demod)


def reference(kind, x, wt, style, demod, w_scale, k4=None, dtype=torch.float64):
    """float64 convolution of the same fp32 inputs (the upsampling forms: followed by the float64 blur; the F(2,2) form:
    the quads it writes).  dtype=torch.float32: the same sums accumulated in fp32, a host stand-in for an fp32 kernel."""
    xs, w = styled(x, style).to(dtype), wt[0].to(dtype)
    if kind in ('direct', 'wino4'):
        return _scaled(F.conv2d(xs, w, padding=1), w_scale, demod)
    z = _scaled(F.conv_transpose2d(xs, w.transpose(0, 1), stride=2), w_scale, demod)
    if kind == 'upwino':
        return z[:, :, :-1, :-1]
    return R.upfirdn2d(z, k4.double(), pad=(1, 1))


def far_norm(a, b, far, image=None):
    """|| a - b || over the far field (of one image, or of the batch)"""
    d = (a.double().cpu() - b.double().cpu()) * far
    return (d if image is None else d[image]).norm().item()


def far_rel(a, b, far, image=None):
    den = b.double().cpu() * far
    return far_norm(a, b, far, image) / ((den if image is None else den[image]).norm().item() + 1e-300)


def w_scale_of(shape):
    return 1 / math.sqrt(shape[1] * 9)
