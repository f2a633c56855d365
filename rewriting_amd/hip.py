"""Tensor-level wrappers over the C ABI (include/rewriting_hip.h).

PyTorch is used here for device memory and streams only: every wrapper allocates its output
with torch, passes ``data_ptr()`` and ``torch.cuda.current_stream().cuda_stream`` to the
library and returns the torch tensor -- the ownership rule of SURVEY.md section 8b.  Inputs
must be float32 tensors on a HIP device (the _f16 / _f64 forms of the three L1 ops: float16 /
float64; the _f64 wrappers of the generator's forward at the end of this file: float64); anything
else raises (no CPU path).
"""
import ctypes
from collections import namedtuple as _namedtuple

import torch

from . import _lib
from ._lib import ConvEpilogue, RgbEpilogue, SolveProblem, check

SQRT2 = 2 ** 0.5


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name='tensor', dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('rewriting_amd: %s is on %s; the HIP kernels need a GPU tensor '
                           '(there is no CPU fallback)' % (name, t.device))
    if t.dtype != dtype:
        if dtype == torch.float32:
            raise RuntimeError('rewriting_amd: %s is %s; the C ABI is fp32 only (RW_ERR_UNSUPPORTED, include/rewriting_hip.h: '
                               'the reference\'s pybind modules also dispatch half and double, this library does not) -- '
                               'cast the model / tensor with .float()' % (name, t.dtype))
        raise RuntimeError('rewriting_amd: %s is %s; this entry takes %s (nothing is converted)' % (name, t.dtype, dtype))
    return t.detach().contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _opt(t, name, dtype=torch.float32):
    return None if t is None else _dev(t, name, dtype)


def lib():
    return _lib.load()


def on_device(t):
    """True when ``t`` lives on a HIP device, i.e. when the kernels (and only the kernels) must
    be used for it.  Host code branches on this, never on try/except around a kernel call."""
    return bool(t.is_cuda)


# ------------------------------------------------------------------ L1 native ops
# These three ops take half and double as well as fp32 (include/rewriting_hip.h): fused_bias_act, bias_grad and
# upfirdn2d_major stay fp32 only, and their _f16 / _f64 forms take the same arguments with every tensor in their one
# dtype (bias, refer and the filter taps included) and return their results in it.  The op layer
# (utils/stylegan2/op/) picks the form by the input's dtype.
_ABI_SUFFIX = {torch.float32: 'f32', torch.float16: 'f16', torch.float64: 'f64'}


def _fused_bias_act_as(dtype, x, b, ref, act, grad, alpha, scale):
    x = _dev(x, 'input', dtype)
    b = _dev(b, 'bias', dtype) if b is not None and b.numel() else None
    ref = _dev(ref, 'refer', dtype) if ref is not None and ref.numel() else None
    y = torch.empty_like(x)
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    size_b = b.numel() if b is not None else 1
    entry = getattr(lib(), 'rw_fused_bias_act_' + _ABI_SUFFIX[dtype])
    check(entry(_p(x), _p(b), _p(ref), _p(y), x.numel(), step_b, size_b, int(act), int(grad), float(alpha),
                float(scale), _stream()))
    return y


def _bias_grad_as(dtype, g):
    g = _dev(g, 'grad', dtype)
    outer = g.shape[0]
    channels = g.shape[1] if g.ndim > 1 else 1
    inner = 1
    for d in g.shape[2:]:
        inner *= d
    gb = torch.empty(channels, device=g.device, dtype=g.dtype)
    check(getattr(lib(), 'rw_bias_grad_' + _ABI_SUFFIX[dtype])(_p(g), _p(gb), outer, channels, inner, _stream()))
    return gb


def _upfirdn2d_major_as(dtype, x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    x = _dev(x, 'input', dtype)
    k = _dev(k, 'kernel', dtype)
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    out_h = (in_h * up_y + py0 + py1 - kh + down_y) // down_y
    out_w = (in_w * up_x + px0 + px1 - kw + down_x) // down_x
    y = torch.empty(major, max(out_h, 0), max(out_w, 0), minor, device=x.device, dtype=x.dtype)
    if y.numel():
        check(getattr(lib(), 'rw_upfirdn2d_' + _ABI_SUFFIX[dtype])(
            _p(x), _p(k), _p(y), major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1,
            _stream()))
    return y


def fused_bias_act(x, b, ref, act, grad, alpha, scale):
    """fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
    (utils/stylegan2/op/fused_bias_act.cpp:11-20); empty tensor = absent."""
    return _fused_bias_act_as(torch.float32, x, b, ref, act, grad, alpha, scale)


def fused_bias_act_f16(x, b, ref, act, grad, alpha, scale):
    """fused_bias_act on float16: the fp32 arithmetic on the widened values, rounded to half once."""
    return _fused_bias_act_as(torch.float16, x, b, ref, act, grad, alpha, scale)


def fused_bias_act_f64(x, b, ref, act, grad, alpha, scale):
    """fused_bias_act on float64, alpha and scale in double."""
    return _fused_bias_act_as(torch.float64, x, b, ref, act, grad, alpha, scale)


def bias_grad(g):
    return _bias_grad_as(torch.float32, g)


def bias_grad_f16(g):
    """bias_grad on float16, summed in fp32 as torch.sum sums half."""
    return _bias_grad_as(torch.float16, g)


def bias_grad_f64(g):
    return _bias_grad_as(torch.float64, g)


def upfirdn2d_major(x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """upfirdn2d_op.upfirdn2d on (major, H, W, minor) (utils/stylegan2/op/upfirdn2d.cpp:12-22)."""
    return _upfirdn2d_major_as(torch.float32, x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1)


def upfirdn2d_major_f16(x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """upfirdn2d_major on float16: fp32 accumulation of the widened values, rounded to half once."""
    return _upfirdn2d_major_as(torch.float16, x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1)


def upfirdn2d_major_f64(x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    return _upfirdn2d_major_as(torch.float64, x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1)


# ------------------------------------------------------------------ generator pieces
# The glue ops run in float32 and in float64 (the _f64 names at the end of this file): one body per op takes the dtype,
# which every tensor operand must have -- nothing is converted -- as the three L1 ops above do.
def _entry(op, dtype):
    return getattr(lib(), 'rw_%s_%s' % (op, _ABI_SUFFIX[dtype]))


def _pixel_norm_as(dtype, x, eps):
    x = _dev(x, 'latent', dtype)
    y = torch.empty_like(x)
    check(_entry('pixel_norm', dtype)(_p(x), _p(y), x.shape[0], x.shape[1], float(eps), _stream()))
    return y


def _equal_linear_as(dtype, x, weight, bias, w_scale, b_scale, act, alpha, act_scale):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != dtype:
        _dev(x, 'input', dtype)                 # raises
    x = x.detach()
    if x.ndim != 2 or x.stride(1) != 1:
        x = x.reshape(x.shape[0], -1).contiguous()
    weight = _dev(weight, 'weight', dtype)
    bias = _opt(bias, 'bias', dtype)
    batch, in_dim = x.shape
    out_dim = weight.shape[0]
    if weight.shape[1] != in_dim:
        raise ValueError('weight is %s, the input has %d features' % (tuple(weight.shape), in_dim))
    y = torch.empty(batch, out_dim, device=x.device, dtype=dtype)
    x_stride = x.stride(0) if batch > 1 else in_dim
    check(_entry('equal_linear', dtype)(_p(x), _p(weight), _p(bias), _p(y), batch, in_dim, out_dim,
                                        max(x_stride, in_dim), float(w_scale), float(b_scale), int(bool(act)),
                                        float(alpha), float(act_scale), _stream()))
    return y


def _adjust_latent_as(dtype, w, avg, n_latent, psi):
    w = _dev(w, 'latent', dtype)
    avg = _opt(avg, 'latent_avg', dtype)
    out = torch.empty(w.shape[0], n_latent, w.shape[1], device=w.device, dtype=dtype)
    check(_entry('adjust_latent', dtype)(_p(w), _p(avg), _p(out), w.shape[0], n_latent, w.shape[1], float(psi),
                                         _stream()))
    return out


def _style_mul_as(dtype, x, style):
    x = _dev(x, 'fmap', dtype)
    style = _dev(style, 'style', dtype)
    b, c, h, w = x.shape
    if tuple(style.shape) != (b, c):
        raise ValueError('style must be batch x channels')
    y = torch.empty_like(x)
    check(_entry('style_mul', dtype)(_p(x), _p(style), _p(y), b, c, h * w, _stream()))
    return y


def _weight_sqsum_as(dtype, weight, w_scale):
    weight = _dev(weight, 'weight', dtype)
    o, i = weight.shape[-4], weight.shape[-3]
    taps = weight.shape[-1] * weight.shape[-2]
    wsq = torch.empty(o, i, device=weight.device, dtype=dtype)
    check(_entry('weight_sqsum', dtype)(_p(weight), _p(wsq), o, i, taps, float(w_scale), _stream()))
    return wsq


def _demod_as(dtype, wsq, style, eps):
    wsq = _dev(wsq, 'wsq', dtype)
    style = _dev(style, 'style', dtype)
    b = style.shape[0]
    o, i = wsq.shape
    if style.shape[1] != i:
        raise ValueError('style must be batch x in_ch')
    out = torch.empty(b, o, device=wsq.device, dtype=dtype)
    check(_entry('demod', dtype)(_p(wsq), _p(style), _p(out), b, o, i, float(eps), _stream()))
    return out


def _noise_add_as(dtype, x, noise, noise_w):
    x = _dev(x, 'fmap', dtype)
    noise = _dev(noise, 'noise', dtype)
    noise_w = _dev(noise_w, 'noise weight', dtype)
    b, c, h, w = x.shape
    if noise.numel() != b * h * w:
        raise ValueError('noise must be batch x (height * width)')
    y = torch.empty_like(x)
    check(_entry('noise_add', dtype)(_p(x), _p(noise), _p(noise_w), _p(y), b, c, h * w, _stream()))
    return y


def _to_rgb_as(dtype, x, weight, style, bias, skip, w_scale):
    x = _dev(x, 'fmap', dtype)
    weight = _dev(weight, 'rgb weight', dtype)
    style = _dev(style, 'style', dtype)
    bias = _opt(bias, 'bias', dtype)
    skip = _opt(skip, 'skip', dtype)
    b, c, h, w = x.shape
    if weight.numel() != 3 * c or tuple(style.shape) != (b, c):
        raise ValueError('rgb weight / style shapes')
    if skip is not None and tuple(skip.shape) != (b, 3, h, w):
        raise ValueError('skip shape')
    y = torch.empty(b, 3, h, w, device=x.device, dtype=dtype)
    check(_entry('to_rgb', dtype)(_p(x), _p(weight), _p(style), _p(bias), _p(skip), _p(y), b, c, h * w, float(w_scale),
                                  _stream()))
    return y


def pixel_norm(x, eps=1e-8):
    return _pixel_norm_as(torch.float32, x, eps)


def equal_linear(x, weight, bias, w_scale, b_scale, act=False, alpha=0.2, act_scale=SQRT2):
    """x may be a strided row view (latent[:, index]): last dim contiguous."""
    return _equal_linear_as(torch.float32, x, weight, bias, w_scale, b_scale, act, alpha, act_scale)


def adjust_latent(w, avg, n_latent, psi):
    return _adjust_latent_as(torch.float32, w, avg, n_latent, psi)


def style_mul(x, style):
    return _style_mul_as(torch.float32, x, style)


def weight_sqsum(weight, w_scale):
    return _weight_sqsum_as(torch.float32, weight, w_scale)


def demod(wsq, style, eps=1e-8):
    return _demod_as(torch.float32, wsq, style, eps)


def noise_add(x, noise, noise_w):
    return _noise_add_as(torch.float32, x, noise, noise_w)


def to_rgb(x, weight, style, bias, skip, w_scale):
    return _to_rgb_as(torch.float32, x, weight, style, bias, skip, w_scale)


def blur_noise_act(x, k4, noise, noise_w, bias, post_scale=None, y_amax=None):
    """Blur(pad 1,1) + noise + bias + leaky ReLU of an upsampling layer in one pass; post_scale (B x C, optional):
    a factor on the result -- the style of the convolution that consumes it; y_amax (hip.new_bound(result elements),
    optional) receives the bound of the result."""
    x = _dev(x, 'fmap')
    k4 = _dev(k4, 'blur kernel')
    noise = _opt(noise, 'noise')
    noise_w = _opt(noise_w, 'noise weight')
    bias = _opt(bias, 'bias')
    b, c, ih, iw = x.shape
    y = torch.empty(b, c, ih - 1, iw - 1, device=x.device, dtype=x.dtype)
    post_scale = _post_scale(post_scale, b, c, 'channels')
    y_amax = _amax_out(y_amax, y.numel())
    check(lib().rw_blur_noise_act_amax_f32(_p(x), _p(k4), _p(noise), _p(noise_w), _p(bias), _p(post_scale), _p(y),
                                           b, c, ih - 1, iw - 1, _p(y_amax), _stream()))
    return y


# A ToRGB's skip that is still the running image one level down: `image` (B, 3, H / 2, W / 2) and the 4 x 4 FIR `fir` that
# Upsample would run over it (up 2, pads 2 / 1).  rgb_combine and conv3x3_wino4_to_rgb take it in the place of the
# materialised (B, 3, H, W) skip and upsample it inside their kernel: the same bits, one launch and one image less.
HalfSkip = _namedtuple('HalfSkip', 'image fir')


def _half_skip(skip, b, h, w):
    """The device tensors of a HalfSkip for a B x 3 x h x w image, shapes checked."""
    image, fir = _dev(skip.image, 'rgb skip (half size)'), _dev(skip.fir, 'upsampling kernel')
    if tuple(image.shape) != (b, 3, h // 2, w // 2) or h % 2 or w % 2 or tuple(fir.shape) != (4, 4):
        raise ValueError('half-size rgb skip / kernel shapes')
    return HalfSkip(image, fir)


def rgb_combine(partials, bias, skip):
    """ToRGB from the partial sums a convolution left (conv3x3_direct16_rgb_partial): sum over partials + bias + skip.
    skip: the (B, 3, H, W) image, or a HalfSkip -- upsampled inside the kernel."""
    partials = _dev(partials, 'rgb partial sums')
    bias = _opt(bias, 'rgb bias')
    n, b, c, h, w = partials.shape
    y = torch.empty(b, 3, h, w, device=partials.device, dtype=partials.dtype)
    if isinstance(skip, HalfSkip):
        if c != 3:
            raise ValueError('rgb partial / skip shapes')
        skip = _half_skip(skip, b, h, w)
        check(lib().rw_rgb_combine_up_f32(_p(partials), n, _p(bias), _p(skip.image), _p(skip.fir), _p(y), b, h, w,
                                          _stream()))
        return y
    skip = _opt(skip, 'rgb skip')
    if c != 3 or (skip is not None and tuple(skip.shape) != (b, 3, h, w)):
        raise ValueError('rgb partial / skip shapes')
    check(lib().rw_rgb_combine_f32(_p(partials), n, _p(bias), _p(skip), _p(y), b, h * w, _stream()))
    return y


# ------------------------------------------------------------------ bounds (the split-operand kernels)
BOUND_LANES = 64                # RW_BOUND_LANES of include/rewriting_hip.h


def bound_floats(n_elems):
    """Floats of the y_amax buffer of a producer whose result has n_elems floats (rw_bound_floats)."""
    return int(lib().rw_bound_floats(int(n_elems)))


def new_bound(n_elems, device):
    """An (uninitialised) y_amax buffer for a result of n_elems floats: BOUND_LANES floats that will hold the bound --
    their maximum is >= max |result| -- followed by the producer's per-wave slots ("a BOUND on a map" in
    include/rewriting_hip.h).  The same tensor is the x_amax of the convolution that reads the result.  Nothing in it is
    zeroed, raised with atomics or read back by a later launch through a device scalar: a producer's waves store their
    own slots plainly, one small launch reduces them, the launch boundary publishes the floats like any feature map."""
    return torch.empty(bound_floats(n_elems), device=device, dtype=torch.float32)


def bound_value(bound):
    """The number a bound stands for (host sync; tests and the packing of split weights, never the forward)."""
    return float(bound[:BOUND_LANES].max())


def absmax(x):
    """The bound of x (rw_absmax_f32): the x_amax of the split-operand kernels where the producer of x did not leave one
    behind."""
    x = _dev(x, 'tensor')
    out = new_bound(0, x.device)            # at most 2048 slots
    check(lib().rw_absmax_f32(_p(x), x.numel(), _p(out), _stream()))
    return out


def _amax_in(x, x_amax):
    """The bound a split-operand kernel gets: the caller's, or measured here."""
    if x_amax is None:
        return absmax(x)
    x_amax = _dev(x_amax, 'x_amax')
    if x_amax.numel() < BOUND_LANES:
        raise ValueError('x_amax must be a bound: at least %d floats (hip.new_bound / hip.absmax)' % BOUND_LANES)
    return x_amax


def _amax_out(y_amax, n_elems):
    if y_amax is None:
        return None
    y_amax = _dev(y_amax, 'y_amax')
    if y_amax.numel() < bound_floats(n_elems):
        raise ValueError('y_amax must come from hip.new_bound(%d, device): %d floats' % (n_elems, bound_floats(n_elems)))
    return y_amax


# ------------------------------------------------------------------ packed weights
def pack_conv_weight(weight, mode):
    weight = _dev(weight, 'weight')
    o, i = weight.shape[-4], weight.shape[-3]
    n = lib().rw_packed_conv_weight_elems(o, i, int(mode))
    if n <= 0:
        raise ValueError('bad weight shape / mode')
    wp = torch.empty(n, device=weight.device, dtype=weight.dtype)   # slab order, then fragment order
    check(lib().rw_pack_conv_weight_f32(_p(weight), _p(wp), o, i, int(mode), _stream()))
    return wp


def _check_packed(wp, out_ch, in_ch, mode):
    """(wp on the device, None): the one packing of pack_conv_weight, as _packed returns a form's."""
    wp = _dev(wp, 'packed weight')
    if wp.numel() != lib().rw_packed_conv_weight_elems(out_ch, in_ch, mode):
        raise ValueError('packed weight does not come from pack_conv_weight(%d x %d, mode %d)'
                         % (out_ch, in_ch, mode))
    return wp, None


def pack_conv_weight_bf16x3(weight):
    weight = _dev(weight, 'weight')
    o, i = weight.shape[-4], weight.shape[-3]
    n = lib().rw_packed_conv_weight_bf16x3_bytes(o, i)
    if n <= 0:
        raise ValueError('no bf16x3 packing for a %d x %d weight' % (o, i))
    wb = torch.empty(n // 4, device=weight.device, dtype=torch.float32)     # opaque: bf16 fragments
    check(lib().rw_pack_conv_weight_bf16x3(_p(weight), _p(wb), o, i, _stream()))
    return wb


class _Form(_namedtuple('_Form', 'pack_fn what plain split k4')):
    """What a packed form is.  pack_fn: the public function that makes it; what: its name in "no <what> weight";
    plain: the (rw_packed_*_elems, rw_pack_*) entries of the fp32 packing, split: the (rw_packed_*_elems, rw_*_absmax_f32,
    rw_pack_*) entries of the one in f16 pairs (None: the form has no such packing); k4: the 4x4 FIR is an operand.
    Entries are named, not resolved: they are looked up on lib() at each call."""


_WINO = _Form('pack_conv_weight_wino', 'Winograd packing for a %d x %d',
              ('rw_packed_conv_weight_wino_elems', 'rw_pack_conv_weight_wino_f32'), None, False)
_WINO4 = _Form('pack_conv_weight_wino4', 'F(4x4,3x3) packing for a %d x %d',
               ('rw_packed_conv_weight_wino4_elems', 'rw_pack_conv_weight_wino4_f32'),
               ('rw_packed_conv_weight_wino4h_elems', 'rw_conv_weight_wino4h_absmax_f32', 'rw_pack_conv_weight_wino4h_f32'),
               False)
_UP_WINO = _Form('pack_conv_transpose_weight_wino', 'F(2,2) packing for a %d x %d transposed-conv',
                 ('rw_packed_conv_transpose_wino_elems', 'rw_pack_conv_transpose_wino_f32'),
                 ('rw_packed_conv_transpose_winoh_elems', 'rw_conv_transpose_weight_winoh_absmax_f32',
                  'rw_pack_conv_transpose_winoh_f32'), False)
_UP_BLUR_WINO4 = _Form('pack_conv_transpose_blur_weight_wino4', 'F(4x4,3x3) phase packing for a %d x %d transposed-conv',
                       ('rw_packed_conv_transpose_blur_wino4_elems', 'rw_pack_conv_transpose_blur_weight_wino4_f32'),
                       ('rw_packed_conv_transpose_blur_wino4h_elems', 'rw_conv_transpose_blur_weight_wino4h_absmax_f32',
                        'rw_pack_conv_transpose_blur_weight_wino4h_f32'), True)
_DIRECT16 = _Form('pack_conv_weight_direct16', 'direct-16 packing for a %d x %d', None,
                  ('rw_packed_dconv_weight_elems', 'rw_dconv_weight_absmax_f32', 'rw_pack_dconv_weight_f32'), False)
_UP_BLUR_DIRECT16 = _Form('pack_conv_transpose_blur_weight_direct16',
                          'direct-16 phase packing for a %d x %d transposed-conv', None,
                          ('rw_packed_dconv_transpose_blur_weight_elems', 'rw_dconv_transpose_blur_weight_absmax_f32',
                           'rw_pack_dconv_transpose_blur_weight_f32'), True)


def _k4(k4):
    k4 = _dev(k4, 'blur kernel')
    if tuple(k4.shape) != (4, 4):
        raise ValueError('the blur kernel must be 4 x 4')
    return k4


def _split_scale(measure, *args):
    """(u_scale, u_inv) of a split-operand packing: `measure` (a rw_*_absmax_f32 entry) leaves max |U| as a bound, the
    host reads it -- ONE sync per weight version, never inside a forward whose weights are packed -- and
    rw_split_weight_scale turns it into the power of two that the pack kernel and every convolution launch then get BY
    VALUE."""
    device = args[0].device
    bound = new_bound(0, device)
    check(measure(*[_p(a) if torch.is_tensor(a) else a for a in args], _p(bound), _stream()))
    u_scale = float(lib().rw_split_weight_scale(bound_value(bound)))
    return u_scale, 1.0 / u_scale


def _pack(form, weight, k4=None, split=False):
    """The plain or the split packing of `form` of weight (and k4, where the form takes it): a flat float32 tensor; the
    scale of a split one rides on it as the attribute rw_u_inv."""
    weight = _dev(weight, 'weight')
    operands = (weight, _k4(k4)) if form.k4 else (weight,)
    o, i = weight.shape[-4], weight.shape[-3]
    entries = form.split if split else form.plain
    n = getattr(lib(), entries[0])(o, i)
    if n <= 0:
        raise ValueError('no %s weight' % (form.what % (o, i)))
    packed = torch.empty(n, device=weight.device, dtype=torch.float32)
    scale = ()
    if split:
        u_scale, packed.rw_u_inv = _split_scale(getattr(lib(), entries[1]), *operands, o, i)
        scale = (u_scale,)
    check(getattr(lib(), entries[-1])(*[_p(t) for t in operands], _p(packed), o, i, *scale, _stream()))
    return packed


def _u_inv(packed):
    """1 / u_scale of a split-operand packing: it travels with the tensor the pack function returned."""
    try:
        return float(packed.rw_u_inv)
    except AttributeError:
        raise ValueError('split-operand packed weights must be the tensor a hip.pack_*(split=True) / pack_*_direct16 call '
                         'returned (its scale travels as the attribute rw_u_inv; a copy does not carry it)') from None


def _packed(t, out_ch, in_ch, form):
    """(the packed weight t on the device, 1 / u_scale of a split -- f16 pair -- packing or None for the plain one): the
    two packings of `form` are told apart by their size.  The scale of a split packing rides on the caller's tensor
    (_u_inv), which is why it is read here, before t is replaced by its contiguous self."""
    wp = _dev(t, 'packed weight')
    if form.plain is not None and wp.numel() == getattr(lib(), form.plain[0])(out_ch, in_ch):
        return wp, None
    if form.split is not None and wp.numel() == getattr(lib(), form.split[0])(out_ch, in_ch):
        return wp, _u_inv(t)
    raise ValueError('packed weight does not come from %s(%d x %d)' % (form.pack_fn, out_ch, in_ch))


def pack_conv_weight_wino(weight):
    return _pack(_WINO, weight)


def pack_conv_weight_wino4(weight, split=False):
    """G g G^T of every filter in the fragment order of the F(4x4,3x3) kernels; split=True: every value as the pair
    of f16 numbers the kernels on the 16-bit matrix pipe multiply (rw_pack_conv_weight_wino4h_f32) -- the convolution
    functions tell the two formats apart by their size."""
    return _pack(_WINO4, weight, split=split)


def pack_conv_transpose_weight_wino(weight, split=False):
    """The 25 F(2,2) points of every filter in fragment order; split=True: as pairs of f16 numbers for the kernel on
    the 16-bit matrix pipe (rw_pack_conv_transpose_winoh_f32) -- told apart by size."""
    return _pack(_UP_WINO, weight, split=split)


def pack_conv_transpose_blur_weight_wino4(weight, k4, split=False):
    """F(4x4,3x3) weights of the four output-parity phases of conv_transpose(stride 2) followed by the 4x4 FIR k4;
    split=True: as f16 pairs (pack_conv_weight_wino4)."""
    return _pack(_UP_BLUR_WINO4, weight, k4, split=split)


def pack_conv_weight_direct16(weight):
    """The weights as f16 pairs in the operand order of the direct kernels on the 16-bit matrix pipe
    (rw_pack_dconv_weight_f32)."""
    return _pack(_DIRECT16, weight, split=True)


def pack_conv_transpose_blur_weight_direct16(weight, k4):
    """The four output-parity phases of conv_transpose(stride 2) followed by the 4x4 FIR k4, as f16 pairs in the operand
    order of the direct kernel (rw_pack_dconv_transpose_blur_weight_f32)."""
    return _pack(_UP_BLUR_DIRECT16, weight, k4, split=True)


# ------------------------------------------------------------------ convolutions
def _epilogue(style=None, demod=None, noise=None, noise_w=None, bias=None, act=False):
    keep = [_opt(style, 'style'), _opt(demod, 'demod'), _opt(noise, 'noise'),
            _opt(noise_w, 'noise weight'), _opt(bias, 'bias')]
    ep = ConvEpilogue(_p(keep[0]).value, _p(keep[1]).value, _p(keep[2]).value,
                      _p(keep[3]).value, _p(keep[4]).value, int(bool(act)))
    return ep, keep


def _rgb_epilogue(rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, out, x, out_ch):
    """The ToRGB block of a convolution of x to out_ch channels that writes `out`: (RgbEpilogue, the tensors it
    points at)."""
    keep = [_dev(rgb_weight, 'rgb weight'), _dev(rgb_style, 'rgb style'), _opt(rgb_bias, 'rgb bias'),
            _opt(rgb_skip, 'rgb skip'), out]
    b, _, h, w = x.shape
    if tuple(keep[0].shape) != (3, out_ch) or tuple(keep[1].shape) != (b, out_ch):
        raise ValueError('rgb weight / style shapes')
    if keep[3] is not None and tuple(keep[3].shape) != (b, 3, h, w):
        raise ValueError('rgb skip shape')
    return RgbEpilogue(*[_p(t).value for t in keep], float(rgb_scale)), keep


def _post_scale(post_scale, batch, channels, named='out_ch'):
    post_scale = _opt(post_scale, 'post scale')
    if post_scale is not None and tuple(post_scale.shape) != (batch, channels):
        raise ValueError('post_scale must be batch x %s' % named)
    return post_scale


def _supported(entry, doc):
    """A shape predicate over the library's own rw_*_supported entry."""
    def supported(out_ch, in_ch, height, width):
        return bool(getattr(lib(), entry)(int(out_ch), int(in_ch), int(height), int(width)))
    supported.__doc__ = '%s (%s).' % (doc, entry)
    return supported


def _conv(entries, x, packed, out_ch, w_scale, ep=None, style_demod=None, x_amax=None, **slots):
    """Calls a convolution entry.  Every one takes its arguments in ONE order (include/rewriting_hip.h), the bracketed
    ones only where it has them:

        x, packed, [k4], [y], batch, in_ch, out_ch, h, w, w_scale, ep | (style, demod), [rgb], [impl], [post_scale],
        [u_inv, x_amax], [y_amax], [skip_half, k4], stream

    entries: the entry's name, or (entry for a plain packing, entry for a split one) -- chosen here, once, by the scale
    that `packed` = (tensor, u_inv or None) carries (_packed).  ep / rgb: what _epilogue / _rgb_epilogue returned;
    style_demod: the two tensors of an entry without an epilogue block.  `slots`: the bracketed arguments this entry has
    -- a slot that is given as None is a null pointer, one that is not given is not in the entry's list.  A split
    packing adds u_inv, the bound of x (x_amax, measured here when None) and, where there is a y_amax slot, the buffer
    that receives the bound of slots['y']; a plain one takes none of the three.  slots['half_skip']: a HalfSkip."""
    wp, u_inv = packed
    b, i, h, w = x.shape
    args = [_p(x), _p(wp)] + [_p(slots[s]) for s in ('k4', 'y') if s in slots] + [b, i, out_ch, h, w, float(w_scale)]
    if ep is not None:
        args.append(ctypes.byref(ep[0]))
    else:
        style_demod = [_opt(style_demod[0], 'style'), _opt(style_demod[1], 'demod')]
        args += [_p(t) for t in style_demod]
    if 'rgb' in slots:
        args.append(ctypes.byref(slots['rgb'][0]))
    if 'impl' in slots:
        args.append(int(slots['impl']))
    if 'post_scale' in slots:
        args.append(_p(slots['post_scale']))
    if u_inv is not None:
        x_amax = _amax_in(x, x_amax)
        args += [u_inv, _p(x_amax)]
        if 'y_amax' in slots:
            y_amax = _amax_out(slots['y_amax'], slots['y'].numel())
            args.append(_p(y_amax))
    if 'half_skip' in slots:
        args += [_p(slots['half_skip'].image), _p(slots['half_skip'].fir)]
    entry = entries if isinstance(entries, str) else entries[u_inv is not None]
    check(getattr(lib(), entry)(*args, _stream()))


def _out(x, out_ch, up=1):
    """The (uninitialised) result of a convolution of x to out_ch channels at `up` times its size."""
    b, _, h, w = x.shape
    return torch.empty(b, out_ch, up * h, up * w, device=x.device, dtype=x.dtype)


def _out_transposed(x, out_ch, out):
    """The (2H+1) x (2W+1) map of a transposed convolution of x: the caller's `out`, or a new one."""
    b, _, h, w = x.shape
    y = out if out is not None else torch.empty(b, out_ch, 2 * h + 1, 2 * w + 1, device=x.device, dtype=x.dtype)
    if tuple(y.shape) != (b, out_ch, 2 * h + 1, 2 * w + 1) or not y.is_contiguous():
        raise ValueError('out has the wrong shape')
    return y


def _styled_whole_maps(x, style):
    """(x, style) as the F(2x2) / F(2,2) fp32 kernels take them.  8^2 and 4^2 maps run as whole images per wave (several
    images per workgroup), and the library takes exactly these already multiplied by their style (style == NULL, see the
    header) -- the same product, rounded the same way, one tiny launch earlier."""
    if style is not None and x.shape[2] == x.shape[3] and x.shape[3] in (4, 8):
        return style_mul(x, _dev(style, 'style')), None
    return x, style


def conv3x3(x, wp, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None, bias=None,
            act=False, impl=0):
    x = _dev(x, 'fmap')
    y = _out(x, out_ch)
    _conv('rw_conv3x3_f32', x, _check_packed(wp, out_ch, x.shape[1], 0), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), y=y, impl=impl)
    return y


def to_rgb_fusable(out_ch, in_ch, width):
    """Shapes rw_conv3x3_to_rgb_f32 takes: one wave holds every out-channel of its pixels."""
    return out_ch in (32, 64) and width >= 24 and in_ch % 16 == 0 and in_ch <= 1024


def conv3x3_to_rgb(x, wp, out_ch, w_scale, rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, style=None,
                   demod=None, noise=None, noise_w=None, bias=None, act=False, store_fmap=False):
    """The styled convolution with ToRGB fused into its epilogue: returns (fmap or None, rgb image)."""
    x = _dev(x, 'fmap')
    y, rgb = _out(x, out_ch) if store_fmap else None, _out(x, 3)
    _conv('rw_conv3x3_to_rgb_f32', x, _check_packed(wp, out_ch, x.shape[1], 0), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), y=y,
          rgb=_rgb_epilogue(rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, rgb, x, out_ch))
    return y, rgb


wino_supported = _supported('rw_conv3x3_wino_supported', 'Shapes the Winograd F(2x2,3x3) stride-1 convolution takes')


def conv3x3_wino(x, uf, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None, bias=None, act=False):
    """Stride-1 3x3 convolution by Winograd F(2x2,3x3) in fp32; same arguments and epilogue as conv3x3."""
    x = _dev(x, 'fmap')
    uf = _packed(uf, out_ch, x.shape[1], _WINO)
    y = _out(x, out_ch)
    x, style = _styled_whole_maps(x, style)
    _conv('rw_conv3x3_wino_f32', x, uf, out_ch, w_scale, _epilogue(style, demod, noise, noise_w, bias, act), y=y)
    return y


def conv3x3_wino_to_rgb(x, uf, out_ch, w_scale, rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, style=None,
                        demod=None, noise=None, noise_w=None, bias=None, act=False, store_fmap=False):
    """conv3x3_wino with ToRGB in the epilogue (out_ch == 32): returns (fmap or None, rgb image)."""
    x = _dev(x, 'fmap')
    y, rgb = _out(x, out_ch) if store_fmap else None, _out(x, 3)
    _conv('rw_conv3x3_wino_to_rgb_f32', x, _packed(uf, out_ch, x.shape[1], _WINO), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), y=y,
          rgb=_rgb_epilogue(rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, rgb, x, out_ch))
    return y, rgb


wino4_supported = _supported('rw_conv3x3_wino4_supported', 'Shapes the Winograd F(4x4,3x3) stride-1 convolution takes')


def conv3x3_wino4(x, uf, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None, bias=None, act=False,
                  x_amax=None, y_amax=None):
    """Stride-1 3x3 convolution by Winograd F(4x4,3x3) (~1e-5 relative error per layer: the default of the
    un-hooked whole-generator forward, never used by a hooked or sliced model -- routing.conv_algo); same arguments
    and epilogue as conv3x3.  With weights from pack_conv_weight_wino4(split=True) the products run on the 16-bit
    matrix pipe (exact f16 operand split, fp32 accumulation): x_amax = the bound of x (hip.absmax(x), or the y_amax its
    producer filled; measured here when None), y_amax = hip.new_bound(y.numel(), device), which receives the bound of y."""
    x = _dev(x, 'fmap')
    y = _out(x, out_ch)
    _conv(('rw_conv3x3_wino4_f32', 'rw_conv3x3_wino4h_f32'), x, _packed(uf, out_ch, x.shape[1], _WINO4), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax, y=y, y_amax=y_amax)
    return y


wino4_to_rgb_supported = _supported('rw_conv3x3_wino4_to_rgb_supported', 'Shapes conv3x3_wino4_to_rgb takes: out_ch == 32')


def conv3x3_wino4_to_rgb(x, uf, out_ch, w_scale, rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, style=None,
                         demod=None, noise=None, noise_w=None, bias=None, act=False, x_amax=None):
    """conv3x3_wino4 with ToRGB in the epilogue (out_ch == 32): returns (None, rgb image); the feature map is not
    written.  Split weights and x_amax as in conv3x3_wino4.  rgb_skip: the (B, 3, H, W) image, or a HalfSkip -- upsampled
    in the epilogue."""
    x = _dev(x, 'fmap')
    rgb = _out(x, 3)
    entries, up = ('rw_conv3x3_wino4_to_rgb_f32', 'rw_conv3x3_wino4h_to_rgb_f32'), {}
    if isinstance(rgb_skip, HalfSkip):
        entries = ('rw_conv3x3_wino4_to_rgb_up_f32', 'rw_conv3x3_wino4h_to_rgb_up_f32')
        up, rgb_skip = dict(half_skip=_half_skip(rgb_skip, x.shape[0], x.shape[2], x.shape[3])), None
    _conv(entries, x, _packed(uf, out_ch, x.shape[1], _WINO4),
          out_ch, w_scale, _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax,
          rgb=_rgb_epilogue(rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, rgb, x, out_ch), **up)
    return None, rgb


def bf16x6_supported(out_ch, in_ch, width):
    """Shapes the opt-in split-precision convolution takes (rw_conv3x3_bf16x6_f32)."""
    return width >= 24 and in_ch % 16 == 0 and in_ch <= 1024 and out_ch % 64 == 0


def conv3x3_bf16x6(x, wb, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None, bias=None,
                   act=False):
    """Opt-in: the stride-1 convolution on the bf16 matrix pipe with exact three-way operand splits
    (six piece products, fp32 accumulation); same arguments and epilogue as conv3x3."""
    x = _dev(x, 'fmap')
    wb = _dev(wb, 'packed weight')
    if wb.numel() * 4 != lib().rw_packed_conv_weight_bf16x3_bytes(out_ch, x.shape[1]):
        raise ValueError('packed weight does not come from pack_conv_weight_bf16x3(%d x %d)' % (out_ch, x.shape[1]))
    y = _out(x, out_ch)
    _conv('rw_conv3x3_bf16x6_f32', x, (wb, None), out_ch, w_scale, _epilogue(style, demod, noise, noise_w, bias, act), y=y)
    return y


def up_halo_applicable(out_ch, in_ch, width):
    """Shapes conv_transpose3x3s2 runs on the halo-tile kernel (halo_applicable() in rw_conv.hip)."""
    return (in_ch % 16 == 0 and in_ch <= 1024 and out_ch % 32 == 0
            and (width >= 24 or 9 <= width <= 16 or (5 <= width <= 8 and out_ch % 128 == 0)))


def up_strips_applicable(out_ch, in_ch):
    """Channel counts conv_transpose3x3s2(impl=8) -- the border row and column of the (2H+1) x (2W+1) map alone -- takes."""
    return in_ch % 16 == 0 and in_ch <= 1024 and out_ch % 32 == 0


def conv_transpose3x3s2(x, wp, out_ch, w_scale, style=None, demod=None, impl=0, out=None):
    x = _dev(x, 'fmap')
    y = _out_transposed(x, out_ch, out)
    _conv('rw_conv_transpose3x3s2_f32', x, _check_packed(wp, out_ch, x.shape[1], 1), out_ch, w_scale,
          _epilogue(style, demod), y=y, impl=impl)
    return y


conv_transpose_wino_supported = _supported('rw_conv_transpose3x3s2_wino_supported', 'Shapes the F(2,2) transposed convolution takes')


conv_transpose_wino_split_supported = _supported('rw_conv_transpose3x3s2_winoh_supported', 'Shapes the split-operand (16-bit matrix pipe) form of conv_transpose3x3s2_wino takes')


def conv_transpose3x3s2_wino(x, uf, out_ch, w_scale, style=None, demod=None, out=None, x_amax=None):
    """The quads y < H, x < W of conv_transpose3x3s2 by F(2,2) (25 instead of 36 multiplies per 2x2 block of quads);
    output row 2H and column 2W are left to conv_transpose3x3s2(..., impl=8, out=...).  With weights from
    pack_conv_transpose_weight_wino(split=True) the products run on the 16-bit matrix pipe (exact f16 operand split,
    fp32 accumulation; x_amax = the bound of x as in conv3x3_wino4, measured here when None)."""
    x = _dev(x, 'fmap')
    uf = _packed(uf, out_ch, x.shape[1], _UP_WINO)
    y = _out_transposed(x, out_ch, out)
    if uf[1] is None:                           # the split kernel takes no 8^2 / 4^2 maps
        x, style = _styled_whole_maps(x, style)
    _conv(('rw_conv_transpose3x3s2_wino_f32', 'rw_conv_transpose3x3s2_winoh_f32'), x, uf, out_ch, w_scale,
          style_demod=(style, demod), x_amax=x_amax, y=y)
    return y


conv_transpose_blur_wino4_supported = _supported('rw_conv_transpose_blur_wino4_supported', 'Shapes the one-pass upsampling StyledConv takes')


def conv_transpose3x3s2_blur_wino4(x, uf, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None,
                                   bias=None, act=False, post_scale=None, x_amax=None, y_amax=None):
    """conv_transpose3x3s2 -> blur(pad 1,1) -> noise -> bias + leaky ReLU in one pass: (B,Cin,H,W) -> (B,Cout,2H,2W),
    the four output-parity phases as virtual channels of the F(4x4,3x3) kernel (its error class: image generation).
    Split weights, x_amax and y_amax (max |y|, post_scale included) as in conv3x3_wino4."""
    x = _dev(x, 'fmap')
    y = _out(x, out_ch, up=2)
    _conv(('rw_conv_transpose3x3s2_blur_wino4_f32', 'rw_conv_transpose3x3s2_blur_wino4h_f32'), x,
          _packed(uf, out_ch, x.shape[1], _UP_BLUR_WINO4), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax, y=y,
          post_scale=_post_scale(post_scale, x.shape[0], out_ch), y_amax=y_amax)
    return y


dconv_supported = _supported('rw_dconv3x3_supported', 'Shapes conv3x3_direct16 takes')


dconv_to_rgb_supported = _supported('rw_dconv3x3_to_rgb_supported', 'Shapes conv3x3_direct16_to_rgb takes')


dconv_transpose_blur_supported = _supported('rw_dconv_transpose_blur_supported', 'Shapes conv_transpose3x3s2_blur_direct16 takes')


def conv3x3_direct16(x, wp, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None, bias=None, act=False,
                     x_amax=None, y_amax=None):
    """Stride-1 3x3 convolution as a direct sum on the 16-bit matrix pipe (exact f16 operand split, fp32 accumulation:
    rw_dconv3x3_f32); arguments, epilogue, x_amax and y_amax as conv3x3_wino4 with split weights."""
    x = _dev(x, 'fmap')
    y = _out(x, out_ch)
    _conv('rw_dconv3x3_f32', x, _packed(wp, out_ch, x.shape[1], _DIRECT16), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax, y=y, y_amax=y_amax)
    return y


def conv3x3_direct16_rgb_partial(x, wp, out_ch, w_scale, rgb_weight, rgb_style, rgb_scale, style=None, demod=None, noise=None,
                                 noise_w=None, bias=None, act=False, x_amax=None, y_amax=None):
    """conv3x3_direct16 that also leaves the channel sums of the ToRGB which reads its result (rw_dconv3x3_rgb_partial_f32):
    returns (feature map, partial images (out_ch / 32, B, 3, H, W)); rgb_combine() turns the partials into the image."""
    x = _dev(x, 'fmap')
    n_part = lib().rw_dconv3x3_rgb_partials(out_ch)
    if n_part <= 0:
        raise ValueError('no ToRGB partial sums for %d out-channels' % out_ch)
    y = _out(x, out_ch)
    part = torch.empty(n_part, x.shape[0], 3, x.shape[2], x.shape[3], device=x.device, dtype=x.dtype)
    _conv('rw_dconv3x3_rgb_partial_f32', x, _packed(wp, out_ch, x.shape[1], _DIRECT16), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax, y=y, y_amax=y_amax,
          rgb=_rgb_epilogue(rgb_weight, rgb_style, None, None, rgb_scale, part, x, out_ch))
    return y, part


def conv3x3_direct16_to_rgb(x, wp, out_ch, w_scale, rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, style=None,
                            demod=None, noise=None, noise_w=None, bias=None, act=False, x_amax=None):
    """conv3x3_direct16 with ToRGB in the epilogue (out_ch == 32): returns (None, rgb image)."""
    x = _dev(x, 'fmap')
    rgb = _out(x, 3)
    _conv('rw_dconv3x3_to_rgb_f32', x, _packed(wp, out_ch, x.shape[1], _DIRECT16), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax,
          rgb=_rgb_epilogue(rgb_weight, rgb_style, rgb_bias, rgb_skip, rgb_scale, rgb, x, out_ch))
    return None, rgb


def conv_transpose3x3s2_blur_direct16(x, wp, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None,
                                      bias=None, act=False, post_scale=None, x_amax=None, y_amax=None):
    """conv_transpose3x3s2 -> blur(pad 1,1) -> noise -> bias + leaky ReLU in one pass as a direct sum on the 16-bit matrix
    pipe: (B,Cin,H,W) -> (B,Cout,2H,2W); arguments as conv_transpose3x3s2_blur_wino4 with split weights."""
    x = _dev(x, 'fmap')
    y = _out(x, out_ch, up=2)
    _conv('rw_dconv_transpose3x3s2_blur_f32', x, _packed(wp, out_ch, x.shape[1], _UP_BLUR_DIRECT16), out_ch, w_scale,
          _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax, y=y,
          post_scale=_post_scale(post_scale, x.shape[0], out_ch), y_amax=y_amax)
    return y


tconv_blur_supported = _supported('rw_tconv_blur_supported', 'Shapes conv_transpose3x3s2_blur_fused takes')


def conv_transpose3x3s2_blur_fused(x, wp, k4, out_ch, w_scale, style=None, demod=None, noise=None, noise_w=None,
                                   bias=None, act=False, post_scale=None, x_amax=None, y_amax=None):
    """conv_transpose3x3s2 -> blur(pad 1,1) -> noise -> bias + leaky ReLU in one pass at the transposed convolution's OWN
    multiply count (rw_tconv_blur_f32: a direct sum on the 16-bit matrix pipe with the exact f16 operand split, the
    (2H+1)^2 map kept in LDS, the FIR read from there): (B,Cin,H,W) -> (B,Cout,2H,2W).  wp = pack_conv_weight_direct16 of
    the layer's weight (the plain packing: nothing is composed with the blur), k4 the 4x4 FIR; the other arguments as
    conv_transpose3x3s2_blur_direct16."""
    x = _dev(x, 'fmap')
    y = _out(x, out_ch, up=2)
    # the scratch of the staged forms (the map as operand words, converted once: include/rewriting_hip.h), registered for
    # this call alone -- the library must never hold a pointer this module has let go of; never during a capture
    nbytes = lib().rw_tconv_stage_bytes(x.shape[0], x.shape[1], out_ch, x.shape[2], x.shape[3])
    staged = nbytes > 0 and not torch.cuda.is_current_stream_capturing()
    if staged:
        ws = _workspace(nbytes, x.device)
        check(lib().rw_tconv_stage_buffer(_stream(), _p(ws), ws.numel()))
    try:
        _conv('rw_tconv_blur_f32', x, _packed(wp, out_ch, x.shape[1], _DIRECT16), out_ch, w_scale,
              _epilogue(style, demod, noise, noise_w, bias, act), x_amax=x_amax, k4=_k4(k4), y=y,
              post_scale=_post_scale(post_scale, x.shape[0], out_ch), y_amax=y_amax)
    finally:
        if staged:
            check(lib().rw_tconv_stage_buffer(_stream(), None, 0))
    return y


# ------------------------------------------------------------------ statistics
_workspaces = {}


def _workspace(nbytes, device):
    """The split-K scratch of the current stream: one per (device, stream), because a launch on a second stream may run
    while the reduction of the first still reads its slabs."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def second_moment_accumulate(mom2, a, nchw=False):
    """mom2 (C,C) += a^T a.  a: (rows, C) row-major, or (B, C, H, W) when nchw.  Any C: the NCHW kernel takes every channel
    count as it lies when H * W is a multiple of 16; other maps are copied to rows, and rows whose C is no multiple of 4
    (the kernel reads float4 along the channels) are zero-padded to the next one and accumulated through a padded scratch,
    whose C x C corner is added to mom2."""
    a = _dev(a, 'sample')
    if not (mom2.is_cuda and mom2.dtype == torch.float32 and mom2.is_contiguous()):
        raise RuntimeError('mom2 must be a contiguous float32 GPU tensor')
    if nchw:
        b, c, h, w = a.shape
        rows, hw, layout = b * h * w, h * w, 1
        if hw % 16:
            a = a.permute(0, 2, 3, 1).reshape(-1, c).contiguous()
            rows, hw, layout = a.shape[0], 0, 0
    else:
        rows, c = a.shape
        hw, layout = 0, 0
    if mom2.shape != (c, c):
        raise RuntimeError('mom2 is %s, the sample has %d channels' % (tuple(mom2.shape), c))
    out = mom2
    if layout == 0 and c % 4:
        a = torch.nn.functional.pad(a, (0, 4 - c % 4))
        out = torch.zeros(a.shape[1], a.shape[1], dtype=torch.float32, device=a.device)
    nbytes = lib().rw_second_moment_workspace_bytes(out.shape[0], rows)
    ws = _workspace(nbytes, a.device)
    check(lib().rw_second_moment_f32(_p(a), _p(out), rows, out.shape[0], hw, layout, _p(ws), _stream()))
    if out is not mom2:
        mom2 += out[:c, :c]
    return mom2


def _channel_reduction(entry, out_rows, a, nchw, square_input):
    a = _dev(a, 'sample')
    if nchw:
        b, c, h, w = a.shape
        rows, hw, layout = b * h * w, h * w, 1
    else:
        rows, c = a.shape
        hw, layout = 0, 0
    out = torch.empty(out_rows, c, device=a.device, dtype=a.dtype)
    check(entry(_p(a), _p(out), rows, c, hw, layout, int(bool(square_input)), _stream()))
    return out


def channel_sums(a, nchw=False, square_input=False):
    """(2, C): the sum and the sum of squares of every channel (of the squared sample when square_input)"""
    return _channel_reduction(lib().rw_channel_sums_f32, 2, a, nchw, square_input)


def channel_moments(a, nchw=False, square_input=False):
    """(3, C): p, sum (v - p), sum (v - p)^2 with p the mean of the channel's first samples -- see rw_channel_moments_f32"""
    return _channel_reduction(lib().rw_channel_moments_f32, 3, a, nchw, square_input)


KEY_RESPONSE_MAX_KEYS = 8       # RW_KEY_RESPONSE_MAX_KEYS of include/rewriting_hip.h


def key_response(acts, keys, want_peak=True):
    """heat (B, K, H, W) = sum_c keys[k][c] * acts[b][c], peak (B, K) = heat's maximum over the pixels (None unless
    want_peak).  acts (B, C, H, W) is read as it lies -- a view that is not contiguous is refused, not copied: it may be
    the resident key maps of rewrite/search.py; keys (K, C) or (C,).  More than KEY_RESPONSE_MAX_KEYS keys run in
    groups of that many; a key's rows do not depend on its group (see the header)."""
    if isinstance(acts, torch.Tensor) and not acts.is_contiguous():
        raise RuntimeError('rewriting_amd: the key map must be contiguous (B, C, H, W); it is read in place')
    acts = _dev(acts, 'key map')
    keys = _dev(keys, 'keys')
    if keys.dim() == 1:
        keys = keys[None]
    if acts.dim() != 4 or keys.dim() != 2 or keys.shape[1] != acts.shape[1] or keys.device != acts.device:
        raise RuntimeError('rewriting_amd: key map %s on %s does not go with keys %s on %s'
                           % (tuple(acts.shape), acts.device, tuple(keys.shape), keys.device))
    b, c, h, w = acts.shape
    heats, peaks = [], []
    for k0 in range(0, keys.shape[0], KEY_RESPONSE_MAX_KEYS):
        group = keys[k0:k0 + KEY_RESPONSE_MAX_KEYS]
        heat = torch.empty(b, group.shape[0], h, w, device=acts.device, dtype=acts.dtype)
        peak = torch.empty(b, group.shape[0], device=acts.device, dtype=acts.dtype) if want_peak else None
        if heat.numel():
            check(lib().rw_key_response_f32(_p(acts), _p(group), _p(heat), _p(peak), b, c, h * w, group.shape[0],
                                            _stream()))
        heats.append(heat)
        peaks.append(peak)
    if len(heats) == 1:
        return heats[0], peaks[0]
    return torch.cat(heats, dim=1), (torch.cat(peaks, dim=1) if want_peak else None)


RENDER_MAX_THICKNESS = 8        # RW_RENDER_MAX_THICKNESS of include/rewriting_hip.h


def _rgb(color):
    """Three colour values as .clamp(0, 255).byte() leaves them, packed r | g << 8 | b << 16."""
    values = [float(v) for v in color]
    if len(values) != 3:
        raise RuntimeError('rewriting_amd: a colour has three components, not %d' % len(values))
    r, g, b = (int(min(max(v, 0.0), 255.0)) if v == v else 0 for v in values)
    return r | g << 8 | b << 16


def _in_place(t, name, dtype=torch.float32, device=None):
    """_dev for an operand that is read where it lies: a view that is not contiguous is refused, not copied, and so is a
    tensor on another device than `device`."""
    if isinstance(t, torch.Tensor) and not t.is_contiguous():
        raise RuntimeError('rewriting_amd: %s must be contiguous; it is read in place' % name)
    t = _dev(t, name, dtype)
    if device is not None and t.device != device:
        raise RuntimeError('rewriting_amd: %s is on %s, the images on %s' % (name, t.device, device))
    return t


def render_bytes(images, activations=None, mask=None, level=None, thickness=1, border_color=None, outside_bright=0.5,
                 inside_color=None):
    """(B, H, W, 3) uint8 on the device: what ImageVisualizer.pytorch_masked_image (utils/imgviz.py) shows for every image
    of images (B, 3, H, W) -- or renormalize.as_image's bytes when neither activations nor mask is given -- in one launch
    of rw_render_bytes_f32.  activations (B, h, w) float32 with a level: inside = bilinear up-sampling > level;
    mask (B, H, W) bool or uint8: inside = non-zero.  The defaults are pytorch_masked_image's (yellow border).  Inputs
    are read in place: a view that is not contiguous, a wrong dtype or device is refused, never copied.  The percentile
    level (activations without level) stays on the host."""
    images = _in_place(images, 'images')
    if images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError('rewriting_amd: images are (B, 3, H, W), not %s' % (tuple(images.shape),))
    b, _, h, w = images.shape
    if activations is not None and mask is not None:
        raise RuntimeError('rewriting_amd: render_bytes takes activations or a mask, not both')
    mode, sel, sh, sw, lvl = 0, None, 0, 0, 0.0
    if activations is not None:
        if level is None:
            raise RuntimeError('rewriting_amd: render_bytes needs a level with activations (the percentile level of '
                               'ImageVisualizer.level_for stays on the host)')
        sel = _in_place(activations, 'activations', device=images.device)
        if sel.dim() != 3 or sel.shape[0] != b:
            raise RuntimeError('rewriting_amd: activations %s do not go with images %s'
                               % (tuple(sel.shape), tuple(images.shape)))
        mode, sh, sw, lvl = 1, sel.shape[1], sel.shape[2], float(level)
    elif mask is not None:
        sel = _in_place(mask, 'mask', torch.bool if getattr(mask, 'dtype', None) == torch.bool else torch.uint8,
                        images.device)
        if tuple(sel.shape) != (b, h, w):
            raise RuntimeError('rewriting_amd: mask %s does not go with images %s'
                               % (tuple(sel.shape), tuple(images.shape)))
        mode, sh, sw = 2, h, w
    border = _rgb([255, 255, 0] if border_color is None else border_color)
    inside = -1 if inside_color is None else _rgb(inside_color)
    out = torch.empty(b, h, w, 3, device=images.device, dtype=torch.uint8)
    if out.numel():
        check(lib().rw_render_bytes_f32(_p(images), _p(sel), _p(out), b, h, w, mode, sh, sw, lvl, int(thickness), border,
                                        inside, float(outside_bright), _stream()))
    return out


def _size(size):
    """(width, height) of a `size` as PIL.Image.resize reads it: two positive integers"""
    import operator
    try:
        width, height = (operator.index(v) for v in size if not isinstance(v, bool))
    except (TypeError, ValueError):              # not a pair, not integers
        width = height = 0
    if width < 1 or height < 1:
        raise RuntimeError('rewriting_amd: size is (width, height), two positive integers as PIL.Image.resize takes '
                           'them, not %r' % (size,))
    return width, height


def resize_bytes(bytes_bhwc, size):
    """(B, size[1], size[0], 3) uint8 on the device: ``PIL.Image.resize(size, resample=BILINEAR)`` of every picture of
    bytes_bhwc (B, H, W, 3) uint8 -- what render_bytes returns, what png_encode takes -- byte for byte, on the current
    stream (rw_resize_bilinear_u8 applies the tables of resample.coefficients: along x, rounded to bytes, then along y).
    `size` is renormalize.as_url's: PIL reads it as (width, height).  size == (W, H) returns the input itself (PIL
    copies; nothing is launched).  The input is read in place: a view that is not contiguous, a wrong dtype or device
    is refused, never copied, and so is a size that is not two positive integers -- all before the library is touched."""
    from . import resample
    ow, oh = _size(size)
    x = _in_place(bytes_bhwc, 'bytes', torch.uint8)
    if x.dim() != 4 or x.shape[3] != 3:
        raise RuntimeError('rewriting_amd: resize_bytes takes bytes (B, H, W, 3), not %s' % (tuple(x.shape),))
    b, h, w, _ = x.shape
    if h < 1 or w < 1 or 3 * max(h * w, h * ow, oh * ow) >= 2 ** 31:
        raise RuntimeError('rewriting_amd: resize_bytes takes pictures of at least 1 x 1 and below 2^31 bytes, before '
                           'and after (RW_ERR_UNSUPPORTED, include/rewriting_hip.h), not %d x %d -> %d x %d'
                           % (h, w, oh, ow))
    if (ow, oh) == (w, h):
        return bytes_bhwc
    out = torch.empty(b, oh, ow, 3, device=x.device, dtype=torch.uint8)
    if b == 0:
        return out
    kx, bounds_x = resample.device_coefficients(w, ow, x.device) if ow != w else (None, None)
    ky, bounds_y = resample.device_coefficients(h, oh, x.device) if oh != h else (None, None)
    scratch = torch.empty(b, h, ow, 3, device=x.device, dtype=torch.uint8) if ow != w and oh != h else None
    check(lib().rw_resize_bilinear_u8(_p(x), _p(kx), _p(bounds_x), _p(ky), _p(bounds_y), _p(scratch), _p(out), b, h, w,
                                      oh, ow, 0 if kx is None else kx.shape[1], 0 if ky is None else ky.shape[1],
                                      _stream()))
    return out


def png_segment_bytes():
    """Stream bytes per deflate block of png_encode (rw_png_segment_bytes)"""
    return int(lib().rw_png_segment_bytes())


def png_encode(bytes_bhwc, timings=None, deferred=False):
    """One PNG file (bytes) per image of bytes_bhwc (B, H, W, 3) uint8 on the device -- what render_bytes returns --
    lossless, 8-bit truecolour: the filters, the histogram, the Huffman coding and the compaction run in rw_png_filter_u8 /
    rw_png_encode_u8 / rw_png_compact_u8, the host builds one code table per image from 256 counts (pngcode) and frames
    the chunks.  Two copies to the host (the counts; the coded bytes with their lengths and Adler sums) and one to the
    device (the tables).  Literals only, no LZ77 matches: photographic content codes like PIL's default, flat images
    cost at least one bit per byte.  The input is read in place: a view that is not contiguous, a wrong dtype or device
    is refused, never copied.  An empty batch gives [].  deferred: return one callable per image that frames its file
    (CRC-32, Adler fold, chunks) when called -- for a pool of writer threads (pngwriter.save_image_set).  timings: a dict
    that receives milliseconds of the stages (filter, host, encode, compact, copy) from HIP events -- it synchronises; for
    benchmarks."""
    import numpy
    from . import pngcode
    x = _in_place(bytes_bhwc, 'bytes', torch.uint8)
    if x.dim() != 4 or x.shape[3] != 3:
        raise RuntimeError('rewriting_amd: png_encode takes bytes (B, H, W, 3), not %s' % (tuple(x.shape),))
    b, h, w, _ = x.shape
    if b == 0:
        return []
    stream_len = h * (1 + 3 * w)
    if h < 1 or w < 1 or stream_len >= 2 ** 31:
        raise RuntimeError('rewriting_amd: png_encode takes images of at least 1 x 1 whose filtered stream H (1 + 3 W) is '
                           'below 2^31 bytes (RW_ERR_UNSUPPORTED, include/rewriting_hip.h), not %d x %d' % (h, w))
    seg, cap, words = png_segment_bytes(), int(lib().rw_png_segment_capacity()), int(lib().rw_png_table_words())
    assert words == pngcode.TABLE_WORDS
    nseg = -(-stream_len // seg)
    dev = x.device
    marks = []

    def mark(name):
        if timings is not None:
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            marks.append((name, event))

    def new(*shape, dtype=torch.int32):
        return torch.empty(*shape, device=dev, dtype=dtype)

    mark('start')
    row_type, stream = new(b, h, dtype=torch.uint8), new(b, nseg * seg, dtype=torch.uint8)
    hist_part, hist, adler = new(b, nseg, 256), new(b, 256), new(b, nseg, 2)
    check(lib().rw_png_filter_u8(_p(x), _p(row_type), _p(stream), _p(hist_part), _p(hist), _p(adler), b, h, w, _stream()))
    mark('filter')
    counts = hist.cpu().numpy().astype(numpy.int64)
    table = numpy.empty((b, words), dtype=numpy.uint32)
    bound = 0
    for i in range(b):
        table[i], lengths = pngcode.code_table(counts[i], nseg)
        bound += pngcode.coded_bytes_bound(counts[i], lengths, int(table[i, 0]), nseg)
    table_dev = torch.from_numpy(table.view(numpy.int32)).to(dev)
    mark('host')
    coded, seg_len = new(b, nseg, cap, dtype=torch.uint8), new(b, nseg)
    check(lib().rw_png_encode_u8(_p(stream), _p(table_dev), _p(coded), _p(seg_len), b, h, w, _stream()))
    mark('encode')
    n = b * nseg
    head_bytes = -(-12 * n // 16) * 16
    packed, offsets = new(head_bytes + bound, dtype=torch.uint8), new(n, dtype=torch.int64)
    check(lib().rw_png_compact_u8(_p(coded), _p(seg_len), _p(adler), _p(offsets), _p(packed),
                                  ctypes.c_void_p(packed.data_ptr() + head_bytes), bound, n, _stream()))
    mark('compact')
    host = packed.cpu().numpy()
    mark('copy')
    if timings is not None:
        torch.cuda.synchronize(dev)
        for (_, before), (name, after) in zip(marks, marks[1:]):
            timings[name] = timings.get(name, 0.0) + before.elapsed_time(after)
    head = host[:12 * n].view('<u4').reshape(b, nseg, 3).astype(numpy.int64)
    if int(head[:, :, 0].sum()) > bound:
        raise RuntimeError('rewriting_amd: png_encode coded %d bytes, the host expected at most %d'
                           % (int(head[:, :, 0].sum()), bound))
    body = memoryview(host)[head_bytes:]
    sizes = [min(seg, stream_len - s * seg) for s in range(nseg)]
    ends = numpy.cumsum(head[:, :, 0].sum(axis=1)).tolist()          # an image's segments lie back to back

    def framer(i):
        parts = list(zip(sizes, head[i, :, 1].tolist(), head[i, :, 2].tolist()))
        middle = body[ends[i - 1] if i else 0:ends[i]]
        return lambda: pngcode.frame(w, h, [middle], pngcode.adler_fold(parts))
    framers = [framer(i) for i in range(b)]
    return framers if deferred else [make() for make in framers]


def _png_stream_of(item, index, h, w, channels):
    """The raw deflate stream of item: item itself, or, if it is a whole PNG file (no deflate stream starts with the PNG
    signature), the stream pngreader.parse finds in it -- refused if the file is of another shape or form"""
    view = memoryview(item).cast('B')
    if bytes(view[:8]) != b'\x89PNG\r\n\x1a\n':
        return view
    from . import pngreader
    try:
        parsed = pngreader.parse(view)
    except ValueError as e:
        raise RuntimeError('rewriting_amd: png_decode: file %d: %s' % (index, e)) from None
    if not isinstance(parsed, pngreader.Parsed) or (parsed.h, parsed.w, parsed.channels) != (h, w, channels):
        raise RuntimeError('rewriting_amd: png_decode: file %d is %s, not the %d x %d x %d of this call'
                           % (index, tuple(parsed)[:3] if isinstance(parsed, pngreader.Parsed) else parsed.form, h, w, channels))
    return parsed.span


def _png_spans(files_or_spans, device):
    """(coded on the device or None, packed host buffer or None, spans (B, 2) int64, device) of png_decode's first argument,
    with its refusals"""
    import numpy
    if isinstance(files_or_spans, tuple) and len(files_or_spans) == 2 and isinstance(files_or_spans[0], torch.Tensor):
        coded = _in_place(files_or_spans[0], 'coded', torch.uint8)
        if coded.dim() != 1:
            raise RuntimeError('rewriting_amd: png_decode takes the coded bytes as a 1-D tensor, not %s' % (tuple(coded.shape),))
        spans = numpy.asarray(files_or_spans[1])
        if spans.size == 0:
            spans = spans.reshape(0, 2)
        if spans.ndim != 2 or spans.shape[1] != 2 or spans.dtype.kind not in 'iu':
            raise RuntimeError('rewriting_amd: png_decode takes spans (B, 2) of integers: offset and length')
        spans = spans.astype(numpy.int64)
        if len(spans) and (spans.min() < 0 or int((spans[:, 0] + spans[:, 1]).max()) > coded.numel()):
            raise RuntimeError('rewriting_amd: png_decode: a span passes the coded buffer of %d bytes' % coded.numel())
        dev, packed = coded.device, None
    else:
        streams = [memoryview(s).cast('B') for s in files_or_spans]
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('rewriting_amd: png_decode decodes on a GPU (there is no CPU fallback), not on %s' % dev)
        offsets, at = [], 0
        for s in streams:
            offsets.append(at)
            at += -(-len(s) // 16) * 16
        spans = numpy.array([[o, len(s)] for o, s in zip(offsets, streams)], dtype=numpy.int64).reshape(-1, 2)
        packed = numpy.zeros(max(at, 16), dtype=numpy.uint8)
        for o, s in zip(offsets, streams):
            packed[o:o + len(s)] = numpy.frombuffer(s, dtype=numpy.uint8)
        coded = None
    return coded, packed, spans, dev


def _png_inflate(coded, packed, spans, dev, expect, mark=lambda name: None):
    """The streams (B, stride) uint8 and status (B, 4) int32, both on the device, behind rw_png_inflate_u8"""
    if coded is None:
        coded = torch.from_numpy(packed).to(dev)
    span_dev = torch.from_numpy(spans).to(dev)               # non-negative int64: the bits of the uint64 the entry reads
    mark('copy')
    b, stride = len(spans), -(-expect // 16) * 16
    stream = torch.empty(b, stride, device=dev, dtype=torch.uint8)
    status = torch.empty(b, 4, device=dev, dtype=torch.int32)
    check(lib().rw_png_inflate_u8(_p(coded), _p(span_dev), _p(stream), stride, expect, _p(status), b, _stream()))
    mark('inflate')
    return stream, status


def png_inflate(files_or_spans, expect, device='cuda'):
    """(streams (B, stride) uint8 on the device, status (B, 4) int64 numpy): rw_png_inflate_u8 alone, for raw deflate
    streams of which `expect` bytes each are expected (row i holds them in its first `expect` bytes; stride is expect
    rounded up to 16).  The arguments and the status are png_decode's."""
    import numpy
    expect = int(expect)
    if expect < 1 or expect >= 2 ** 31:
        raise RuntimeError('rewriting_amd: png_inflate takes streams of 1 to 2^31 - 1 bytes (RW_ERR_UNSUPPORTED, '
                           'include/rewriting_hip.h), not %d' % expect)
    coded, packed, spans, dev = _png_spans(files_or_spans, device)
    if len(spans) == 0:
        return torch.empty(0, -(-expect // 16) * 16, device=dev, dtype=torch.uint8), numpy.zeros((0, 4), dtype=numpy.int64)
    with torch.cuda.device(dev):
        stream, status = _png_inflate(coded, packed, spans, dev, expect)
        return stream, status.cpu().numpy().astype(numpy.int64) & 0xffffffff


PNG_STATUS = ('ok', 'truncated input', 'bad block type', 'stored length mismatch', 'bad code-length set',
              'bad literal/length set', 'bad distance set', 'missing end-of-block', 'invalid symbol',
              'distance too far back', 'more output than expected', 'less output than expected', 'bad filter type')
PNG_MAX_WIDTH = 16384        # rw_png_unfilter_u8 keeps one row of 4 W bytes in LDS


def png_decode(files_or_spans, h, w, channels, device='cuda', timings=None):
    """(bytes (B, h, w, 3) uint8 on the device, status (B, 4) int64 numpy) of B PNG images of one shape class -- h rows of
    w pixels with `channels` in {1, 3, 4} bytes each, 8 bits a sample, not interlaced: rw_png_inflate_u8 (one wave per
    raw deflate stream) and rw_png_unfilter_u8, the way back from png_encode.  Grey comes out in all three channels and
    alpha is dropped, as PIL's convert('RGB') does.  files_or_spans is either

    * a list of raw deflate streams (bytes-like: the IDAT payload without the two bytes of the zlib header and the four
      of the Adler trailer) or of whole PNG files of this shape, in which pngreader.parse finds that stream (the file's
      Adler trailer is then the caller's to compare with the status: pngreader.decode does); they are packed into one host
      buffer, each at a 16-byte boundary, and go to the device in one copy; or
    * a pair (coded, spans): coded a 1-D uint8 tensor that is already on the device, read in place, and spans (B, 2)
      integers on the host: offset and length of every stream inside it.

    status[i] = (code, bytes produced, s1, s2): code 0 is RW_PNG_OK, the others index PNG_STATUS
    (include/rewriting_hip.h); pngcode.adler_fold([(produced, s1, s2)]) is the Adler-32 of what was produced.  The pixels
    of an image whose code is not 0 are zeros.  An empty batch returns an empty tensor; nothing is launched for it.  A
    wrong dtype or device, channels outside {1, 3, 4}, an extent below 1, a stream H (1 + channels W) of 2^31 bytes or
    more and a span that passes the buffer are refused before anything is launched.  timings: a dict that receives
    milliseconds of the stages (copy, inflate, unfilter) from HIP events -- it synchronises; for benchmarks."""
    import numpy
    h, w, channels = int(h), int(w), int(channels)
    if channels not in (1, 3, 4):
        raise RuntimeError('rewriting_amd: png_decode takes 1 (grey), 3 (RGB) or 4 (RGBA) channels of 8 bits '
                           '(RW_ERR_UNSUPPORTED, include/rewriting_hip.h), not %d' % channels)
    expect = h * (1 + channels * w)
    if h < 1 or w < 1 or expect >= 2 ** 31 or w > PNG_MAX_WIDTH:
        raise RuntimeError('rewriting_amd: png_decode takes images of at least 1 x 1, at most %d wide, whose filtered stream '
                           'H (1 + channels W) is below 2^31 bytes (RW_ERR_UNSUPPORTED, include/rewriting_hip.h), not %d x %d'
                           % (PNG_MAX_WIDTH, h, w))
    if not isinstance(files_or_spans, tuple):
        files_or_spans = [_png_stream_of(item, i, h, w, channels) for i, item in enumerate(files_or_spans)]
    coded, packed, spans, dev = _png_spans(files_or_spans, device)
    b = len(spans)
    out = torch.empty(b, h, w, 3, device=dev, dtype=torch.uint8)
    if b == 0:
        return out, numpy.zeros((0, 4), dtype=numpy.int64)
    marks = []

    def mark(name):
        if timings is not None:
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            marks.append((name, event))

    with torch.cuda.device(dev):
        mark('start')
        stream, status = _png_inflate(coded, packed, spans, dev, expect, mark)
        stride = stream.shape[1]
        check(lib().rw_png_unfilter_u8(_p(stream), stride, _p(status), _p(out), b, h, w, channels, _stream()))
        mark('unfilter')
        host = status.cpu().numpy().astype(numpy.int64) & 0xffffffff
        if timings is not None:
            torch.cuda.synchronize(dev)
            for (_, before), (name, after) in zip(marks, marks[1:]):
                timings[name] = timings.get(name, 0.0) + before.elapsed_time(after)
    return out, host


# ------------------------------------------------------------------ solve
def project_weight(w, context, base=None, out=None):
    """out = base + P(w), P = projected_conv (rewrite/ganrewrite.py:806-813).  w (..., O, I, kh, kw)."""
    wc = _dev(w, 'weight')
    context = _dev(context, 'context')
    base = _opt(base, 'base')
    o, i = wc.shape[-4], wc.shape[-3]
    taps = wc.shape[-1] * wc.shape[-2]
    if out is None:
        out = torch.empty_like(wc)
    check(lib().rw_project_weight_f32(_p(wc), _p(context), _p(base), _p(out), o, i, taps,
                                      context.shape[0], 1.0, _stream()))
    return out


def solve_ksplit(out_ch, in_ch, h, w):
    return lib().rw_solve_ksplit(out_ch, in_ch, h, w)


def solve_supported(out_ch, in_ch, h, w, upsample, plain, constrained):
    """True when rw_solve_step_f32 takes this target (h, w: the key crop); never raises."""
    return lib().rw_solve_supported(out_ch, in_ch, h, w, int(bool(upsample)), int(bool(plain)),
                                    int(bool(constrained))) == 1


def solve_scratch_elems(out_ch, in_ch, h, w, upsample):
    """Element counts of the solver's scratch buffers and the split-K factor they are sized for -- both from the
    library, so that rw_solve_problem.ksplit and the buffers cannot disagree."""
    sizes = (ctypes.c_longlong * 6)()
    check(lib().rw_solve_scratch_elems(out_ch, in_ch, h, w, int(bool(upsample)), sizes))
    return dict(zip(('conv', 'wsq', 'gd', 'c2', 'grad', 'ksplit'), (int(v) for v in sizes)))


def solve_run_supported(out_ch, in_ch, h, w, rank, upsample, linear):
    """True when the one-launch solver (rw_solve_run_f32) takes this target."""
    return lib().rw_solve_run_supported(out_ch, in_ch, h, w, int(rank), int(bool(upsample)), int(bool(linear))) == 1


def solve_run_scratch_elems(out_ch, in_ch, h, w, niter):
    """Floats of the scratch rw_solve_run_f32 needs (per-channel loss parts + the streamed crop's copy)."""
    n = lib().rw_solve_run_scratch_elems(int(out_ch), int(in_ch), int(h), int(w), int(niter))
    if n < 0:
        raise ValueError('rw_solve_run_scratch_elems(%d, %d, %d, %d, %d)' % (out_ch, in_ch, h, w, niter))
    return n


def solve_run(problem, it_begin, it_end, niter, piter, low_rank_insert, lpart):
    check(lib().rw_solve_run_f32(ctypes.byref(problem), int(it_begin), int(it_end), int(niter), int(piter),
                                 int(bool(low_rank_insert)), _p(lpart), _stream()))


def solve_step(problem, project):
    check(lib().rw_solve_step_f32(ctypes.byref(problem), int(bool(project)), _stream()))


# ------------------------------------------------------------------ gradients of the styled convolution (autograd path)
def conv_wgrad(g, x, upsample, scale=1.0, gscale=None, xscale=None):
    """dW (out_ch, in_ch, 3, 3) of y = conv(x, W) [stride 1, pad 1] or conv_transpose(x, W) [stride 2] given
    g = dL/dy: scale * sum_{b,p} (g * gscale[b,o]) * (xcol * xscale[b,i]) -- rw_conv_wgrad_f32."""
    g = _dev(g, 'output gradient')
    x = _dev(x, 'fmap')
    b, i, h, w = x.shape
    o = g.shape[1]
    want = (b, o, 2 * h + 1, 2 * w + 1) if upsample else (b, o, h, w)
    if tuple(g.shape) != want:
        raise ValueError('output gradient %s does not belong to an input map %s' % (tuple(g.shape), tuple(x.shape)))
    gscale, xscale = _opt(gscale, 'gscale'), _opt(xscale, 'xscale')
    ks = lib().rw_conv_wgrad_ksplit(b, i, o, h, w, int(bool(upsample)))
    scratch = torch.empty(ks * o * i * 9, device=x.device, dtype=torch.float32)
    dw = torch.empty(o, i, 3, 3, device=x.device, dtype=torch.float32)
    check(lib().rw_conv_wgrad_f32(_p(g), _p(x), _p(gscale), _p(xscale), _p(scratch), _p(dw), b, i, o, h, w,
                                  int(bool(upsample)), float(scale), _stream()))
    return dw


def rowdot(a, b):
    """(rows,) sums of a * b over everything but the leading `a.dim() - 2` ... dimensions: a, b (..., H, W) ->
    (...,) = sum over the last two dimensions (rw_rowdot_f32)."""
    a = _dev(a, 'a')
    b = _dev(b, 'b')
    if a.shape != b.shape or a.dim() < 3:
        raise ValueError('rowdot takes two maps of the same (..., H, W) shape')
    lead = tuple(a.shape[:-2])
    n = a.shape[-1] * a.shape[-2]
    rows = a.numel() // n
    out = torch.empty(rows, device=a.device, dtype=torch.float32)
    check(lib().rw_rowdot_f32(_p(a), _p(b), _p(out), rows, n, _stream()))
    return out.view(lead)


# ------------------------------------------------------------------ gradients of ToRGB (a loss on the image)
def to_rgb_input_grad(g, weight, style, w_scale):
    """d fmap (B, C, H, W) of to_rgb given g = dL/d image (B, 3, H, W): w_scale * style[b, i] * sum_c weight[c, i] g[b, c]
    -- rw_to_rgb_input_grad_f32."""
    g = _dev(g, 'image gradient')
    weight = _dev(weight, 'rgb weight')
    style = _dev(style, 'style')
    b, three, h, w = g.shape
    c = style.shape[1]
    if three != 3 or tuple(weight.shape) != (3, c) or style.shape[0] != b:
        raise ValueError('image gradient / rgb weight / style shapes')
    gx = torch.empty(b, c, h, w, device=g.device, dtype=torch.float32)
    check(lib().rw_to_rgb_input_grad_f32(_p(g), _p(weight), _p(style), _p(gx), b, c, h * w, float(w_scale), _stream()))
    return gx


def to_rgb_weight_sums(g, x):
    """(B, 3, C) sums over the pixels of g[b, c] * x[b, i] for g = dL/d image (B, 3, H, W) and the feature map x
    (B, C, H, W) that to_rgb read: what d weight and d style are made of -- rw_to_rgb_weight_sums_f32 (deterministic)."""
    g = _dev(g, 'image gradient')
    x = _dev(x, 'fmap')
    b, c, h, w = x.shape
    if tuple(g.shape) != (b, 3, h, w):
        raise ValueError('image gradient %s does not belong to a feature map %s' % (tuple(g.shape), tuple(x.shape)))
    n = lib().rw_to_rgb_weight_sums_scratch_elems(b, c, h * w)
    scratch = torch.empty(n, device=x.device, dtype=torch.float32)
    t = torch.empty(b, 3, c, device=x.device, dtype=torch.float32)
    check(lib().rw_to_rgb_weight_sums_f32(_p(g), _p(x), _p(scratch), _p(t), b, c, h * w, _stream()))
    return t


# ------------------------------------------------------------------ the perceptual network (perceptual.py)
CONV_RGB_MAX_OUT = 64           # PC_MAX_OUT of rw_percept.hip: every out-channel's weights sit in LDS


def _fmap4(t, name):
    t = _dev(t, name)
    if t.dim() != 4 or 0 in t.shape:
        raise ValueError('%s must be a non-empty (B, C, H, W) map, not %s' % (name, tuple(t.shape)))
    return t


def bias_relu_pool(x, bias, pool=False, keep=True, out=None):
    """(y, pooled) of y = relu(x + bias[None, :, None, None]) and pooled = max_pool2d(y, 2, 2) in one pass
    (rw_bias_relu_pool_f32).  pool=False: pooled is None; keep=False (with pool): the full-size map is not stored and y
    is None; out: the tensor that receives y -- it may be x itself."""
    x = _fmap4(x, 'fmap')
    bias = _dev(bias, 'bias')
    b, c, h, w = x.shape
    if tuple(bias.shape) != (c,):
        raise ValueError('bias must have one value per channel (%d), not %s' % (c, tuple(bias.shape)))
    if not pool and not keep:
        raise ValueError('bias_relu_pool: nothing to compute (pool=False, keep=False)')
    y = None
    if keep:
        y = torch.empty_like(x) if out is None else _in_place(out, 'out', device=x.device)
        if y.shape != x.shape:
            raise ValueError('out is %s, the map %s' % (tuple(y.shape), tuple(x.shape)))
    pooled = torch.empty(b, c, h // 2, w // 2, device=x.device, dtype=x.dtype) if pool else None
    check(lib().rw_bias_relu_pool_f32(_p(x), _p(bias), _p(y), _p(pooled), b, c, h, w, _stream()))
    return y, pooled


def bias_relu_pool_grad(g, y, pooled=False):
    """d x of bias_relu_pool from the saved y (rw_bias_relu_pool_grad_f32): g is the gradient at y (pooled=False) or at the
    pooled map (pooled=True: routed to the first maximum of every window, where y is positive)."""
    y = _fmap4(y, 'saved activation')
    g = _dev(g, 'output gradient')
    b, c, h, w = y.shape
    want = (b, c, h // 2, w // 2) if pooled else (b, c, h, w)
    if tuple(g.shape) != want or g.device != y.device:
        raise ValueError('output gradient %s on %s does not belong to an activation %s on %s (pooled=%s)'
                         % (tuple(g.shape), g.device, tuple(y.shape), y.device, bool(pooled)))
    gx = torch.empty_like(y)
    if g.numel() == 0:                  # a map below 2 x 2 has no window: nothing flows back
        return gx.zero_()
    check(lib().rw_bias_relu_pool_grad_f32(_p(g), _p(y), _p(gx), b, c, h, w, int(bool(pooled)), _stream()))
    return gx


def _rgb_weight(weight):
    weight = _dev(weight, 'weight')
    o = weight.shape[0] if weight.dim() else 0
    if tuple(weight.shape) != (o, 3, 3, 3) or not 1 <= o <= CONV_RGB_MAX_OUT:
        raise ValueError('the first layer\'s weight must be (out_ch <= %d, 3, 3, 3) as stored, not %s (RW_ERR_UNSUPPORTED, '
                         'include/rewriting_hip.h)' % (CONV_RGB_MAX_OUT, tuple(weight.shape)))
    return weight, o


def conv3x3_rgb(x, weight, bias):
    """relu(F.conv2d(x (B, 3, H, W), weight (out_ch, 3, 3, 3), bias, padding=1)) -- rw_conv3x3_rgb_f32."""
    x = _fmap4(x, 'image')
    weight, o = _rgb_weight(weight)
    bias = _dev(bias, 'bias')
    if x.shape[1] != 3 or tuple(bias.shape) != (o,) or weight.device != x.device or bias.device != x.device:
        raise ValueError('conv3x3_rgb takes an image (B, 3, H, W) and a bias (%d,) on the weight\'s device, not %s / %s'
                         % (o, tuple(x.shape), tuple(bias.shape)))
    b, _, h, w = x.shape
    y = torch.empty(b, o, h, w, device=x.device, dtype=x.dtype)
    check(lib().rw_conv3x3_rgb_f32(_p(x), _p(weight), _p(bias), _p(y), b, o, h, w, _stream()))
    return y


def conv3x3_rgb_input_grad(g, weight):
    """d image (B, 3, H, W) of conv3x3_rgb given g (B, out_ch, H, W), the gradient at its output already masked by the
    ReLU -- rw_conv3x3_rgb_input_grad_f32."""
    g = _fmap4(g, 'output gradient')
    weight, o = _rgb_weight(weight)
    if g.shape[1] != o or weight.device != g.device:
        raise ValueError('output gradient %s does not belong to a weight %s' % (tuple(g.shape), tuple(weight.shape)))
    b, _, h, w = g.shape
    gx = torch.empty(b, 3, h, w, device=g.device, dtype=g.dtype)
    check(lib().rw_conv3x3_rgb_input_grad_f32(_p(g), _p(weight), _p(gx), b, o, h, w, _stream()))
    return gx


# ------------------------------------------------------------------ LPIPS and the masked edit distances (lpips.py, distances.py)
LPIPS_MAX_TAPS = _lib.LPIPS_MAX_TAPS


def _reduce_scratch(batch, hw, device):
    n = lib().rw_lpips_reduce_scratch_elems(batch, hw)
    if n < 0:
        raise ValueError('an image of %d pixels is more than the per-image reduction takes (RW_ERR_UNSUPPORTED, '
                         'include/rewriting_hip.h)' % hw)
    return torch.empty(n, device=device, dtype=torch.float32)


def _lpips_tap_operands(who, f0, f1, lin, gd=None):
    """the operands of lpips_tap (and, with gd, of lpips_tap_grad), read in place: f0 (B, C, H, W), f1 (B or 1, C, H, W), lin (C,)
    and gd (B, H, W) on f0's device"""
    f0 = _fmap4(_in_place(f0, 'tap'), 'tap')
    f1 = _in_place(f1, 'second tap', device=f0.device)
    lin = _in_place(lin, 'lin weight', device=f0.device)
    if gd is not None:
        gd = _in_place(gd, 'distance gradient', device=f0.device)
    b, c, h, w = f0.shape
    if f1.dim() != 4 or tuple(f1.shape[1:]) != (c, h, w) or f1.shape[0] not in (1, b) or tuple(lin.shape) != (c,) \
            or (gd is not None and tuple(gd.shape) != (b, h, w)):
        raise ValueError('%s takes two maps (B, C, H, W) and (B or 1, C, H, W)%s, not %s'
                         % (who, ' and a weight (C,)' if gd is None else ', a weight (C,) and a gradient (B, H, W)',
                            ' / '.join(str(tuple(t.shape)) for t in (f0, f1, lin, gd) if t is not None)))
    return f0, f1, lin, gd


def _lpips_tables(tables, k, size, b, weight, device):
    """(idx, lam, h, w, weight, the weight's batch or 0) of a combine call over k taps: tables of lpips.device_tables for an output
    of size = (H, W), weight (B or 1, 1, H, W) or None, all on `device`"""
    idx = _in_place(tables[0], 'index table', torch.int32, device)
    lam = _in_place(tables[1], 'weight table', device=device)
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or tuple(idx.shape) != (k, 2 * h + 2 * w) or tuple(lam.shape) != (k, h + w):
        raise ValueError('the tables %s / %s do not belong to %d taps and an output of %d x %d'
                         % (tuple(idx.shape), tuple(lam.shape), k, h, w))
    if weight is not None:
        weight = _in_place(weight, 'weight', device=device)
        if weight.dim() != 4 or tuple(weight.shape[1:]) != (1, h, w) or weight.shape[0] not in (1, b):
            raise ValueError('the weight must be (B or 1, 1, H, W) = (%d or 1, 1, %d, %d), not %s' % (b, h, w, tuple(weight.shape)))
    return idx, lam, h, w, weight, weight.shape[0] if weight is not None else 0


def _lpips_maps(struct, tensors):
    """rw_lpips_maps / rw_lpips_grad_maps of the tensors (B, h_k, w_k)"""
    maps = struct()
    for n, t in enumerate(tensors):
        maps.d[n], maps.h[n], maps.w[n] = t.data_ptr(), t.shape[1], t.shape[2]
    maps.n = len(tensors)
    return maps


def _lpips_tap_count(who, n):
    if not 1 <= n <= LPIPS_MAX_TAPS:
        raise ValueError('%s takes 1 .. %d tap maps, not %d (RW_ERR_UNSUPPORTED, include/rewriting_hip.h)' % (who, LPIPS_MAX_TAPS, n))


def lpips_tap(f0, f1, lin):
    """d (B, H, W) of one LPIPS tap (rw_lpips_tap_f32): sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 with the norms
    over the channels of a pixel; f0 (B, C, H, W), f1 (B or 1, C, H, W), lin (C,).  Read in place."""
    f0, f1, lin, _ = _lpips_tap_operands('lpips_tap', f0, f1, lin)
    b, c, h, w = f0.shape
    d = torch.empty(b, h, w, device=f0.device, dtype=torch.float32)
    check(lib().rw_lpips_tap_f32(_p(f0), _p(f1), _p(lin), _p(d), b, f1.shape[0], c, h * w, _stream()))
    return d


def lpips_combine(taps, tables, size, weight=None, want_map=True, want_sums=False):
    """(out (B, 1, H, W) or None, sums (B, 2) or None) of rw_lpips_combine_f32: out = the sum over the tap maps (B, h_k, w_k) of
    their bilinear up-sampling to size = (H, W) with tables = (idx int32 (K, 2H + 2W), lam float32 (K, H + W)) of
    lpips.device_tables; sums[b] = (sum out * weight, sum weight), weight (B or 1, 1, H, W) or None (all ones)."""
    _lpips_tap_count('lpips_combine', len(taps))
    if not (want_map or want_sums):
        raise ValueError('lpips_combine: nothing to compute (want_map=False, want_sums=False)')
    taps = [_in_place(t, 'tap map') for t in taps]
    device = taps[0].device
    b = taps[0].shape[0]
    idx, lam, h, w, weight, weight_batch = _lpips_tables(tables, len(taps), size, b, weight, device)
    for n, t in enumerate(taps):
        if t.dim() != 3 or t.shape[0] != b or 0 in t.shape or t.device != device:
            raise ValueError('tap map %d is %s on %s; every one is (B = %d, h, w) on %s' % (n, tuple(t.shape), t.device, b, device))
    maps = _lpips_maps(_lib.LpipsMaps, taps)
    out = torch.empty(b, 1, h, w, device=device, dtype=torch.float32) if want_map else None
    sums = torch.empty(b, 2, device=device, dtype=torch.float32) if want_sums else None
    scratch = _reduce_scratch(b, h * w, device) if want_sums else None
    check(lib().rw_lpips_combine_f32(ctypes.byref(maps), _p(idx), _p(lam), _p(weight), weight_batch, _p(out), _p(sums),
                                     _p(scratch), b, h, w, _stream()))
    return out, sums


def lpips_tap_grad(f0, f1, lin, gd, acc=None, relu_mask=False, out=None):
    """The adjoint of lpips_tap to f0 (rw_lpips_tap_grad_f32): acc + gd (2 / den0) (lin t - f0 S / (r0 den0)), (B, C, H, W); gd
    (B, H, W) is the gradient at d, acc (B, C, H, W) the gradient that is already there (None: zeros), out the tensor that
    receives the result -- it may be acc.  relu_mask: an element with f0 <= 0 gets exactly acc.  A pixel whose f0 is all zero
    contributes exactly 0.  Read in place."""
    f0, f1, lin, gd = _lpips_tap_operands('lpips_tap_grad', f0, f1, lin, gd)
    b, c, h, w = f0.shape
    if acc is not None:
        acc = _in_place(acc, 'incoming gradient', device=f0.device)
        if acc.shape != f0.shape:
            raise ValueError('the incoming gradient is %s, the tap %s' % (tuple(acc.shape), tuple(f0.shape)))
    if out is None:
        out = torch.empty_like(f0)
    else:
        out = _in_place(out, 'out', device=f0.device)
        if out.shape != f0.shape:
            raise ValueError('out is %s, the tap %s' % (tuple(out.shape), tuple(f0.shape)))
    check(lib().rw_lpips_tap_grad_f32(_p(f0), _p(f1), _p(lin), _p(gd), _p(acc), _p(out), b, f1.shape[0], c, h * w,
                                      int(bool(relu_mask)), _stream()))
    return out


def lpips_combine_grad(tap_sizes, tables, ranges, size, gscale, weight=None):
    """[gd_k (B, h_k, w_k)] of rw_lpips_combine_grad_f32, the adjoint of lpips_combine's ``sum(out * weight)`` to every tap map:
    tap_sizes = ((h_k, w_k), ...), tables as lpips_combine takes them, ranges int32 (2 sum_k (h_k + w_k),) of
    lpips.device_adjoint_tables, size = (H, W), gscale (B,) the gradient at an image's weighted sum, weight (B or 1, 1, H, W)
    or None (all ones)."""
    tap_sizes = [(int(a), int(b)) for a, b in tap_sizes]
    _lpips_tap_count('lpips_combine_grad', len(tap_sizes))
    gscale = _in_place(gscale, 'gradient scale')
    device = gscale.device
    ranges = _in_place(ranges, 'range table', torch.int32, device)
    if gscale.dim() != 1 or gscale.shape[0] < 1:
        raise ValueError('the gradient scale must be (B,), not %s' % (tuple(gscale.shape),))
    b = gscale.shape[0]
    idx, lam, h, w, weight, weight_batch = _lpips_tables(tables, len(tap_sizes), size, b, weight, device)
    if any(a < 1 or c < 1 for a, c in tap_sizes) or tuple(ranges.shape) != (2 * sum(a + c for a, c in tap_sizes),):
        raise ValueError('the range table %s does not belong to taps of %s' % (tuple(ranges.shape), tap_sizes))
    grads = [torch.empty(b, hk, wk, device=device, dtype=torch.float32) for hk, wk in tap_sizes]
    maps = _lpips_maps(_lib.LpipsGradMaps, grads)
    check(lib().rw_lpips_combine_grad_f32(ctypes.byref(maps), _p(idx), _p(lam), _p(ranges), _p(weight), weight_batch, _p(gscale),
                                          b, h, w, _stream()))
    return grads


def masked_l1(a, b, mask):
    """(B, 2): per image (sum_p mask sum_c |a - b|, sum_p mask) for images a, b (B, 3, H, W) and mask (B or 1, H, W) float32 --
    rw_masked_l1_rgb_f32."""
    a = _fmap4(_in_place(a, 'images'), 'images')
    b = _in_place(b, 'second images', device=a.device)
    mask = _in_place(mask, 'mask', device=a.device)
    n, c, h, w = a.shape
    if c != 3 or b.shape != a.shape or mask.dim() != 3 or tuple(mask.shape[1:]) != (h, w) or mask.shape[0] not in (1, n):
        raise ValueError('masked_l1 takes two image batches (B, 3, H, W) and a mask (B or 1, H, W), not %s / %s / %s'
                         % (tuple(a.shape), tuple(b.shape), tuple(mask.shape)))
    sums = torch.empty(n, 2, device=a.device, dtype=torch.float32)
    scratch = _reduce_scratch(n, h * w, a.device)
    check(lib().rw_masked_l1_rgb_f32(_p(a), _p(b), _p(mask), mask.shape[0], _p(sums), _p(scratch), n, h * w, _stream()))
    return sums


__all__ = [n for n in dir() if not n.startswith('_')] + ['SolveProblem', 'ConvEpilogue']


# ------------------------------------------------------------------ the float64 forward
# The generator's forward in double (include/rewriting_hip.h, last section): the same pieces as above on float64
# tensors, module by module -- no packed weights, no epilogues, no routes.  Every tensor operand must be float64
# (nothing is converted); the fp32 wrappers above keep refusing it.  The glue ops are the bodies of "generator pieces"
# above, called with the dtype.
_F64 = torch.float64


def pixel_norm_f64(x, eps=1e-8):
    return _pixel_norm_as(_F64, x, eps)


def equal_linear_f64(x, weight, bias, w_scale, b_scale, act=False, alpha=0.2, act_scale=SQRT2):
    """x may be a strided row view (latent[:, index]): last dim contiguous."""
    return _equal_linear_as(_F64, x, weight, bias, w_scale, b_scale, act, alpha, act_scale)


def adjust_latent_f64(w, avg, n_latent, psi):
    return _adjust_latent_as(_F64, w, avg, n_latent, psi)


def style_mul_f64(x, style):
    return _style_mul_as(_F64, x, style)


def weight_sqsum_f64(weight, w_scale):
    return _weight_sqsum_as(_F64, weight, w_scale)


def demod_f64(wsq, style, eps=1e-8):
    return _demod_as(_F64, wsq, style, eps)


def noise_add_f64(x, noise, noise_w):
    return _noise_add_as(_F64, x, noise, noise_w)


def to_rgb_f64(x, weight, style, bias, skip, w_scale):
    return _to_rgb_as(_F64, x, weight, style, bias, skip, w_scale)


def _conv_f64(entry, up, x, weight, w_scale, style, demod):
    x = _dev(x, 'fmap', _F64)
    weight = _dev(weight, 'weight', _F64)
    style = _opt(style, 'style', _F64)
    demod = _opt(demod, 'demod', _F64)
    b, i, h, w = x.shape
    o = weight.shape[-4]
    if tuple(weight.shape[-4:]) != (o, i, 3, 3) or weight.numel() != o * i * 9:
        raise ValueError('weight must be (out_ch, %d, 3, 3) as stored, it is %s' % (i, tuple(weight.shape)))
    if style is not None and tuple(style.shape) != (b, i):
        raise ValueError('style must be batch x in_ch')
    if demod is not None and tuple(demod.shape) != (b, o):
        raise ValueError('demod must be batch x out_ch')
    y = torch.empty((b, o, 2 * h + 1, 2 * w + 1) if up else (b, o, h, w), device=x.device, dtype=_F64)
    check(getattr(lib(), entry)(_p(x), _p(weight), _p(y), b, i, o, h, w, float(w_scale), _p(style), _p(demod),
                                _stream()))
    return y


def conv3x3_f64(x, weight, w_scale, style=None, demod=None):
    """F.conv2d(x * style, w_scale * weight, padding=1) * demod in double; weight (out_ch, in_ch, 3, 3) as stored."""
    return _conv_f64('rw_conv3x3_f64', False, x, weight, w_scale, style, demod)


def conv_transpose3x3s2_f64(x, weight, w_scale, style=None, demod=None):
    """F.conv_transpose2d(x * style, w_scale * weight^T, stride=2) * demod in double, to (2H+1) x (2W+1)."""
    return _conv_f64('rw_conv_transpose3x3s2_f64', True, x, weight, w_scale, style, demod)


# ------------------------------------------------------------------ the Frechet distance on the device
# rw_frechet.hip: a float64 block one-sided Jacobi eigensolver for symmetric PSD matrices, the f64 GEMM and the final
# sums (include/rewriting_hip.h, last section).  torch allocates, pads, sorts and slices; every sum and every rotation
# is the library's.
JACOBI_BLOCK = 16               # columns per block (8 or 16): the faster of the two on the MI355X, profiles/frechet_distance.json
JACOBI_MAX_SWEEPS = 40


def jacobi_padded_order(n, block=None):
    """The order the kernels run at: a multiple of the block width, at least one block pair."""
    block = JACOBI_BLOCK if block is None else block
    return max(2 * block, -(-n // block) * block)


def _square_f64(t, name):
    """The refusals of the eigensolver and the distance, the device last (so that they read the same on any host)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if t.dim() != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 1:
        raise ValueError('%s must be a square matrix, it is %s' % (name, tuple(t.shape)))
    if t.dtype != torch.float64:
        raise RuntimeError('rewriting_amd: %s is %s; this entry takes torch.float64 (nothing is converted)' % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous (nothing is copied)' % name)
    if not t.is_cuda:
        raise RuntimeError('rewriting_amd: %s is on %s; the HIP kernels need a GPU tensor (there is no CPU fallback)'
                           % (name, t.device))
    return t.detach()


def _padded(s, npad):
    n = s.shape[0]
    g = torch.zeros(npad, npad, dtype=_F64, device=s.device)
    g[:n, :n] = s
    return g


def colnorm_f64(g, mode=0):
    """Norms of the rows of g (mode 0), their squares (1) or their square roots (2)."""
    g = _dev(g, 'matrix', _F64)
    out = torch.empty(g.shape[0], dtype=_F64, device=g.device)
    check(lib().rw_colnorm_f64(_p(g), _p(out), g.shape[0], mode, _stream()))
    return out


def _jacobi_solve(g, vectors, max_sweeps, block):
    """Block Jacobi on the padded array g (rows = columns of G), in place.  Returns (v or None, sweeps); reads two integers
    per sweep and nothing else."""
    npad = g.shape[0]
    blocks = npad // block
    m = blocks + (blocks & 1)
    v = torch.eye(npad, dtype=_F64, device=g.device) if vectors else None
    norms_sq = colnorm_f64(g, 1)
    slots = torch.empty((m - 1) * (m // 2), dtype=torch.int32, device=g.device)
    out = torch.empty(2, dtype=torch.int64, device=g.device)
    step_fn, stream = lib().rw_jacobi_step_f64, _stream()
    for sweep in range(1, max_sweeps + 1):
        for step in range(m - 1):
            check(step_fn(_p(g), _p(v), npad, block, step, _p(norms_sq),
                          ctypes.c_void_p(slots.data_ptr() + 4 * step * (m // 2)), stream))
        check(lib().rw_jacobi_count_i32(_p(slots), slots.numel(), _p(out), stream))
        count, bad = out.tolist()
        if bad:
            raise ValueError('the matrix holds a non-finite value')
        if count == 0:
            return v, sweep
    raise RuntimeError('rewriting_amd: the Jacobi iteration did not converge in %d sweeps (%d rotations in the last one)'
                       % (max_sweeps, count))


def eigh_psd_f64(S, vectors=True, max_sweeps=JACOBI_MAX_SWEEPS, block=None):
    """(eigenvalues ascending, eigenvectors as columns or None, sweeps) of a symmetric PSD float64 matrix on the device by
    the block one-sided Jacobi of rw_frechet.hip.  Refuses non-square, non-float64, non-contiguous, host and non-finite
    input; raises when ``max_sweeps`` is reached without convergence."""
    S = _square_f64(S, 'S')
    block = JACOBI_BLOCK if block is None else block
    n = S.shape[0]
    npad = jacobi_padded_order(n, block)
    g = _padded(S, npad)
    v, sweeps = _jacobi_solve(g, vectors, max_sweeps, block)
    lam = colnorm_f64(g, 0)
    if not vectors:
        return torch.sort(lam).values[npad - n:], None, sweeps      # the padding's columns stay exact zeros
    keep = ~(v[:, n:] != 0).any(1)                                   # ... and their vectors unit vectors past row n
    lam, v = lam[keep], v[keep, :n]
    lam, order = torch.sort(lam)
    return lam, v[order].t(), sweeps


def gemm_f64(a, b, trans_a=False, trans_b=False, row_scale=None, col_scale=None):
    """diag(row_scale) op(a) op(b) diag(col_scale) in float64."""
    a, b = _dev(a, 'a', _F64), _dev(b, 'b', _F64)
    m, k = (a.shape[1], a.shape[0]) if trans_a else a.shape
    k2, n = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if a.dim() != 2 or b.dim() != 2 or k != k2:
        raise ValueError('shapes do not multiply: op(a) %d x %d, op(b) %d x %d' % (m, k, k2, n))
    row_scale, col_scale = _opt(row_scale, 'row_scale', _F64), _opt(col_scale, 'col_scale', _F64)
    if (row_scale is not None and row_scale.numel() != m) or (col_scale is not None and col_scale.numel() != n):
        raise ValueError('row_scale must have %d entries and col_scale %d' % (m, n))
    c = torch.empty(m, n, dtype=_F64, device=a.device)
    check(lib().rw_gemm_f64(_p(a), _p(b), _p(c), m, n, k, int(trans_a), int(trans_b), _p(row_scale), _p(col_scale), _stream()))
    return c


def frechet_distance_f64(mu1, sigma1, mu2, sigma2, max_sweeps=JACOBI_MAX_SWEEPS, block=None, parts=None):
    """d^2 = |mu1 - mu2|^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)) of float64 device tensors as a Python float: eigh(S1) -> T =
    diag(sqrt(lambda)) V^T S2 -> B = T V diag(sqrt(lambda)) -> eigenvalues of B -> the sums, one copy to the host at the
    end.  ``parts``: a dict that receives the sweeps of both solves and the five sums."""
    sigma1, sigma2 = _square_f64(sigma1, 'sigma1'), _square_f64(sigma2, 'sigma2')
    mu1, mu2 = _dev(mu1, 'mu1', _F64), _dev(mu2, 'mu2', _F64)
    n = sigma1.shape[0]
    if sigma2.shape != sigma1.shape or mu1.shape != (n,) or mu2.shape != (n,):
        raise ValueError('mu must be (%d,) and sigma (%d, %d) for both sets' % (n, n, n))
    block = JACOBI_BLOCK if block is None else block
    npad = jacobi_padded_order(n, block)
    g = _padded(sigma1, npad)
    v, sweeps1 = _jacobi_solve(g, True, max_sweeps, block)
    root = colnorm_f64(g, 2)
    t = gemm_f64(v, _padded(sigma2, npad), row_scale=root)
    bmat = gemm_f64(t, v, trans_b=True, col_scale=root)
    _, sweeps2 = _jacobi_solve(bmat, False, max_sweeps, block)
    ev = colnorm_f64(bmat, 0)
    out = torch.empty(5, dtype=_F64, device=g.device)
    check(lib().rw_frechet_finish_f64(_p(mu1), _p(mu2), _p(sigma1), _p(sigma2), _p(ev), n, npad, _p(out), _stream()))
    sums = out.tolist()
    if parts is not None:
        parts.update(sweeps=(sweeps1, sweeps2), order=npad, block=block,
                     sums=dict(zip(('d2', 'dmu2', 'tr1', 'tr2', 'tr_sqrt'), sums)))
    return sums[0]


# ------------------------------------------------------------------ the Inception-v3 pool3 features (inception.py)
CONV2D_MAX_TAP = 7              # IC_MAX_TAP of rw_inception.hip
POOL_MODES = {'max_s2': 0, 'avg': 1, 'max_s1': 2}


def _pair(v, name):
    """(a, b) of an int or a pair of ints."""
    if isinstance(v, int):
        return v, v
    if len(v) != 2 or not all(isinstance(e, int) for e in v):
        raise ValueError('%s must be an int or a pair of ints, not %r' % (name, v))
    return int(v[0]), int(v[1])


def _slice_out(out, c_off, b, ch, oh, ow, like):
    """(the tensor written, c_off, c_total) of a result of `ch` channels: a new (b, ch, oh, ow) tensor, or the channels
    [c_off, c_off + ch) of ``out`` (b, c_total, oh, ow), which is written where it lies."""
    if out is None:
        if c_off:
            raise ValueError('c_off=%d needs the tensor it counts in: pass out=' % c_off)
        return torch.empty(b, ch, oh, ow, device=like.device, dtype=torch.float32), 0, ch
    out = _in_place(out, 'out', device=like.device)
    if out.dim() != 4 or out.shape[0] != b or tuple(out.shape[2:]) != (oh, ow):
        raise ValueError('out must be (%d, c_total, %d, %d), not %s' % (b, oh, ow, tuple(out.shape)))
    if not isinstance(c_off, int) or c_off < 0 or c_off + ch > out.shape[1]:
        raise ValueError('c_off=%r: channels [c_off, c_off + %d) do not lie in out\'s %d' % (c_off, ch, out.shape[1]))
    return out, c_off, out.shape[1]


def conv2d_out_size(h, w, kernel, stride, padding):
    """(oh, ow) of conv2d, after the checks rw_conv2d_f32 makes of the kernel, the stride and the padding."""
    (kh, kw), (ph, pw) = kernel, padding
    if not (1 <= kh <= CONV2D_MAX_TAP and 1 <= kw <= CONV2D_MAX_TAP):
        raise ValueError('the kernel must be within %d x %d, not %d x %d (RW_ERR_UNSUPPORTED, include/rewriting_hip.h)'
                         % (CONV2D_MAX_TAP, CONV2D_MAX_TAP, kh, kw))
    if stride not in (1, 2):
        raise ValueError('stride must be 1 or 2, not %r' % (stride,))
    if not (0 <= ph < kh and 0 <= pw < kw):
        raise ValueError('padding must be below the kernel (%d, %d), not (%d, %d)' % (kh, kw, ph, pw))
    if h + 2 * ph < kh or w + 2 * pw < kw:
        raise ValueError('fmap of %d x %d is smaller than the kernel %d x %d with padding (%d, %d)' % (h, w, kh, kw, ph, pw))
    return (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1


def conv2d_pack_weight(weight):
    """The packed form of a (out_ch, in_ch, kh, kw) weight that ``conv2d`` reads (rw_pack_conv2d_weight_f32); once per
    weight version."""
    weight = _dev(weight, 'weight')
    if weight.dim() != 4 or 0 in weight.shape:
        raise ValueError('weight must be a non-empty (out_ch, in_ch, kh, kw), not %s' % (tuple(weight.shape),))
    o, i, kh, kw = weight.shape
    n = lib().rw_conv2d_packed_weight_elems(o, i, kh, kw)
    if n <= 0:
        raise ValueError('weight %s: the kernel must be within %d x %d (RW_ERR_UNSUPPORTED, include/rewriting_hip.h)'
                         % (tuple(weight.shape), CONV2D_MAX_TAP, CONV2D_MAX_TAP))
    wp = torch.empty(n, device=weight.device, dtype=torch.float32)
    check(lib().rw_pack_conv2d_weight_f32(_p(weight), _p(wp), o, i, kh, kw, _stream()))
    return wp


def _conv2d_operands(x, wp, weight_shape, bias, stride, padding):
    """(x, wp, bias, the shape arguments of rw_conv2d_f32 from batch to pw, (oh, ow)) after the checks conv2d and conv2d_add
    share."""
    x = _fmap4(x, 'fmap')
    wp = _dev(wp, 'packed weight')
    o, i, kh, kw = (int(e) for e in weight_shape)
    ph, pw = _pair(padding, 'padding')
    b, c, h, w = x.shape
    if c != i:
        raise ValueError('fmap has %d channels, the weight takes %d' % (c, i))
    size = conv2d_out_size(h, w, (kh, kw), stride, (ph, pw))
    if wp.device != x.device or wp.numel() != lib().rw_conv2d_packed_weight_elems(o, i, kh, kw):
        raise ValueError('packed weight of %d floats on %s does not belong to a weight %s on %s'
                         % (wp.numel(), wp.device, (o, i, kh, kw), x.device))
    bias = _opt(bias, 'bias')
    if bias is not None and (tuple(bias.shape) != (o,) or bias.device != x.device):
        raise ValueError('bias must have one value per out-channel (%d) on %s, not %s on %s'
                         % (o, x.device, tuple(bias.shape), bias.device))
    return x, wp, bias, (b, i, h, w, o, kh, kw, int(stride), ph, pw), size


def conv2d(x, wp, weight_shape, bias=None, stride=1, padding=0, relu=False, out=None, c_off=0):
    """act(F.conv2d(x, weight, bias, stride, padding)) -- rw_conv2d_f32.  wp = conv2d_pack_weight(weight), weight_shape
    the (out_ch, in_ch, kh, kw) it was packed from; padding an int or (ph, pw).  With ``out=`` (B, c_total, oh, ow) the
    result is written to its channels [c_off, c_off + out_ch) and ``out`` is returned; its other channels are not touched."""
    x, wp, bias, shape, (oh, ow) = _conv2d_operands(x, wp, weight_shape, bias, stride, padding)
    y, c_off, c_total = _slice_out(out, c_off, shape[0], shape[4], oh, ow, x)
    check(lib().rw_conv2d_f32(_p(x), _p(wp), _p(bias), _p(y), *shape, int(bool(relu)), c_off, c_total, _stream()))
    return y if out is None else out


def pool3x3(x, mode, out=None, c_off=0):
    """The 3x3 poolings of the Inception graph (rw_pool3x3_f32).  mode 'max_s2' (0): max_pool2d(x, 3, 2); 'avg' (1):
    avg_pool2d(x, 3, 1, 1, count_include_pad=False); 'max_s1' (2): max_pool2d(x, 3, 1, 1).  ``out=`` / ``c_off=`` as in
    ``conv2d``."""
    x = _fmap4(x, 'fmap')
    mode = POOL_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError('mode must be one of %s or 0 / 1 / 2, not %r' % (sorted(POOL_MODES), mode))
    b, c, h, w = x.shape
    if mode == 0 and (h < 3 or w < 3):
        raise ValueError('fmap of %d x %d has no 3 x 3 window' % (h, w))
    oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == 0 else (h, w)
    y, c_off, c_total = _slice_out(out, c_off, b, c, oh, ow, x)
    check(lib().rw_pool3x3_f32(_p(x), _p(y), b, c, h, w, mode, c_off, c_total, _stream()))
    return y if out is None else out


def global_avgpool(x):
    """(B, C) means of the maps of x (B, C, H, W) -- rw_global_avgpool_f32."""
    x = _fmap4(x, 'fmap')
    b, c, h, w = x.shape
    y = torch.empty(b, c, device=x.device, dtype=torch.float32)
    check(lib().rw_global_avgpool_f32(_p(x), _p(y), b, c, h, w, _stream()))
    return y


INCEPTION_SIZE = 299


def inception_input(images, size=INCEPTION_SIZE):
    """The Inception network's input (B, 3, oh, ow) float32 (rw_inception_input_f32) from ``images``: float32 (B, 3, H, W),
    clamped to [-1, 1], or uint8 (B, H, W, 3) -- what render_bytes / png_decode yield -- mapped by x / 127.5 - 1; resized
    like F.interpolate(mode='bilinear', align_corners=False) to ``size`` (an int or (oh, ow)), or kept at its size with
    ``size=None``."""
    if not isinstance(images, torch.Tensor):
        raise TypeError('images must be a torch.Tensor')
    is_bytes = images.dtype == torch.uint8
    images = _dev(images, 'images', torch.uint8 if is_bytes else torch.float32)
    if images.dim() != 4 or 0 in images.shape or images.shape[3 if is_bytes else 1] != 3:
        raise ValueError('images must be float32 (B, 3, H, W) or uint8 (B, H, W, 3), not %s %s'
                         % (images.dtype, tuple(images.shape)))
    b = images.shape[0]
    h, w = (images.shape[1], images.shape[2]) if is_bytes else (images.shape[2], images.shape[3])
    oh, ow = (h, w) if size is None else _pair(size, 'size')
    if oh < 1 or ow < 1:
        raise ValueError('size must be positive, not %r' % (size,))
    y = torch.empty(b, 3, oh, ow, device=images.device, dtype=torch.float32)
    check(lib().rw_inception_input_f32(_p(images), _p(y), b, h, w, oh, ow, int(is_bytes), _stream()))
    return y


# ------------------------------------------------------------------ the face-parsing BiSeNet (faceparse.py) and the counts
SEG_MAX_CLASSES = 64            # FP_MAX_CLASSES of rw_faceparse.hip
SEG_MAX_SET = 16                # FP_MAX_SET


def conv2d_add(x, wp, weight_shape, bias, res, stride=1, padding=0, relu=False, out=None):
    """act((F.conv2d(x, weight, bias, stride, padding)) + res) -- rw_conv2d_add_f32, the tail of a residual block; the
    operands of ``conv2d`` and res (B, out_ch, oh, ow).  ``out=`` is written where it lies and returned; it may be ``res``
    itself."""
    x, wp, bias, shape, (oh, ow) = _conv2d_operands(x, wp, weight_shape, bias, stride, padding)
    res = _in_place(res, 'res', device=x.device)
    want = (shape[0], shape[4], oh, ow)
    if tuple(res.shape) != want:
        raise ValueError('res must be %s, the shape of the convolution\'s output, not %s' % (want, tuple(res.shape)))
    if out is None:
        y = torch.empty(want, device=x.device, dtype=torch.float32)
    else:
        y = _in_place(out, 'out', device=x.device)
        if tuple(y.shape) != want:
            raise ValueError('out must be %s, not %s' % (want, tuple(y.shape)))
    check(lib().rw_conv2d_add_f32(_p(x), _p(wp), _p(bias), _p(res), _p(y), *shape, int(bool(relu)), _stream()))
    return y if out is None else out


def maxpool3x3s2p1(x):
    """F.max_pool2d(x, 3, 2, 1) -- rw_maxpool3x3s2p1_f32: (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)."""
    x = _fmap4(x, 'fmap')
    b, c, h, w = x.shape
    y = torch.empty(b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, device=x.device, dtype=torch.float32)
    check(lib().rw_maxpool3x3s2p1_f32(_p(x), _p(y), b, c, h, w, _stream()))
    return y


def _index_table(t, n, name, device):
    """an int32 (n,) table on `device`, or None"""
    if t is None:
        return None
    t = _dev(t, name, torch.int32)
    if tuple(t.shape) != (n,) or t.device != device:
        raise ValueError('%s must be int32 (%d,) on %s, not %s on %s' % (name, n, device, tuple(t.shape), t.device))
    return t


def gate_resample(x, gate=None, add_map=None, add_vec=None, rows=None, cols=None):
    """y[b, c, oy, ox] = x[b, c, rows[oy], cols[ox]] * sigmoid(gate[b, c]) + (add_map[b, c, rows[oy], cols[ox]] or
    add_vec[b, c]) -- rw_gate_resample_f32.  rows / cols: int32 nearest-neighbour tables on x's device (faceparse.nearest_table),
    their lengths the output's size; None keeps that axis.  gate, add_vec: (B, C) or (B, C, 1, 1); add_map: a map of x's
    shape (it may be x); each of the three is optional, add_map and add_vec exclude each other.  With only tables it is
    F.interpolate(x, size) (nearest), bit for bit."""
    x = _fmap4(x, 'fmap')
    b, c, h, w = x.shape

    def per_channel(t, name):
        t = _opt(t, name)
        if t is not None and (t.numel() != b * c or tuple(t.shape[:2]) != (b, c) or t.device != x.device):
            raise ValueError('%s must be (%d, %d) or (%d, %d, 1, 1) on %s, not %s on %s'
                             % (name, b, c, b, c, x.device, tuple(t.shape), t.device))
        return t
    gate, add_vec = per_channel(gate, 'gate'), per_channel(add_vec, 'add_vec')
    if add_map is not None and add_vec is not None:
        raise ValueError('add_map and add_vec exclude each other (RW_ERR_BAD_ARGUMENT, include/rewriting_hip.h)')
    add_map = _opt(add_map, 'add_map')
    if add_map is not None and (add_map.shape != x.shape or add_map.device != x.device):
        raise ValueError('add_map must be a map of the fmap\'s shape %s on %s, not %s on %s'
                         % (tuple(x.shape), x.device, tuple(add_map.shape), add_map.device))
    oh = h if rows is None else int(rows.numel()) if isinstance(rows, torch.Tensor) else -1
    ow = w if cols is None else int(cols.numel()) if isinstance(cols, torch.Tensor) else -1
    rows, cols = _index_table(rows, oh, 'rows', x.device), _index_table(cols, ow, 'cols', x.device)
    if oh < 1 or ow < 1:
        raise ValueError('rows and cols must not be empty')
    y = torch.empty(b, c, oh, ow, device=x.device, dtype=torch.float32)
    check(lib().rw_gate_resample_f32(_p(x), _p(gate), _p(add_map), _p(add_vec), _p(rows), _p(cols), _p(y), b, c, h, w, oh, ow,
                                     _stream()))
    return y


def _ac_tables(idx, lam, oh, ow, device):
    idx, lam = _dev(idx, 'idx', torch.int32), _dev(lam, 'lam')
    if tuple(idx.shape) != (2 * oh + 2 * ow,) or tuple(lam.shape) != (oh + ow,) or idx.device != device or lam.device != device:
        raise ValueError('idx must be int32 (%d,) and lam float32 (%d,) on %s -- faceparse.device_ac_tables -- not %s on %s and '
                         '%s on %s' % (2 * oh + 2 * ow, oh + ow, device, tuple(idx.shape), idx.device, tuple(lam.shape),
                                       lam.device))
    return idx, lam


def bilinear_ac(x, size, idx, lam):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) -- rw_bilinear_ac_f32.  (idx, lam) =
    faceparse.device_ac_tables((H, W), size, device)."""
    x = _fmap4(x, 'fmap')
    b, c, h, w = x.shape
    oh, ow = _pair(size, 'size')
    if oh < 1 or ow < 1:
        raise ValueError('size must be positive, not %r' % (size,))
    idx, lam = _ac_tables(idx, lam, oh, ow, x.device)
    y = torch.empty(b, c, oh, ow, device=x.device, dtype=torch.float32)
    check(lib().rw_bilinear_ac_f32(_p(x), _p(y), b, c, h, w, oh, ow, _p(idx), _p(lam), _stream()))
    return y


def seg_labels(logits, size, idx, lam, pick_rows=None, pick_cols=None):
    """(B, 1, OH, OW) int64: the arg-max over the classes of bilinear_ac(logits, size, idx, lam) -- the lowest index among
    equals, a NaN first -- read at the pixels (pick_rows[oy], pick_cols[ox]) (int32 nearest tables; None keeps that axis) --
    rw_seg_labels_i64; the up-sampled scores are not written."""
    logits = _fmap4(logits, 'logits')
    b, n, h, w = logits.shape
    if n > SEG_MAX_CLASSES:
        raise ValueError('logits have %d classes, at most %d are taken (RW_ERR_UNSUPPORTED, include/rewriting_hip.h)'
                         % (n, SEG_MAX_CLASSES))
    H, W = _pair(size, 'size')
    if H < 1 or W < 1:
        raise ValueError('size must be positive, not %r' % (size,))
    idx, lam = _ac_tables(idx, lam, H, W, logits.device)
    OH = H if pick_rows is None else int(pick_rows.numel()) if isinstance(pick_rows, torch.Tensor) else -1
    OW = W if pick_cols is None else int(pick_cols.numel()) if isinstance(pick_cols, torch.Tensor) else -1
    pick_rows = _index_table(pick_rows, OH, 'pick_rows', logits.device)
    pick_cols = _index_table(pick_cols, OW, 'pick_cols', logits.device)
    if OH < 1 or OW < 1:
        raise ValueError('pick_rows and pick_cols must not be empty')
    labels = torch.empty(b, 1, OH, OW, device=logits.device, dtype=torch.int64)
    check(lib().rw_seg_labels_i64(_p(logits), _p(labels), b, n, h, w, H, W, _p(idx), _p(lam), _p(pick_rows), _p(pick_cols),
                                  OH, OW, _stream()))
    return labels


def _label_set(labels, name):
    labels = [int(v) for v in labels]
    if not 1 <= len(labels) <= SEG_MAX_SET:
        raise ValueError('%s must name 1 .. %d labels, not %d' % (name, SEG_MAX_SET, len(labels)))
    return (ctypes.c_int64 * len(labels))(*labels), len(labels)


def _label_maps(t, channel, name):
    """(the contiguous int64 tensor, the pointer of its channel `channel`, elements per image, H W)"""
    t = _dev(t, name, torch.int64)
    if t.dim() not in (3, 4) or 0 in t.shape:
        raise ValueError('%s must be a non-empty int64 (B, H, W) or (B, C, H, W), not %s' % (name, tuple(t.shape)))
    channels = t.shape[1] if t.dim() == 4 else 1
    if not isinstance(channel, int) or not 0 <= channel < channels:
        raise ValueError('%s has %d channel(s), channel %r is none of them' % (name, channels, channel))
    hw = t.shape[-2] * t.shape[-1]
    return t, ctypes.c_void_p(t.data_ptr() + 8 * channel * hw), channels * hw, hw


def seg_correct_counts(before, after, src, tgt, srcc=0, tgtc=0):
    """(B, 2) int64 (total, count) per image -- rw_seg_correct_counts_i64: count = the pixels whose ``before`` label is in
    ``src``, total = those of them whose ``after`` label is in ``tgt`` (1 .. 16 labels each).  before, after: int64
    (B, H, W) or (B, C, H, W) with the channel srcc / tgtc, read where they lie."""
    src, n_src = _label_set(src, 'src')
    tgt, n_tgt = _label_set(tgt, 'tgt')
    before, bp, bstride, hw = _label_maps(before, srcc, 'before')
    after, ap, astride, ahw = _label_maps(after, tgtc, 'after')
    if after.shape[0] != before.shape[0] or tuple(after.shape[-2:]) != tuple(before.shape[-2:]) or after.device != before.device:
        raise ValueError('before %s on %s and after %s on %s must agree in batch, size and device'
                         % (tuple(before.shape), before.device, tuple(after.shape), after.device))
    out = torch.empty(before.shape[0], 2, device=before.device, dtype=torch.int64)
    check(lib().rw_seg_correct_counts_i64(bp, ap, before.shape[0], hw, bstride, astride, src, n_src, tgt, n_tgt, _p(out),
                                          _stream()))
    return out
