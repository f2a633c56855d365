"""Sequential StyleGANv2 generator on MI355X kernels.

Drop-in for utils/stylegan2/models.py: the same class names, constructor arguments, child-module
names and state-dict keys (level B2), so ``nethook.subsequence``,
``InstrumentedModel`` and ``ganrewrite.SeqStyleGanRewriter`` split and hook it exactly as they
split the reference.  Every non-leaf is an ``nn.Sequential``; data flows as ``DataBag`` dicts.

What differs is underneath: every leaf calls a hand-written gfx950 kernel through the C ABI
(``rewriting_amd.hip``), and a ``StyledConvSeq`` whose children are all present and un-hooked
runs as ONE fused block (style multiply folded into the implicit-GEMM gather; demodulation,
noise, bias and leaky-ReLU in its epilogue) -- invisible at the module boundaries the
rewriter observes, because any hook or split turns the fusion off for that block.

A model cast with ``.double()`` runs its forward on the float64 kernels (``hip.*_f64``): every module dispatches on the
dtype of the tensor it is given, before any routing or fusion logic.  float32 takes the path described above; float64
runs module by module (no fusion, no side streams, no packed weights), forward only: under grad mode a double layer
that would have to record a graph raises, and the rewriters refuse a double model.
"""
import contextlib
import math
import re
import threading
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch
from torch import nn

from . import grad, op, routing
from .routing import switches
from ... import hip

# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------

_weight_epoch = [0]


def bump_weight_epoch():
    """Called by code that rewrites parameters through raw device pointers (the HIP solver),
    which torch's version counters cannot see; invalidates every derived-weight cache."""
    _weight_epoch[0] += 1


class _DerivedWeights:
    """Cache of tensors derived from a parameter (repacked weights, squared sums), keyed on the
    parameter's storage, torch version counter and the package-wide epoch."""

    def __init__(self):
        self.store = {}

    def get(self, name, param, make):
        key = (param.data_ptr(), param._version, _weight_epoch[0], str(param.device))
        hit = self.store.get(name)
        if hit is None or hit[0] != key:
            hit = (key, make())
            self.store[name] = hit
        return hit[1]


_noise_streams = {}


def reference_noise(batch, hw, device, double=False):
    """The reference regenerates ``np.random.RandomState(0).randn(batch, H*W)`` on the host for
    every noise layer of every call (utils/stylegan2/models.py:542-545; quirk Q1).  That is a
    fixed stream prefix, so it is generated once and kept on the device.  double: the same float32
    rows widened to float64, as torch's promotion widens them when the feature map is double
    (models.py:539-546) -- a stream of its own, widened on the host."""
    need = batch * hw
    key = (str(device), 'f64') if double else str(device)
    stream = _noise_streams.get(key)
    if stream is None or stream.numel() < need:
        n = max(need, 1 << 16)
        host = np.random.RandomState(0).randn(n).astype('float32')
        if double:
            host = host.astype('float64')
        stream = torch.from_numpy(host).to(device)
        _noise_streams[key] = stream
    period = _noise_period[0]
    if period == 1 and batch > 1:
        return reference_noise_row0(hw, device, double).expand(batch, hw)
    if period and batch > period:
        # Several reference-sized batches run as one launch: image j takes the noise row it would have
        # had in its own batch of `period` (row j mod period), see noise_batch_period().
        if batch % period:
            raise ValueError('batch %d is not a multiple of the noise period %d' % (batch, period))
        rows = reference_noise(period, hw, device, double)
        return rows.repeat(batch // period, 1)
    return stream[:need].view(batch, hw)


def reference_noise_row0(hw, device, double=False):
    _noise_period[0], saved = 0, _noise_period[0]
    try:
        return reference_noise(1, hw, device, double)
    finally:
        _noise_period[0] = saved


_noise_period = [0]


class noise_batch_period:
    """Context manager.  The reference's noise depends on an image's ROW WITHIN ITS BATCH (quirk Q1),
    and its statistics sweeps use batches of 10 (utils/tally.py:631-647).  Inside this context a
    batch of k*period images is treated as k consecutive reference batches, so a sweep can run
    large launches and still give every seed exactly the noise the reference gives it."""

    def __init__(self, period):
        self.period = int(period)

    def __enter__(self):
        self.old = _noise_period[0]
        _noise_period[0] = self.period
        return self

    def __exit__(self, *exc):
        _noise_period[0] = self.old


def make_kernel(k):
    k = torch.tensor(k, dtype=torch.float32)
    if k.ndim == 1:
        k = torch.outer(k, k)
    return k / k.sum()


_F64 = torch.float64


def _double(what, x, **operands):
    """The dtype dispatch of a module: True when it runs on the float64 kernels (hip.*_f64), False for today's float32
    path (which also refuses every other dtype, in rewriting_amd.hip).  `x` is the incoming tensor, `operands` the
    module's own tensors (None = absent): if any of them is float64 all must be -- otherwise RuntimeError, naming
    both dtypes, before anything is launched."""
    if x.dtype is not _F64 and all(t is None or t.dtype is not _F64 for t in operands.values()):
        return False
    for name, t in operands.items():
        if t is not None and t.dtype != x.dtype:
            raise RuntimeError('rewriting_amd: %s: the input is %s and the %s %s -- cast the model and its input to one '
                               'dtype, .float() or .double() (nothing is converted)' % (what, x.dtype, name, t.dtype))
    return True


def _forward_only_f64(what, *tensors):
    """The float64 path is forward only (grad.py, the adjoints of the styled convolution, is float32): a double layer
    that would have to record a graph raises instead of returning a result without one."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError('rewriting_amd: %s: the float64 path is forward only -- no graph is recorded for double '
                                  'tensors (the adjoints in utils/stylegan2/grad.py are float32); run it under '
                                  'torch.no_grad(), or differentiate a .float() model' % what)


def _unhooked(*modules):
    """nethook hooks a layer by planting a ``forward`` attribute on the instance
    (utils/nethook.py:197-201)."""
    return all('forward' not in m.__dict__ for m in modules)


# The RGB branch (up_rgbK, to_rgbK) is HBM-bound and hangs off the feature-map trunk, whose convolutions
# are MFMA-bound: when the WHOLE generator runs un-hooked (SeqStyleGAN2.forward below) the branch is
# issued on a second HIP stream so that it overlaps the next styled convolutions, and is joined
# before the image is returned.  Hooked / sliced models (nethook) never see this: the mode is on only
# inside that forward.
def _idle():
    """The record of the running forward while none runs: every field, and its default, is stated here."""
    return dict(
        stream=None,        # the RGB branch's stream and ...
        aux=None,           # ... the auxiliary one (border strips, prefetch) of the running side-stream forward
        keep=[],            # trunk tensors the side streams still read: referenced until the join (_side_streams_joined)
        final=None,         # (last StyledConvSeq, its ToRGBF, latent index of the ToRGB) of the running forward
        image_path=False,   # inside the un-hooked forward of a whole generator (see routing.conv_algo)
        inline_up=False,    # ... in which UpsampleO hands the running image on at half size (hip.HalfSkip): RW_RGB_INLINE_UP
        switches=None,      # routing.switches() of the running generator forward
        neighbours={},      # id(StyledConvSeq) -> _Neighbours of the running un-hooked forward (SeqStyleGAN2._topology)
        pre={},             # id(StyledConvSeq) -> (style, demod factors), id(ToRGBF) -> style: computed up front
        pre_join=None)      # the stream they were computed on, until the trunk has waited for it


class _RunningForward(threading.local):     # per thread: two threads may run generators concurrently
    def __init__(self):
        vars(self).update(_idle())


_running = _RunningForward()
_side_streams = {}              # (device, 'rgb' / 'aux') -> stream; module-level: models are deep-copied by the rewriters
# who reads a StyledConvSeq's result: `reader` the next StyledConvSeq (any kind); `successor` (the stride-1 StyledConvSeq
# directly behind this upsampling one, its latent index); `torgb` (the ToRGBF directly behind, its latent index); or None
_Neighbours = namedtuple('_Neighbours', 'reader successor torgb')
_NO_NEIGHBOURS = _Neighbours(None, None, None)


class _scope:
    """with _scope(field=value, ...): the only place that assigns fields of the running forward's record.  The values
    they had return on exit, whether or not the body raised."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        record = vars(_running)
        self.saved = {name: record[name] for name in self.fields}
        record.update(self.fields)

    def __exit__(self, *exc):
        vars(_running).update(self.saved)


def _side_stream(device, which):
    """The device's stream `which` ('rgb' / 'aux') for the work beside the trunk (RGB branch, border strips, prefetch),
    made at its first use.  RW_SIDE_PRIORITY (default 0): the priority torch gives it (positive = below the trunk's
    stream; clamped to the device's range)."""
    stream = _side_streams.get((device, which))
    if stream is None:
        stream = _side_streams[device, which] = torch.cuda.Stream(device=device, priority=_switches().side_priority)
    return stream


@contextlib.contextmanager
def _side_streams_joined(device):
    """The side-stream scope of one generator forward: the device's two streams are installed; on the way out, raised or
    not, the caller's stream (which is yielded) first waits for the RGB branch -- the image is then complete on it --
    and only THEN are the tensors of `keep` released, to the trunk's pool.  The branch reads trunk tensors from another
    stream, so they stay referenced until that join (Tensor.record_stream would do, but it defers the allocator's reuse
    of multi-GB blocks unpredictably and shows up as intermittent hipMalloc stalls at large batch)."""
    main, side = torch.cuda.current_stream(), _side_stream(device, 'rgb')
    try:
        with _scope(stream=side, aux=_side_stream(device, 'aux')):
            yield main
    finally:
        main.wait_stream(side)      # the join is queued first ...
        del _running.keep[:]        # ... then the kept tensors go, to the trunk's pool


def _rgb_stream():
    return _running.stream


def _prefetched(module):
    """(style, demod) of a StyledConvSeq / the style of a ToRGBF computed at the start of the un-hooked forward
    (SeqStyleGAN2._prefetch_modulations), or None.  The first reader makes the trunk wait for the stream they
    were computed on."""
    entry = _running.pre.get(id(module))
    if entry is not None and _running.pre_join is not None:
        torch.cuda.current_stream().wait_stream(_running.pre_join)
        _running.pre_join = None        # consumed once (the one assignment outside _scope, which restores it anyway)
    return entry


def _style_of(module, ahead, latent, index=None):
    """The style of a StyledConvSeq / ToRGBF for the row latent[:, index] (`latent` itself without an index): `ahead`, what
    _prefetched(module) gave the caller (whose stream then waits for it), else computed now on the current stream."""
    styled = isinstance(module, StyledConvSeq)
    if ahead is not None:
        return ahead[0] if styled else ahead
    row = latent if index is None else latent[:, index]
    return module.mconv.modulation(DataBag(style=row)).style if styled else module.conv.modulation(row)


def _switches():
    """The snapshot of the RW_* switches that the running generator forward took at its start, else a fresh one."""
    return _running.switches or switches()


def fusion_enabled():
    return _switches().fuse


def conv_impl():
    """rw_conv3x3_f32's impl for the 3x3 convolutions (RW_CONV_IMPL, see routing.Switches)."""
    return _switches().conv_impl


def matrix_mode_of_image_path():
    """matrix_mode() as the un-hooked forward of a whole generator sees it (bench.py labels its line with it)."""
    return routing.matrix_mode(_switches(), True)


def micro_batch():
    """(images per slice, first resolution run in slices) of SeqStyleGAN2._forward_micro: RW_MICRO_BATCH = "k[:res]"."""
    return _switches().micro_batch


def _context(tensor, weight_changes=False):
    """routing.Context of a layer that is about to run on `tensor`'s device."""
    on_device = tensor.is_cuda
    return routing.Context(_running.image_path, on_device, on_device and torch.cuda.is_current_stream_capturing(),
                           _running.stream is not None, _running.aux is not None, weight_changes)


def _amax_of(fmap):
    """The bound of |fmap| that its producer -- a fused layer of the running un-hooked forward -- left ON the tensor
    (attribute rw_amax: (bound, the tensor's version counter when it was written)), or None: the kernels then measure
    the map themselves (hip.absmax).  It travels with the tensor object, not with an address or a bag key: a slice, a
    copy or a map that was edited in place since (hooks) carries no usable bound.  Trusted only inside the un-hooked
    forward of a whole generator, where producer and consumer are both ours."""
    if fmap is None or not _running.image_path:
        return None
    entry = getattr(fmap, 'rw_amax', None)
    if entry is not None and entry[1] == fmap._version:
        return entry[0]
    return None


class DataBag(dict):
    """dict with attribute access, carrying latent / style / fmap / output / noise through the
    sequential generator (reference: utils/stylegan2/models.py:204-230)."""

    def __init__(self, rep=None, **kwargs):
        super().__init__()
        self.update(rep, **kwargs)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def __delattr__(self, name):
        try:
            del self[name]
        except KeyError:
            raise AttributeError(name)

    def update(self, rep=None, **kwargs):
        if rep is not None:
            super().update(rep)
        super().update(kwargs)


# ------------------------------------------------------------------------------------------
# leaves
# ------------------------------------------------------------------------------------------

class InputLatent(nn.Module):
    def forward(self, z):
        return DataBag(latent=z)


class ReturnOutput(nn.Module):
    def forward(self, d):
        return d.output


class PixelNormL(nn.Module):
    def forward(self, d):
        if d.latent.dtype is _F64:
            return DataBag(d, latent=hip.pixel_norm_f64(d.latent))
        if grad.records(d.latent):
            return DataBag(d, latent=grad.PixelNorm.apply(d.latent, 1e-8))
        return DataBag(d, latent=hip.pixel_norm(d.latent))


class EqualLinear(nn.Linear):
    """Equalised-learning-rate linear layer (reference: models.py:487-517)."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, lr_mul=1, activation=None):
        self.bias_init = bias_init
        self.lr_mul = lr_mul
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul
        super().__init__(in_dim, out_dim, bias)
        self.activation = activation

    def reset_parameters(self):
        nn.init.normal_(self.weight, std=1.0 / self.lr_mul)
        if self.bias is not None:
            nn.init.constant_(self.bias, self.bias_init)

    def forward(self, input):
        if _double('EqualLinear', input, weight=self.weight, bias=self.bias):
            return hip.equal_linear_f64(input, self.weight, self.bias, self.scale, self.lr_mul,
                                        act=bool(self.activation))
        if grad.records(input, self.weight, self.bias):
            return grad.EqualLinear.apply(input, self.weight, self.bias, self)
        return hip.equal_linear(input, self.weight, self.bias, self.scale, self.lr_mul,
                                act=bool(self.activation))

    def __repr__(self):
        return '%s(%d, %d)' % (type(self).__name__, self.weight.shape[1], self.weight.shape[0])


class EqualLinearL(EqualLinear):
    def forward(self, d):
        return DataBag(d, latent=super().forward(d.latent))


class EqualLinearS(EqualLinear):
    def forward(self, d):
        return DataBag(d, style=super().forward(d.style))


class AdjustLatent(nn.Module):
    """Truncation toward ``latent_avg`` and broadcast to one row per layer (models.py:570-583).
    As in the reference the buffer starts as a 0-d placeholder and truncation only applies once
    it has been given a real vector."""

    def __init__(self, n_latent, truncation=1.0):
        super().__init__()
        self.n_latent = n_latent
        self.truncation = truncation
        self.register_buffer('latent_avg', torch.tensor(0.0))

    def forward(self, d):
        truncate = self.truncation != 1.0 and self.latent_avg.ndim > 0
        adjust = hip.adjust_latent
        if _double('AdjustLatent', d.latent, latent_avg=self.latent_avg if truncate else None):
            adjust = hip.adjust_latent_f64
        elif grad.records(d.latent):
            adjust = grad.AdjustLatent.apply
        lat = adjust(d.latent, self.latent_avg if truncate else None, self.n_latent,
                     self.truncation)
        return DataBag(d, latent=lat)


class PickLatent(nn.Module):
    def __init__(self, index):
        super().__init__()
        self.index = index

    def __repr__(self):
        return '%s(%d)' % (type(self).__name__, self.index)

    def forward(self, d):
        return DataBag(d, style=d.latent[:, self.index])


class NoiseBuffers(nn.Module):
    def __init__(self, replace_input=False):
        super().__init__()
        self.replace_input = replace_input

    def forward(self, d):
        for name, buf in self.named_buffers(recurse=False):
            if name.startswith('noise_') and (self.replace_input or name not in d):
                d[name] = buf
        return d


class FixedNoiseBuffers(NoiseBuffers):
    """Per-layer fixed noise images noise_0.. (models.py:342-352).  Present in the state dict for
    checkpoint compatibility; NoiseInjectionF never reads them (quirk Q1)."""

    def __init__(self, num_layers, seed, replace_input=False):
        super().__init__(replace_input=replace_input)
        self.num_layers = num_layers
        rng = np.random.RandomState(seed)
        for idx in range(num_layers):
            res = 2 ** ((idx + 5) // 2)
            self.register_buffer('noise_%d' % idx,
                                 torch.from_numpy(rng.randn(1, 1, res, res).astype('float32')))


class ConstantInputF(nn.Module):
    def __init__(self, channel, size=4):
        super().__init__()
        self.input = nn.Parameter(torch.randn(1, channel, size, size))

    def forward(self, d):
        if grad.records(self.input) and self.input.dtype is not _F64:
            return DataBag(d, fmap=self.input.repeat(d.latent.shape[0], 1, 1, 1))      # the constant is trained too
        return DataBag(d, fmap=self.input.detach().repeat(d.latent.shape[0], 1, 1, 1))


class ApplyStyle(nn.Module):
    """fmap * style -- its output is the rewriter's key (rewrite/ganrewrite.py:662-665)."""

    def forward(self, d):
        if _double('ApplyStyle', d.fmap, style=d.style):
            _forward_only_f64('ApplyStyle', d.fmap, d.style)
            return DataBag(d, fmap=hip.style_mul_f64(d.fmap, d.style))
        return DataBag(d, fmap=grad.StyleMul.apply(d.fmap, d.style))


class DemodulatedConv2dF(nn.Module):
    """The plain linear convolution the rewriter edits, followed by the demodulation factor
    (models.py:291-329).  Stride 1: 3x3 conv, pad 1.  upsample: stride-2 transposed conv to
    (2H+1, 2W+1)."""

    def __init__(self, in_channel, out_channel, kernel_size, demodulate=True, upsample=False):
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError('the gfx950 kernels implement 3x3 styled convolutions')
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.padding = kernel_size // 2
        self.demodulate = demodulate
        self.upsample = upsample
        self.weight = nn.Parameter(torch.randn(1, out_channel, in_channel, kernel_size, kernel_size))
        self._derived = _DerivedWeights()

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_derived'] = _DerivedWeights()       # caches are not copied or pickled
        return state

    def __repr__(self):
        return '%s(%d, %d, %d, upsample=%s)' % (type(self).__name__, self.in_channel,
                                                self.out_channel, self.kernel_size, self.upsample)

    def packed_weight(self):
        return self._derived.get('packed', self.weight,
                                 lambda: hip.pack_conv_weight(self.weight, 1 if self.upsample else 0))

    def wino_weight(self):
        return self._derived.get('wino', self.weight, lambda: hip.pack_conv_weight_wino(self.weight))

    def up_wino_weight(self, split=False):
        return self._derived.get('upwino_split' if split else 'upwino', self.weight,
                                 lambda: hip.pack_conv_transpose_weight_wino(self.weight, split=split))

    def up_blur_wino4_weight(self, k4, split=False):
        return self._derived.get('upblur4_split' if split else 'upblur4', self.weight,
                                 lambda: hip.pack_conv_transpose_blur_weight_wino4(self.weight, k4, split=split))

    def direct16_weight(self):
        return self._derived.get('direct16', self.weight, lambda: hip.pack_conv_weight_direct16(self.weight))

    def up_blur_direct16_weight(self, k4):
        return self._derived.get('upblur_direct16', self.weight,
                                 lambda: hip.pack_conv_transpose_blur_weight_direct16(self.weight, k4))

    def wino4_weight(self, split=False):
        return self._derived.get('wino4_split' if split else 'wino4', self.weight,
                                 lambda: hip.pack_conv_weight_wino4(self.weight, split=split))

    def bf16x6_weight(self):
        return self._derived.get('packed_bf16x3', self.weight, lambda: hip.pack_conv_weight_bf16x3(self.weight))

    def route(self, ctx, h, w, blur=None):
        """THE routing decision for a map of h x w.  blur: the layer's BlurF where the caller runs the whole StyledConv."""
        if not self.upsample:
            return routing.stride1_route(_switches(), ctx, self.in_channel, self.out_channel, h, w)
        whole = blur is not None and tuple(blur.pad) == (1, 1) and tuple(blur.kernel.shape) == (4, 4)
        return routing.upsample_route(_switches(), ctx, self.in_channel, self.out_channel, h, w, whole)

    def hooked_direct16(self, h, w):
        """The hooked branch of routing.stride1_route (the one direct sum that reports no bound) for a map of h x w?"""
        route = self.route(_context(self.weight), h, w)
        return route.kernel == 'direct16' and not route.reports_bound

    def squared_sums(self):
        return self._derived.get('wsq', self.weight, lambda: hip.weight_sqsum(self.weight, self.scale))

    def demod_factors(self, style, ahead=None):
        """The demodulation factors: `ahead` where the running forward computed them up front, else computed now."""
        if ahead is not None:
            return ahead
        return hip.demod(self.squared_sums(), style) if self.demodulate else None

    # route kernel (routing.STRIDE1_KERNELS, the whole-layer UP_KERNELS) -> (stem of its wrapper in `hip`, looked up there at
    # call time, the weight packed for it); stem + '_to_rgb': ToRGB in the epilogue, stem + '_rgb_partial': its partial sums
    KERNELS = {
        'direct16': ('conv3x3_direct16', lambda m, route, fir: m.direct16_weight()),
        'wino4_split': ('conv3x3_wino4', lambda m, route, fir: m.wino4_weight(True)),
        'wino4': ('conv3x3_wino4', lambda m, route, fir: m.wino4_weight(False)),
        'wino': ('conv3x3_wino', lambda m, route, fir: m.wino_weight()),
        'bf16x6': ('conv3x3_bf16x6', lambda m, route, fir: m.bf16x6_weight()),
        'gemm': ('conv3x3', lambda m, route, fir: m.packed_weight()),          # the one that takes impl=conv_impl()
        'fused': ('conv_transpose3x3s2_blur_fused', lambda m, route, fir: m.direct16_weight()),    # and the FIR itself
        'one_pass_direct16': ('conv_transpose3x3s2_blur_direct16', lambda m, route, fir: m.up_blur_direct16_weight(fir)),
        'one_pass_wino4': ('conv_transpose3x3s2_blur_wino4', lambda m, route, fir: m.up_blur_wino4_weight(fir, route.split)),
    }

    def run(self, fmap, style, style_on_load, demod=None, x_amax=None, y_amax=None, rgb=None, to_rgb=None,
            weight_changes=False, route=None, **epilogue):
        """Dispatches on `route` (self.route(...) of the map; computed here if the caller has not).  x_amax: the bound of
        |fmap| if its producer left one (hip.new_bound; the kernels of route.reads_bound take it and measure the map
        themselves otherwise); y_amax: a hip.new_bound buffer that receives the result's bound where route.reports_bound;
        rgb: (ToRGB weight (3, out), its style (B, out), its scale), only where route.rgb_partials -- the result is then
        (map, partial images); to_rgb: (ToRGB weight, its style, bias, running image, scale) with a routing.FinalRgbRoute
        -- the result is then (None, image); weight_changes: the caller differentiates with respect to the weight."""
        if route is None:
            route = self.route(_context(fmap, weight_changes), fmap.shape[-2], fmap.shape[-1])
        if rgb is not None and (self.upsample or not route.rgb_partials):
            raise RuntimeError('run(rgb=...) on a layer that does not leave ToRGB partial sums')
        args = dict(style=style if style_on_load else None, demod=self.demod_factors(style, demod))
        if self.upsample:
            return self._run_two_pass(fmap, route, x_amax, args)
        stem, packed = self.KERNELS[route.kernel]
        args.update(epilogue)
        if route.reads_bound:
            args['x_amax'] = x_amax
        head = (fmap, packed(self, route, None), self.out_channel, self.scale)
        if to_rgb is not None:
            return getattr(hip, stem + '_to_rgb')(*head, *to_rgb, **args)
        if route.reports_bound:
            args['y_amax'] = y_amax
        if rgb is not None:
            return getattr(hip, stem + '_rgb_partial')(*head, *rgb, **args)
        if route.kernel == 'gemm':
            args['impl'] = conv_impl()
        return getattr(hip, stem)(*head, **args)

    def run_whole_layer(self, fmap, style, route, fir, demod=None, **rest):
        """The upsampling layer in one launch (route.runs_layer): transposed convolution, blur by `fir`, then what `rest`
        names -- noise, the epilogue, post_scale and the bounds, as the kernel's wrapper takes them.  Under
        RW_UP_FUSED2_JOIN the current stream first waits for the running forward's RGB stream, in front of the fused kernel."""
        stem, packed = self.KERNELS[route.kernel]
        fused = route.kernel == 'fused'
        if fused and _switches().up_fused2_join and _running.stream is not None:
            torch.cuda.current_stream().wait_stream(_running.stream)
        return getattr(hip, stem)(fmap, packed(self, route, fir), *((fir,) if fused else ()), self.out_channel, self.scale,
                                  style=style, demod=self.demod_factors(style, demod), **rest)

    def _run_two_pass(self, fmap, route, x_amax, args):
        """The transposed convolution alone, to the (2H+1) x (2W+1) map (its blur is the caller's)."""
        if route.kernel == 'plain':
            return hip.conv_transpose3x3s2(fmap, self.packed_weight(), self.out_channel, self.scale, impl=conv_impl(), **args)
        f22 = {'f22_strips': True, 'halo_strips': False}[route.kernel]        # no other name: KeyError
        # quad tiles (F(2,2) where it applies, else the direct halo kernel) and the border row / column strips write
        # disjoint elements of the same map.  The strips (latency-bound, 2 % of the step) go to an auxiliary stream beside
        # the tiles: the one of the running whole-generator forward, else (a sliced or hooked model: the statistics
        # sweeps, the rewriter's sub-models) the device's own -- in a 250-seed sweep launch the three strip kernels were
        # 17 % of the time, in line
        b, _, h, w = fmap.shape
        aux = None
        if route.side_strips:
            aux = _running.aux if _running.aux is not None else _side_stream(fmap.device, 'aux')
        out = torch.empty(b, self.out_channel, 2 * h + 1, 2 * w + 1, device=fmap.device, dtype=fmap.dtype)
        wp = self.packed_weight()      # (re)packed on the trunk's stream BEFORE the fork
        uf = self.up_wino_weight(route.split) if f22 else None
        if f22 and route.split and x_amax is None:
            x_amax = hip.absmax(fmap)
        if aux is not None:
            main = torch.cuda.current_stream()
            aux.wait_stream(main)
        with torch.cuda.stream(aux) if aux is not None else contextlib.nullcontext():
            hip.conv_transpose3x3s2(fmap, wp, self.out_channel, self.scale, impl=8, out=out, **args)
        if f22:
            hip.conv_transpose3x3s2_wino(fmap, uf, self.out_channel, self.scale, out=out,
                                         x_amax=x_amax if route.split else None, **args)
        else:
            hip.conv_transpose3x3s2(fmap, wp, self.out_channel, self.scale, impl=7, out=out, **args)
        if aux is not None:
            main.wait_stream(aux)      # queued while fmap / style / demod / out are still referenced
        return out

    def squared_sums_f64(self):
        """The one derived tensor of the double path (none of the packed weights applies): cached per weight version."""
        return self._derived.get('wsq_f64', self.weight, lambda: hip.weight_sqsum_f64(self.weight, self.scale))

    def run_f64(self, fmap, style, style_on_load):
        """The double form of run(): the convolution on the weight as stored, then the demodulation factor."""
        demod = hip.demod_f64(self.squared_sums_f64(), style) if self.demodulate else None
        conv = hip.conv_transpose3x3s2_f64 if self.upsample else hip.conv3x3_f64
        return conv(fmap, self.weight[0], self.scale, style=style if style_on_load else None, demod=demod)

    def forward(self, d):
        if _double('DemodulatedConv2dF', d.fmap, weight=self.weight, style=d.style):
            _forward_only_f64('DemodulatedConv2dF', d.fmap, self.weight, d.style)
            return DataBag(d, fmap=self.run_f64(d.fmap, d.style, style_on_load=False))
        # through torch.autograd (grad.DemodConv: backward to the input map, the weight -- both terms, quirk Q3 --
        # and the style); without a graph this is run() and nothing else
        return DataBag(d, fmap=grad.DemodConv.apply(d.fmap, self.weight, d.style, self))


class Blur(nn.Module):
    def __init__(self, kernel, pad, upsample_factor=1):
        super().__init__()
        k = make_kernel(kernel)
        if upsample_factor > 1:
            k = k * (upsample_factor ** 2)
        self.register_buffer('kernel', k)
        self.pad = pad

    def forward(self, input):
        return op.upfirdn2d(input, self.kernel, pad=self.pad)


class BlurF(Blur):
    def forward(self, d):
        return DataBag(d, fmap=super().forward(d.fmap))


class Upsample(nn.Module):
    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer('kernel', make_kernel(kernel) * (factor ** 2))
        p = self.kernel.shape[0] - factor
        self.pad = ((p + 1) // 2 + factor - 1, p // 2)

    def forward(self, input):
        return op.upfirdn2d(input, self.kernel, up=self.factor, down=1, pad=self.pad)


class UpsampleF(Upsample):
    def forward(self, d):
        return DataBag(d, fmap=super().forward(d.fmap))


class UpsampleO(Upsample):
    def __init__(self, kernel=[1, 3, 3, 1], factor=2):
        super().__init__(kernel, factor)

    def forward(self, d):
        side = _rgb_stream()
        if side is None:
            return DataBag(d, output=super().forward(d.output))
        if (_running.inline_up and d.output.dtype is torch.float32 and self.factor == 2
                and tuple(self.kernel.shape) == (4, 4)):
            # inside the un-hooked forward the ToRGB one level up reads the image where it is and upsamples it inside its
            # own kernel (hip.HalfSkip); a consumer that cannot asks for this launch after all (_full_size)
            return DataBag(d, output=hip.HalfSkip(d.output, self.kernel))
        with torch.cuda.stream(side):              # the previous RGB image was produced on this stream
            return DataBag(d, output=super().forward(d.output))


def _full_size(skip):
    """The running image as a tensor: the upsampling launch that UpsampleO left out (a hip.HalfSkip in the bag), issued on
    the RGB stream as it would have been, for a ToRGB whose kernel takes the materialised image only."""
    if not isinstance(skip, hip.HalfSkip):
        return skip
    with torch.cuda.stream(_rgb_stream()):
        return op.upfirdn2d(skip.image, skip.fir, up=2, down=1, pad=(2, 1))


class NoiseInjectionF(nn.Module):
    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1))

    def noise_for(self, d, batch, height, width, device, double=False):
        noise = d.get('noise', None)
        if noise is None:
            rows = d.get('batch_rows', None)
            if rows is not None:        # a slice [start, start + batch) of a launch of `total` images keeps its rows
                start, total = rows
                return reference_noise(total, height * width, device, double)[start:start + batch]
            return reference_noise(batch, height * width, device, double)
        return noise.reshape(batch, height * width)

    def forward(self, d):
        b, _, h, w = d.fmap.shape
        if _double('NoiseInjectionF', d.fmap, weight=self.weight, noise=d.get('noise', None)):
            _forward_only_f64('NoiseInjectionF', d.fmap, self.weight)
            noise = self.noise_for(d, b, h, w, d.fmap.device, double=True)
            return DataBag(d, fmap=hip.noise_add_f64(d.fmap, noise, self.weight))
        return DataBag(d, fmap=grad.NoiseAdd.apply(d.fmap, self.noise_for(d, b, h, w, d.fmap.device), self.weight))


class FusedLeakyReLUF(op.FusedLeakyReLU):
    def forward(self, d):
        return DataBag(d, fmap=super().forward(d.fmap))


class ModulatedConv2d(nn.Module):
    """Style-modulated convolution taking (input, style) tensors (models.py:354-425).  3x3 uses
    the styled implicit-GEMM kernels (style folded into the gather, demodulation in the
    epilogue: the same arithmetic as modulating the weights first); 1x1 without demodulation is
    the ToRGB projection."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, demodulate=True,
                 upsample=False, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        self.eps = 1e-8
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.upsample = upsample
        if upsample:
            factor = 2
            p = (len(blur_kernel) - factor) - (kernel_size - 1)
            self.blur = Blur(blur_kernel, pad=((p + 1) // 2 + factor - 1, p // 2 + 1),
                             upsample_factor=factor)
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.padding = kernel_size // 2
        self.weight = nn.Parameter(torch.randn(1, out_channel, in_channel, kernel_size, kernel_size))
        self.modulation = EqualLinear(style_dim, in_channel, bias_init=1)
        self.demodulate = demodulate
        self._derived = _DerivedWeights()

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_derived'] = _DerivedWeights()
        return state

    def __repr__(self):
        return '%s(%d, %d, %d, upsample=%s, downsample=False)' % (
            type(self).__name__, self.in_channel, self.out_channel, self.kernel_size, self.upsample)

    def forward(self, input, style):
        double = _double('ModulatedConv2d', input, weight=self.weight, style=style)
        style = self.modulation(style)
        if self.kernel_size == 1:
            if self.demodulate or self.upsample or self.out_channel != 3:
                raise NotImplementedError('1x1 modulated conv is implemented for ToRGB only')
            to_rgb = hip.to_rgb_f64 if double else hip.to_rgb
            return to_rgb(input, self.weight.view(3, self.in_channel), style, None, None, self.scale)
        if self.kernel_size != 3:
            raise NotImplementedError('kernel_size %d' % self.kernel_size)
        if double:
            # the weight as stored, the style on load: only wsq is cached per weight version
            demod = None
            if self.demodulate:
                wsq = self._derived.get('wsq_f64', self.weight, lambda: hip.weight_sqsum_f64(self.weight, self.scale))
                demod = hip.demod_f64(wsq, style)
            if self.upsample:
                return self.blur(hip.conv_transpose3x3s2_f64(input, self.weight[0], self.scale, style=style, demod=demod))
            return hip.conv3x3_f64(input, self.weight[0], self.scale, style=style, demod=demod)
        wp = self._derived.get('packed', self.weight,
                               lambda: hip.pack_conv_weight(self.weight, 1 if self.upsample else 0))
        demod = None
        if self.demodulate:
            wsq = self._derived.get('wsq', self.weight, lambda: hip.weight_sqsum(self.weight, self.scale))
            demod = hip.demod(wsq, style)
        if self.upsample:
            out = hip.conv_transpose3x3s2(input, wp, self.out_channel, self.scale, style=style,
                                          demod=demod, impl=conv_impl())
            return self.blur(out)
        return hip.conv3x3(input, wp, self.out_channel, self.scale, style=style, demod=demod,
                           impl=conv_impl())


class ModulatedConv2dF(ModulatedConv2d):
    def forward(self, d):
        return DataBag(d, fmap=super().forward(d.fmap, d.style))


class ToRGBF(nn.Module):
    """Modulated 1x1 projection to RGB + bias + running skip image (models.py:628-655)."""

    def __init__(self, in_channel, style_dim, upsample=True, blur_kernel=[1, 3, 3, 1], skip=False):
        super().__init__()
        if upsample:
            self.upsample = Upsample(blur_kernel)
        self.conv = ModulatedConv2d(in_channel, 3, 1, style_dim, demodulate=False)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))
        self.skip = skip

    def forward(self, d):
        if d.get('fused_rgb') is not None:          # already computed in the epilogue of the last styled conv
            return DataBag(d, output=d.fused_rgb, fused_rgb=None)
        skip = d.get('output') if self.skip else None
        if isinstance(skip, hip.HalfSkip) and d.get('rgb_partials') is None:
            skip = _full_size(skip)                 # only rgb_combine upsamples the skip itself
        if _double('ToRGBF', d.fmap, weight=self.conv.weight, bias=self.bias, style=d.style,
                   skip=skip.image if isinstance(skip, hip.HalfSkip) else skip):
            return self._forward_f64(d)
        if torch.is_tensor(skip) and tuple(skip.shape[2:]) != tuple(d.fmap.shape[2:]):
            up = self.upsample if hasattr(self, 'upsample') else Upsample([1, 3, 3, 1]).to(skip.device)
            if _rgb_stream() is None:
                skip = up(skip)
            else:
                with torch.cuda.stream(_rgb_stream()):
                    skip = up(skip)
        conv = self.conv
        side = _rgb_stream()
        partials = d.get('rgb_partials')
        if partials is not None:                    # the producing convolution left this ToRGB's channel sums
            if side is None:
                raise RuntimeError('ToRGB partial sums outside the forward that produces them')
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = hip.rgb_combine(partials, self.bias.view(3), skip)
            _running.keep.append((partials,))
            nd = DataBag(d, output=out)
            nd.pop('rgb_partials', None)        # bags that callers see never carry the key
            return nd
        if side is None:
            style = conv.modulation(d.style)
            weight, bias = conv.weight.view(3, conv.in_channel), self.bias.view(3)
            if grad.records(d.fmap, weight, style, bias, skip):
                out = grad.ToRGB.apply(d.fmap, weight, style, bias, skip, conv.scale)
            else:
                out = hip.to_rgb(d.fmap, weight, style, bias, skip, conv.scale)
            return DataBag(d, output=out)
        ahead = _prefetched(self)
        side.wait_stream(torch.cuda.current_stream())      # the feature map and the latent come from the trunk
        with torch.cuda.stream(side):
            out = hip.to_rgb(d.fmap, conv.weight.view(3, conv.in_channel), _style_of(self, ahead, d.style),
                             self.bias.view(3), skip, conv.scale)
        _running.keep.append((d.fmap, d.style))         # read on the side stream: referenced until the join
        return DataBag(d, output=out)

    def _forward_f64(self, d):
        """The double form: the running image (upsampled here if it is smaller), the style, ToRGB -- on the caller's
        stream."""
        conv = self.conv
        skip = d.output if self.skip else None
        if skip is not None and tuple(skip.shape[2:]) != tuple(d.fmap.shape[2:]):
            up = self.upsample if hasattr(self, 'upsample') else Upsample([1, 3, 3, 1]).to(skip.device).double()
            skip = up(skip)
        style = conv.modulation(d.style)
        out = hip.to_rgb_f64(d.fmap, conv.weight.view(3, conv.in_channel), style, self.bias.view(3), skip, conv.scale)
        return DataBag(d, output=out)


# ------------------------------------------------------------------------------------------
# containers
# ------------------------------------------------------------------------------------------

class ModulatedConv2dSeq(nn.Sequential):
    """modulation -> adain -> dconv [-> blur], explicitly separated so that the learned linear
    convolution can be rewritten as an associative memory (models.py:259-289)."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, demodulate=True,
                 upsample=False, blur_kernel=[1, 3, 3, 1]):
        self.eps = 1e-8
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.upsample = upsample
        steps = [
            ('modulation', EqualLinearS(style_dim, in_channel, bias_init=1)),
            ('adain', ApplyStyle()),
            ('dconv', DemodulatedConv2dF(in_channel, out_channel, kernel_size,
                                         demodulate=demodulate, upsample=upsample)),
        ]
        if upsample:
            factor = 2
            p = (len(blur_kernel) - factor) - (kernel_size - 1)
            steps.append(('blur', BlurF(blur_kernel, pad=((p + 1) // 2 + factor - 1, p // 2 + 1),
                                        upsample_factor=factor)))
        super().__init__(OrderedDict(steps))


class StyledConvSeq(nn.Sequential):
    """mconv -> noise -> activate (models.py:232-257).  When nothing inside is hooked the block
    runs fused; otherwise child by child, so hooks and splits observe reference semantics."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, upsample=False,
                 blur_kernel=[1, 3, 3, 1], demodulate=True, mconv=None):
        assert mconv in [None, 'seq', 'fast']
        conv_cls = ModulatedConv2dSeq if mconv == 'seq' else ModulatedConv2dF
        super().__init__(OrderedDict([
            ('mconv', conv_cls(in_channel, out_channel, kernel_size, style_dim, upsample=upsample,
                               blur_kernel=blur_kernel, demodulate=demodulate)),
            ('noise', NoiseInjectionF()),
            ('activate', FusedLeakyReLUF(out_channel)),
        ]))

    def _fusable(self, d=None):
        if not fusion_enabled() or set(self._modules) != {'mconv', 'noise', 'activate'}:
            return False
        if d is not None and torch.is_tensor(d.get('fmap')) and d.fmap.dtype is _F64:
            return False            # the double path runs module by module (the fused kernels are float32)
        if torch.is_grad_enabled() and (
                any(p.requires_grad for p in self.parameters())     # dconv weight, modulation, noise strength, act bias
                or (d is not None and any(torch.is_tensor(t) and t.requires_grad for t in (d.get('fmap'), d.get('style'),
                                                                                           d.get('latent'))))):
            # somebody may differentiate through this layer (an `insert` whose target spans it, rewrite/ganrewrite.py:
            # 265-283; a linear_insert that froze every parameter and edits a layer in FRONT of this one: then only
            # the incoming map carries the graph): module by module, where every step carries its adjoint (grad.py) --
            # the fused path calls raw-pointer kernels that record no grad_fn.  Image generation and the statistics
            # sweeps run under no_grad and never come here.
            return False
        mconv = self.mconv
        if not isinstance(mconv, ModulatedConv2dSeq):
            return False
        want = {'modulation', 'adain', 'dconv'} | ({'blur'} if mconv.upsample else set())
        if set(mconv._modules) != want:
            return False
        return _unhooked(mconv, self.noise, self.activate, *mconv._modules.values())

    def _standard_activation(self):
        act = self.activate
        return act.negative_slope == 0.2 and abs(act.scale - 2 ** 0.5) <= 1e-12         # what the kernels' epilogues compute

    def _module_by_module(self, d):
        if d.get('prescaled') is not None:
            raise RuntimeError('a pre-scaled feature map reached a layer that runs module by module')
        return super().forward(d)

    def _route(self, ctx, h, w):
        """The route of this layer's convolution when the block runs fused on a map of h x w."""
        mconv = self.mconv
        return mconv.dconv.route(ctx, h, w, mconv.blur if mconv.upsample else None)

    def forward(self, d):
        # ONE reading of the RW_* switches per layer where no generator forward took one (a sliced model: the sweeps)
        with _scope(switches=_switches()):
            return self._forward(d)

    def _forward(self, d):
        received = d                # with the hand-over key, if any: what a re-entry must see
        pre = d.get('prescaled')
        if not self._fusable(d):
            return self._module_by_module(d)
        # `pre`: the layer in front already multiplied this layer's style into fmap (and computed it)
        ahead = _prefetched(self)
        style = pre if pre is not None else _style_of(self, ahead, d.style)
        demod = ahead[1] if ahead is not None else None        # else: computed in front of the launch (dconv.demod_factors)
        if not self._standard_activation():
            return self._module_by_module(d)
        fmap, dconv = d.fmap, self.mconv.dconv
        sw, ctx = _switches(), _context(fmap)
        x_amax = None if sw.mm_no_handover else _amax_of(fmap)      # the producer's bound on |fmap|, if it left one
        if pre is not None:         # bags that callers see never carry the key
            d = DataBag(d)
            d.pop('prescaled', None)
        if self.mconv.upsample:
            if pre is not None:
                raise RuntimeError('a pre-scaled feature map reached an upsampling layer')
            return self._run_upsampling(d, style, demod, ctx, x_amax)
        b, _, h, w = fmap.shape
        epilogue = dict(noise=self.noise.noise_for(d, b, h, w, fmap.device), noise_w=self.noise.weight, bias=self.activate.bias,
                        act=True)
        fin = _running.final
        if fin is not None and fin[0] is self:
            final = routing.final_rgb_route(sw, ctx, dconv.in_channel, dconv.out_channel, h, w)
            if final is not None:
                return self._run_final(d, style, demod, x_amax, pre is None, epilogue, final, received)
        return self._run_stride1(d, style, demod, ctx, x_amax, pre is None, epilogue)

    def _result_bound(self, ctx, fmap, height, width):
        """A buffer for the bound of the result where its reader takes one (inside the un-hooked forward only), else None."""
        reader = _running.neighbours.get(id(self), _NO_NEIGHBOURS).reader
        if (reader is None or routing.matrix_mode(_switches(), True) != 'split' or not reader._fusable()
                or not reader._route(ctx, height, width).reads_bound):
            return None
        return hip.new_bound(fmap.shape[0] * self.mconv.dconv.out_channel * height * width, fmap.device)

    def _run_upsampling(self, d, style, demod, ctx, x_amax):
        """One launch where route.runs_layer, else two passes.  Hands over the result's bound (on the tensor) and `prescaled`."""
        fmap, dconv, fir = d.fmap, self.mconv.dconv, self.mconv.blur.kernel
        route = self._route(ctx, fmap.shape[2], fmap.shape[3])
        h, w = 2 * fmap.shape[2], 2 * fmap.shape[3]
        # inside the un-hooked forward the result has one reader, the next styled convolution: where that one runs F(4x4,3x3)
        # (vector-bound beside its MFMAs) its style multiply, 18 packed multiplies per 6x6 item, moves into this epilogue
        post = None
        nxt = _running.neighbours.get(id(self), _NO_NEIGHBOURS).successor
        if (nxt is not None and nxt[0]._fusable() and nxt[0]._standard_activation()
                and not nxt[0].mconv.upsample and nxt[0]._route(ctx, h, w).prescaled):
            post = _style_of(nxt[0], _prefetched(nxt[0]), d.latent, nxt[1])
        noise = self.noise.noise_for(d, fmap.shape[0], h, w, fmap.device)
        y_amax = self._result_bound(ctx, fmap, h, w)
        if route.runs_layer and not route.split:
            y_amax = None               # allocated and dropped: the fp32 phase kernel neither reads nor reports a bound
        bound = dict(y_amax=y_amax) if y_amax is not None else {}
        if route.runs_layer:
            bound.update(dict(x_amax=x_amax) if route.split else {})
            out = dconv.run_whole_layer(fmap, style, route, fir, demod, noise=noise, post_scale=post, **bound,
                                        noise_w=self.noise.weight, bias=self.activate.bias, act=True)
        else:
            wide = dconv.run(fmap, style, style_on_load=True, demod=demod, x_amax=x_amax, route=route)
            out = hip.blur_noise_act(wide, fir, noise, self.noise.weight, self.activate.bias, post_scale=post, **bound)
        if y_amax is not None:
            out.rw_amax = (y_amax, out._version)
        return DataBag(d, style=style, fmap=out, **({} if post is None else dict(prescaled=post)))

    def _run_final(self, d, style, demod, x_amax, style_on_load, epilogue, route, received):
        """The last layer of the un-hooked generator, ToRGB in its epilogue: the map is never written.  Hands over `fused_rgb`."""
        _, torgb, idx = _running.final
        skip = d.output if torgb.skip else None
        if isinstance(skip, hip.HalfSkip) and route.kernel not in ('wino4', 'wino4_split'):
            skip = _full_size(skip)                 # only the F(4x4) epilogues upsample the skip themselves
        if torch.is_tensor(skip) and tuple(skip.shape[2:]) != tuple(d.fmap.shape[2:]):
            with _scope(final=None):        # not fused after all: as the bag came, before anything was launched
                return self.forward(received)
        main = torch.cuda.current_stream()          # this form needs a device: without one it raises here, nothing launched
        if _running.stream is not None:
            main.wait_stream(_running.stream)       # the running image comes from the RGB stream
        rgb_style = _style_of(torgb, _prefetched(torgb), d.latent, idx)
        to_rgb = (torgb.conv.weight.view(3, torgb.conv.in_channel), rgb_style, torgb.bias.view(3), skip, torgb.conv.scale)
        _, rgb = self.mconv.dconv.run(d.fmap, style, style_on_load, demod=demod, x_amax=x_amax, to_rgb=to_rgb, route=route,
                                      **epilogue)
        return DataBag(d, style=style, fmap=None, fused_rgb=rgb)

    def _run_stride1(self, d, style, demod, ctx, x_amax, style_on_load, epilogue):
        """The stride-1 layer in one launch.  Hands over the bound of its result (on the tensor) and `rgb_partials`."""
        fmap, (h, w) = d.fmap, d.fmap.shape[2:]
        route = self._route(ctx, h, w)
        y_amax = self._result_bound(ctx, fmap, h, w) if route.reports_bound else None
        # the ToRGB that reads the result (to_rgbK follows layer 2K): the direct-sum kernel leaves its channel sums itself
        tr = _running.neighbours.get(id(self), _NO_NEIGHBOURS).torgb if route.rgb_partials else None
        rgb = None
        if tr is not None:
            torgb, idx = tr
            rgb_style = _style_of(torgb, _prefetched(torgb), d.latent, idx)
            rgb = (torgb.conv.weight.view(3, torgb.conv.in_channel), rgb_style, torgb.conv.scale)
        out = self.mconv.dconv.run(fmap, style, style_on_load, demod=demod, x_amax=x_amax, y_amax=y_amax, rgb=rgb,
                                   route=route, **epilogue)
        extra = {}
        if rgb is not None:
            out, extra['rgb_partials'] = out
        if y_amax is not None:
            out.rw_amax = (y_amax, out._version)
        return DataBag(d, style=style, fmap=out, **extra)


class SeqStyleGAN2(nn.Sequential):
    """The whole generator as named sequential steps (models.py:31-141): bag_in, style, latents,
    noises, input, layer2, to_rgb1, then per resolution up_rgbK, layer(2j+1), layer(2j+2),
    to_rgbK, and output."""

    def __init__(self, size, style_dim, n_mlp, channel_multiplier=2, blur_kernel=[1, 3, 3, 1],
                 lr_mlp=0.01, truncation=1.0, mconv=None, bag_input=False, bag_output=False):
        self.size = size
        self.style_dim = style_dim
        self.mconv = mconv
        self.bag_input = bag_input
        self.bag_output = bag_output
        cm = channel_multiplier
        self.channels = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm,
                         256: 64 * cm, 512: 32 * cm, 1024: 16 * cm}
        self.log_size = int(math.log(size, 2))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.n_latent = self.log_size * 2 - 2

        def styled(cin, cout, upsample=False):
            return StyledConvSeq(cin, cout, 3, style_dim, upsample=upsample,
                                 blur_kernel=blur_kernel, mconv=mconv)

        def picked(index, name, module):
            return nn.Sequential(OrderedDict([('lat%d' % index, PickLatent(index)), (name, module)]))

        mapping = [PixelNormL()] + [
            EqualLinearL(style_dim, style_dim, lr_mul=lr_mlp, activation='fused_lrelu')
            for _ in range(n_mlp)]
        c4 = self.channels[4]
        steps = [] if bag_input else [('bag_in', InputLatent())]
        steps += [
            ('style', nn.Sequential(*mapping)),
            ('latents', AdjustLatent(self.n_latent, truncation)),
            ('noises', FixedNoiseBuffers(self.num_layers, 1, replace_input=False)),
            ('input', ConstantInputF(c4)),
            ('layer2', picked(0, 'conv', styled(c4, c4))),
            ('to_rgb1', picked(1, 'rgb', ToRGBF(c4, style_dim, upsample=False))),
        ]
        cin, lat = c4, 1
        for level in range(3, self.log_size + 1):
            cout = self.channels[2 ** level]
            steps += [
                ('up_rgb%d' % (level - 2), UpsampleO()),
                ('layer%d' % (lat + 2), picked(lat, 'sconv', styled(cin, cout, upsample=True))),
                ('layer%d' % (lat + 3), picked(lat + 1, 'sconv', styled(cout, cout))),
                ('to_rgb%d' % (level - 1),
                 picked(lat + 2, 'rgb', ToRGBF(cout, style_dim, skip=True, upsample=False))),
            ]
            cin, lat = cout, lat + 2
        if not bag_output:
            steps.append(('output', ReturnOutput()))
        super().__init__(OrderedDict(steps))

    def _checked_f64(self, input):
        """True when this forward runs in double.  A float64 input into a float32 model, or the other way round, raises
        here -- before anything is launched -- and so does a double forward that would have to record a graph."""
        t = input if torch.is_tensor(input) else input.get('latent') if isinstance(input, dict) else None
        own = next(self.parameters(), None)
        if not torch.is_tensor(t) or own is None or (t.dtype is not _F64 and own.dtype is not _F64):
            return False
        if t.dtype != own.dtype:
            raise RuntimeError('rewriting_amd: SeqStyleGAN2: the input is %s and the model\'s parameters are %s -- cast the '
                               'model and its input to one dtype, .float() or .double() (nothing is converted)'
                               % (t.dtype, own.dtype))
        if isinstance(input, dict) and torch.is_tensor(input.get('noise')) and input['noise'].dtype != own.dtype:
            raise RuntimeError('rewriting_amd: SeqStyleGAN2: the noise handed in is %s and the model\'s parameters are %s '
                               '(nothing is converted)' % (input['noise'].dtype, own.dtype))
        graph = [m.weight for m in self.modules() if isinstance(m, (DemodulatedConv2dF, NoiseInjectionF))]
        _forward_only_f64('SeqStyleGAN2', t, *graph)
        return True

    def _records_graph(self, input):
        """True when this forward has to leave a graph from the image back to the latent, the mapping network, a
        modulation, a ToRGB or the constant input: the adjoints that exist for a loss on the image (grad.py, second
        half).  Nothing else changes the way the generator runs: under torch.no_grad() this is False at once, and a model
        in which only parameters of the styled convolutions proper (dconv weight, noise strength, activation bias)
        require a gradient keeps the forward it had -- the layers concerned already run module by module
        (StyledConvSeq._fusable), and the image carries no graph."""
        if not torch.is_grad_enabled():
            return False
        t = input if torch.is_tensor(input) else input.get('latent') if isinstance(input, dict) else None
        if torch.is_tensor(t) and t.requires_grad:
            return True
        for m in self.modules():
            own = isinstance(m, (EqualLinear, ConstantInputF, ToRGBF)) or \
                (isinstance(m, ModulatedConv2d) and m.kernel_size == 1)
            if own and any(p.requires_grad for p in m.parameters(recurse=False)):
                return True
        return False

    def forward(self, input):
        if self._checked_f64(input):
            return super().forward(input)       # module by module: no side stream, no micro-batching
        with _scope(switches=switches()):       # ONE reading of the RW_* switches per forward
            if self._records_graph(input):
                # module by module on the caller's stream: no RGB side stream, no style prefetch, no micro-batches, no
                # ToRGB sums left by a convolution -- every step is then a Function of grad.py / op/ (or a fused block
                # none of whose own parameters and inputs requires a gradient: StyledConvSeq._fusable), and autograd
                # replays them on this one stream
                return super().forward(input)
            whole = (fusion_enabled() and torch.is_tensor(input) and not self.bag_output and not self.bag_input
                     and not _running.image_path and _unhooked(*self.modules()))
            if not whole:
                return self._forward(input)
            topology = self._topology()
            with _scope(image_path=True, neighbours=topology[0]):
                return self._forward(input, topology)

    def _forward(self, input, topology=None):
        mb, from_res = micro_batch()
        micro = (mb and fusion_enabled() and torch.is_tensor(input) and not self.bag_output
                 and not self.bag_input and input.shape[0] > mb and 'up_rgb%d' % (int(math.log2(from_res)) - 2)
                 in self._modules and _running.stream is None and _unhooked(*self.modules()))
        side_ok = (not micro and fusion_enabled() and _switches().rgb_stream and torch.is_tensor(input)
                   and input.is_cuda and not self.bag_output and _running.stream is None
                   and not torch.cuda.is_current_stream_capturing()
                   and _unhooked(*self.modules()))
        if not micro and not side_ok:
            return super().forward(input)
        final = (topology or self._topology())[1] if _switches().fuse_final_rgb else None
        if micro:
            return self._forward_micro(input, mb, from_res, final)
        with contextlib.ExitStack() as scopes:
            main = scopes.enter_context(_side_streams_joined(input.device))
            # the running image travels at half size between up_rgbK and the ToRGB that reads it only where nothing
            # looks into the bags on the way: a forward hook of torch's on any module would
            inline_up = (_running.image_path and _switches().rgb_inline_up
                         and not any(m._forward_hooks or m._forward_pre_hooks for m in self.modules()))
            scopes.enter_context(_scope(final=final, inline_up=inline_up))
            out = input
            for name, module in self._modules.items():
                out = module(out)
                if name == 'latents' and _running.image_path and _switches().prefetch_styles:
                    scopes.enter_context(_scope(**self._prefetch_modulations(out, _running.aux)))
        if torch.is_tensor(out):
            out.record_stream(main)
        return out

    def _forward_micro(self, z, mb, from_res, final):
        """The un-hooked generator on a large batch: the low-resolution steps on the whole batch (their launches
        need it to fill 256 CUs), the steps from resolution `from_res` up on `mb` images at a time, so that the
        feature maps handed from one kernel to the next (134 MB per image at 1024^2) are still in the 256 MB
        memory-side cache when the next kernel reads them instead of making a round trip through HBM.  The slices
        reuse the same allocator blocks, image rows keep their noise rows (`batch_rows`), results are those of
        the one-launch path."""
        mods = list(self._modules.values())
        k = list(self._modules).index('up_rgb%d' % (int(math.log2(from_res)) - 2))
        d = z
        for m in mods[:k]:
            d = m(d)
        total = d.latent.shape[0]
        out = None
        with _scope(final=final):
            for s in range(0, total, mb):
                e = min(s + mb, total)
                part = DataBag({key: (v[s:e] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == total else v)
                                for key, v in d.items()})
                part['batch_rows'] = (s, total)
                for m in mods[k:]:
                    part = m(part)
                if out is None:
                    out = part.new_empty((total,) + tuple(part.shape[1:]))
                out[s:e] = part
                del part
        return out

    def _prefetch_modulations(self, d, aux):
        """Every styled convolution's style (EqualLinearS of its latent row) and demodulation factors, and every
        ToRGB's style, depend on the latents and the weights only: inside the un-hooked forward they are all computed
        HERE, right after the mapping network, on the auxiliary stream beside the 4x4 / 8x8 layers -- instead of as
        ~60 launches of a few microseconds each BETWEEN the large convolutions, where each one is a kernel boundary on
        the trunk and two of them (in front of layers 15 / 17) sat 0.3 - 0.6 ms behind the grid-stride workgroups of
        the RGB branch waiting for a wave slot (rocprofv3 trace of round 2).  The first layer's are computed inline
        (it needs them at once); the trunk waits for the rest at its first use (_prefetched).  Values are those of
        the per-layer path: same kernels, same inputs.  Returns the fields to install for the rest of the forward."""
        pre = {}
        todo = []
        for name, mod in self._modules.items():
            if not isinstance(mod, nn.Sequential) or isinstance(mod, StyledConvSeq):
                continue
            kids = list(mod.children())
            if len(kids) != 2 or not isinstance(kids[0], PickLatent):
                continue
            if isinstance(kids[1], StyledConvSeq) and kids[1]._fusable() and isinstance(kids[1].mconv, ModulatedConv2dSeq):
                todo.append((kids[0].index, kids[1]))
            elif isinstance(kids[1], ToRGBF):
                todo.append((kids[0].index, kids[1]))
        if len(todo) < 3:
            return {}
        main = torch.cuda.current_stream()
        aux.wait_stream(main)                       # the latents come from the trunk
        with torch.cuda.stream(aux):
            for index, mod in todo[2:]:
                lat = d.latent[:, index]
                if isinstance(mod, ToRGBF):
                    pre[id(mod)] = mod.conv.modulation(lat)
                else:
                    style = mod.mconv.modulation(DataBag(style=lat)).style
                    pre[id(mod)] = (style, mod.mconv.dconv.demod_factors(style))
        return dict(pre=pre, pre_join=aux)

    def _topology(self):
        """({id(StyledConvSeq): _Neighbours}, final) of this sequence as it stands now, from one walk of its steps (the
        rewriters edit sequences between forwards).  `final`: (last styled conv 'layer{num_layers+1}', the ToRGBF of
        the step 'to_rgb{log_size-1}' directly behind it, that step's latent index), or None.  A step's styled conv is
        its child 'sconv' ('layer2': 'conv', which only a reader or a ToRGB may follow); the step behind hands its
        latent index over where it has a single PickLatent -- as its first child for a successor, and as the first of
        exactly two, in front of the ToRGBF, for a ToRGB (models.py:126-131)."""
        near, final, prev = {}, None, None
        last = ('layer%d' % (self.num_layers + 1), 'to_rgb%d' % (self.log_size - 1))
        steps = list(self._modules.items())
        for (name, step), (nname, nstep) in zip(steps, steps[1:] + [(None, None)]):
            sconv = getattr(step, 'sconv', None)
            conv = sconv or getattr(step, 'conv', None)
            if not isinstance(conv, StyledConvSeq):
                continue
            if prev is not None:        # the ToRGB / up_rgb steps in between pass the feature map on untouched
                near[id(prev)] = near[id(prev)]._replace(reader=conv)
            prev = conv
            kids = list(nstep.children()) if nstep is not None else []
            picks = [m for m in kids if isinstance(m, PickLatent)]
            index = picks[0].index if len(picks) == 1 else None
            leads = index is not None and kids[0] is picks[0]
            nconv, rgb = getattr(nstep, 'sconv', None), getattr(nstep, 'rgb', None)
            successor = torgb = None
            if (conv is sconv and leads and isinstance(nconv, StyledConvSeq)
                    and getattr(conv.mconv, 'upsample', False) and not getattr(nconv.mconv, 'upsample', False)):
                successor = (nconv, index)
            if isinstance(rgb, ToRGBF):
                if leads and len(kids) == 2 and kids[1] is rgb:
                    torgb = (rgb, index)
                if conv is sconv and index is not None and (name, nname) == last:
                    final = (conv, rgb, index)
            near[id(conv)] = _Neighbours(None, successor, torgb)
        return near, final

    def bag_from_z(self, z):
        return InputLatent()(z)

    def output_from_bag(self, bag):
        return ReturnOutput()(bag)

    def load_state_dict(self, data, latent_avg=None, **kwargs):
        """Accepts this class's own keys, or a rosinality/stylegan2-pytorch generator
        checkpoint (``{'g_ema': ..., 'latent_avg': ...}`` or its ``g_ema`` dict), renaming
        keys the way the reference does (models.py:149-202)."""
        try:
            return super().load_state_dict(data, **kwargs)
        except Exception:
            pass
        if len(data) < 10 and 'g_ema' in data and 'latent_avg' in data:
            latent_avg = data['latent_avg']
            data = data['g_ema']
        converted = convert_rosinality_keys(data, seq=(self.mconv == 'seq'))
        current = self.state_dict()
        if latent_avg is not None:
            converted['latents.latent_avg'] = latent_avg
        elif 'latents.latent_avg' not in converted:
            if self.latents.truncation != 1.0:
                warnings.warn('Need to provide latent_avg to use truncation.')
            converted['latents.latent_avg'] = current['latents.latent_avg']
        for key in current:
            if key.startswith('noises') and key not in converted:
                converted[key] = current[key]
        return super().load_state_dict(converted, **kwargs)


_ROSINALITY_RULES = [
    (r'^conv1\.conv\.', lambda m: 'layer2.conv.mconv.'),
    (r'^conv1\.', lambda m: 'layer2.conv.'),
    (r'^convs\.(\d+)\.conv', lambda m: 'layer%d.sconv.mconv' % (int(m.group(1)) + 3)),
    (r'^convs\.(\d+)\.', lambda m: 'layer%d.sconv.' % (int(m.group(1)) + 3)),
    (r'^to_rgb1\.(conv\.|bias$)', lambda m: 'to_rgb1.rgb.%s' % m.group(1)),
    (r'^to_rgbs\.(\d+)\.upsample\.', lambda m: 'up_rgb%d.' % (int(m.group(1)) + 1)),
    (r'^to_rgbs\.(\d+)\.', lambda m: 'to_rgb%d.rgb.' % (int(m.group(1)) + 2)),
]


def convert_rosinality_keys(data, seq=True):
    out = {}
    for key, value in data.items():
        for pattern, repl in _ROSINALITY_RULES:
            key = re.sub(pattern, repl, key)
        if seq:
            key = re.sub(r'mconv\.weight$', 'mconv.dconv.weight', key)
        else:
            key = re.sub(r'mconv\.dconv\.weight$', 'mconv.weight', key)
        out[key] = value
    return out
