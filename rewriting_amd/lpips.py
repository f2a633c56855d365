"""LPIPS (v0.1, ``net-lin``, ``vgg``) on the HIP kernels: the perceptual distance of the reference's edit tables.

The reference wraps ``models.PerceptualLoss(model='net-lin', net='vgg', spatial=True)`` of the PerceptualSimilarity submodule
(metrics/distances.py:18-59) and reduces its per-pixel map with a mask, ``sum(loss * w) / sum(w)``.  The submodule is not needed:
the arithmetic is

1. images in [-1, 1]; ``x' = (x - shift[c]) / scale[c]`` with ``shift = (-.030, -.088, -.188)``, ``scale = (.458, .448, .450)``;
2. torchvision's ``vgg16().features[:30]``; the five taps are the ReLU outputs before each pool (features 3, 8, 15, 22, 29:
   64, 128, 256, 512, 512 channels at H, H/2, H/4, H/8, H/16);
3. per tap and pixel ``d_k = sum_c lin_k[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2`` (``hip.lpips_tap``);
4. ``spatial=True``: the sum of the ``d_k`` up-sampled to (H, W), bilinear, ``align_corners=False``; ``spatial=False``: the sum
   of their means; with a weight ``w``: ``sum(out * w) / sum(w)`` per image (``hip.lpips_combine``).

``LPIPS`` is built from a ``perceptual.VGG16Features`` -- whose nine blocks it reuses -- and four more blocks (21 with its
pool, 24, 26, 28).  The two images' networks run block by block side by side, and a tap is dropped as soon as its ``d_k``
exists; maps narrower than 32 take the split-K form of the direct sum (SPLIT_K below).  float32 on a HIP device only.
``forward`` is the metric and refuses gradients; ``loss`` is the same value per image as a LOSS, differentiable to its first
image (``hip.lpips_combine_grad``, ``hip.lpips_tap_grad`` and the blocks' adjoints to their inputs, one autograd node for
the whole metric), against a ``target`` whose taps are computed once; ``OverfitTerm`` is that loss as the perceptual term
of ``all_weights_insert``.  No weights ship: ``lpips_vgg(vgg_path, lin_path)`` loads a torchvision VGG16 state dict and the ``lin`` layers
of LPIPS v0.1 (``lin{k}.model.1.weight``); the environment variables ``RW_VGG16_WEIGHTS`` and ``RW_LPIPS_WEIGHTS`` name the
two files.
"""
import functools

import numpy
import torch
from torch import nn

from torch.autograd import Function

from . import hip, perceptual
from .utils.stylegan2 import grad

WEIGHTS_ENV = 'RW_LPIPS_WEIGHTS'
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# the convolutions past perceptual.LAYERS, same columns
TAIL_LAYERS = ((21, 512, 512, True), (24, 512, 512, False), (26, 512, 512, False), (28, 512, 512, False))
TAPS = (2, 7, 14, 21, 28)               # the convolutions whose activated maps LPIPS reads
CHANNELS = (64, 128, 256, 512, 512)
# Maps narrower than SPLIT_K_BELOW take the direct sum whose four waves split K (hip.conv3x3's impl 6, the form made for
# 4 x 4 .. 16 x 16 maps): a term's chain of additions is a quarter as long.  Against float64, 2-norm over whole maps
# (profiles/lpips_route_accuracy.json): 1.5e-7 .. 4.0e-7 where the serial direct sum has 2.9e-7 .. 8.0e-7 and F(2x2,3x3)
# 2.3e-7 .. 6.5e-7 -- and nearly equal pairs amplify the features' rounding by 1 / |n0 - n1|.
SPLIT_K = 6
SPLIT_K_BELOW = 32
MIN_SIZE = 16                           # four pools: a 16 x 16 image leaves 1 x 1 maps at the last tap


@functools.lru_cache(maxsize=256)
def upsample_table(n_in, n_out):
    """(i0, i1 int32, lam float64), each (n_out,): output sample o of ``F.interpolate(mode='bilinear', align_corners=False)``
    along an axis of n_in samples is ``(1 - lam[o]) * x[i0[o]] + lam[o] * x[i1[o]]``.  torch's arithmetic
    (upsample_bilinear2d) in float64: ``src = max((o + 0.5) * n_in / n_out - 0.5, 0)``, ``i0 = floor(src)``,
    ``i1 = min(i0 + 1, n_in - 1)``, ``lam = src - i0``.  The one place it lives; read-only arrays."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError('lpips.upsample_table: lengths must be positive, not %d -> %d' % (n_in, n_out))
    scale = n_in / n_out
    src = numpy.maximum((numpy.arange(n_out, dtype=numpy.float64) + 0.5) * scale - 0.5, 0.0)
    i0 = numpy.minimum(src.astype(numpy.int64), n_in - 1)
    i1 = numpy.minimum(i0 + 1, n_in - 1)
    lam = src - i0
    tables = (i0.astype(numpy.int32), i1.astype(numpy.int32), lam)
    for t in tables:
        t.setflags(write=False)
    return tables


@functools.lru_cache(maxsize=256)
def adjoint_table(n_in, n_out):
    """(lo, hi int32), each (n_in,): the outputs o of upsample_table(n_in, n_out) that read input i -- i0[o] == i or
    i1[o] == i -- are exactly lo[i] <= o < hi[i].  i0 and i1 do not decrease, and the outputs with i1 == i are those with
    i0 == i - 1 (and, at the last input, with i0 == i): two adjacent runs.  An input no output reads has lo == hi.  Read-only
    arrays."""
    i0, i1, _ = upsample_table(n_in, n_out)
    at = numpy.arange(int(n_in))
    lo0, hi0 = numpy.searchsorted(i0, at, 'left'), numpy.searchsorted(i0, at, 'right')
    lo1, hi1 = numpy.searchsorted(i1, at, 'left'), numpy.searchsorted(i1, at, 'right')
    lo = numpy.where(hi0 > lo0, numpy.where(hi1 > lo1, numpy.minimum(lo0, lo1), lo0), lo1)
    hi = numpy.where(hi0 > lo0, numpy.where(hi1 > lo1, numpy.maximum(hi0, hi1), hi0), hi1)
    tables = (lo.astype(numpy.int32), hi.astype(numpy.int32))
    for t in tables:
        t.setflags(write=False)
    return tables


_device_cache = {}


def _on_device(build, tap_sizes, size, device):
    """The arrays build(taps, H, W) makes on the host, as tensors on `device`: copied once per (build, sizes, device) and kept,
    64 entries per build -- then its cache starts again."""
    device = torch.device(device)
    h, w = int(size[0]), int(size[1])
    key = (tuple((int(a), int(b)) for a, b in tap_sizes), h, w, device.type, device.index)
    cache = _device_cache.setdefault(build, {})
    tables = cache.get(key)
    if tables is None:
        tables = tuple(torch.from_numpy(a).to(device) for a in build(key[0], h, w))
        if len(cache) >= 64:
            cache.clear()
        cache[key] = tables
    return tables


def _adjoint_arrays(taps, h, w):
    parts = []
    for hk, wk in taps:
        parts.extend(adjoint_table(hk, h) + adjoint_table(wk, w))
    return (numpy.concatenate(parts),)


def _forward_arrays(taps, h, w):
    idx = numpy.empty((len(taps), 2 * h + 2 * w), dtype=numpy.int32)
    lam = numpy.empty((len(taps), h + w), dtype=numpy.float32)
    for k, (hk, wk) in enumerate(taps):
        y0, y1, ly = upsample_table(hk, h)
        x0, x1, lx = upsample_table(wk, w)
        idx[k] = numpy.concatenate([y0, y1, x0, x1])
        lam[k] = numpy.concatenate([ly, lx]).astype(numpy.float32)
    return idx, lam


def device_adjoint_tables(tap_sizes, size, device):
    """int32 (2 sum_k (h_k + w_k),) on `device`, as rw_lpips_combine_grad_f32 reads it: tap after tap the rows' lo, the rows'
    hi, the columns' lo, the columns' hi of adjoint_table.  Copied once per (sizes, device)."""
    return _on_device(_adjoint_arrays, tap_sizes, size, device)[0]


def device_tables(tap_sizes, size, device):
    """(idx int32 (K, 2H + 2W), lam float32 (K, H + W)) on `device` for taps of tap_sizes = ((h_k, w_k), ...) up-sampled to
    size = (H, W), as rw_lpips_combine_f32 reads them: per tap the rows' i0 and i1, then the columns'; the rows' lam, then the
    columns' -- rounded to float32 here, once.  Copied once per (sizes, device)."""
    return _on_device(_forward_arrays, tap_sizes, size, device)


class Target:
    """The constant side of ``LPIPS.loss``: the five tap maps of an image batch (B or 1) and the image's size.  Made by
    ``LPIPS.target`` once, read by every iteration."""

    def __init__(self, taps, size):
        self.taps, self.size = tuple(taps), (int(size[0]), int(size[1]))

    @property
    def batch(self):
        return self.taps[0].shape[0]

    @property
    def device(self):
        return self.taps[0].device


def _evaluate(net, im0, target, w, spatial, keep):
    """(value (B,), the thirteen activated maps of im0 where keep, else [], what the backward needs of the reduction):
    forward's walk for im0 and forward's reduction, against the taps of `target`."""
    ds, saved = [], []
    for index, y0 in net._walk(im0, 'all'):
        if index in TAPS:
            ds.append(hip.lpips_tap(y0, target.taps[len(ds)], net.lins[len(ds)]))
        if keep:
            saved.append(y0)
        del y0
    value, total = _reduce(ds, (im0.shape[2], im0.shape[3]), w, spatial, want_map=False)
    return value, saved, total


def _reduce(ds, size, w, spatial, want_map):
    """(value, the weights' sums (B,) the backward divides by, or None where there are none) of the five d_k for an image of
    size = (H, W).  spatial: the map (B, 1, H, W) where want_map, else ``sum(map * w) / sum(w)`` per image (w None: ones), which
    never writes the map.  Not spatial: the sum of the taps' means, (B, 1, 1, 1) where want_map and w is None, else (B,), under
    w as the 1 x 1 map it is."""
    device, sizes = ds[0].device, tuple((d.shape[1], d.shape[2]) for d in ds)
    if spatial:
        out, sums = hip.lpips_combine(ds, device_tables(sizes, size, device), size, weight=w, want_map=want_map,
                                      want_sums=not want_map)
        return (out, None) if want_map else (sums[:, 0] / sums[:, 1], sums[:, 1])
    out = 0
    for d, own in zip(ds, sizes):                               # the same entry at the tap's own size: (sum d_k, pixels)
        _, sums = hip.lpips_combine([d], device_tables((own,), own, device), own, want_map=False, want_sums=True)
        out = out + sums[:, 0] / sums[:, 1]
    if w is None:
        return (out.view(-1, 1, 1, 1) if want_map else out), None
    _, sums = hip.lpips_combine([out.view(-1, 1, 1).contiguous()], device_tables(((1, 1),), size, device), size, weight=w,
                                want_map=False, want_sums=True)
    return sums[:, 0] / sums[:, 1], sums[:, 1]


class _LossFunction(Function):
    """The whole metric as one node: saves im0's thirteen activated maps (five of them are the taps) and the weights' sums."""

    @staticmethod
    def forward(ctx, im0, net, target, w, spatial, trace):
        value, saved, total = _evaluate(net, im0, target, w, spatial, keep=True)
        if trace is not None:
            trace.extend(saved)
        ctx.net, ctx.target, ctx.w, ctx.spatial, ctx.total = net, target, w, spatial, total
        ctx.save_for_backward(*saved)
        return value

    @staticmethod
    def backward(ctx, g):
        net, target, w = ctx.net, ctx.target, ctx.w
        saved = ctx.saved_tensors
        b, _, h, wd = saved[0].shape
        device = saved[0].device
        sizes = tuple((saved[n].shape[2], saved[n].shape[3]) for n, (index, _) in enumerate(net.blocks()) if index in TAPS)
        g = g.detach().to(torch.float32).contiguous()
        if ctx.spatial:
            gds = hip.lpips_combine_grad(sizes, device_tables(sizes, (h, wd), device), device_adjoint_tables(sizes, (h, wd), device),
                                         (h, wd), g / ctx.total, weight=w)
        else:
            if w is not None:                                   # the 1 x 1 map of the taps' means under the weight
                one = ((1, 1),)
                g = hip.lpips_combine_grad(one, device_tables(one, (h, wd), device), device_adjoint_tables(one, (h, wd), device),
                                           (h, wd), g / ctx.total, weight=w)[0].view(b)
            gds = [hip.lpips_combine_grad((size,), device_tables((size,), size, device),
                                          device_adjoint_tables((size,), size, device), size, g / (size[0] * size[1]))[0]
                   for size in sizes]
        gx, k = None, len(sizes)
        for (index, block), y in reversed(list(zip(net.blocks(), saved))):
            gy = None if gx is None else hip.bias_relu_pool_grad(gx, y, pooled=block.pool)
            if index in TAPS:
                k -= 1
                gy = hip.lpips_tap_grad(y, target.taps[k], net.lins[k], gds[k], acc=gy, relu_mask=True, out=gy)
            gx = block.conv_input_grad(gy)
        return gx / net.scale, None, None, None, None, None


class LPIPS(nn.Module):
    """``forward(im0, im1, w=None, spatial=True)``: LPIPS v0.1 (vgg) of images in [-1, 1], (B, 3, H, W) float32 on a HIP device;
    im1 may have batch 1 (its network then runs once).  The parameters are ``features.N.*`` (the VGG16Features handed in),
    ``tail.N.*`` (N = 21, 24, 26, 28) and ``lins.k`` (C_k,); all frozen."""

    def __init__(self, features=None):
        super().__init__()
        self.features = features if features is not None else perceptual.VGG16Features()
        if not isinstance(self.features, perceptual.VGG16Features):
            raise TypeError('rewriting_amd: LPIPS is built from a perceptual.VGG16Features, not %s' % type(features).__name__)
        self.tail = nn.ModuleDict({str(index): perceptual._Block(in_ch, out_ch, pool) for index, in_ch, out_ch, pool in TAIL_LAYERS})
        self.lins = nn.ParameterList([nn.Parameter(torch.zeros(c), requires_grad=False) for c in CHANNELS])
        self.register_buffer('shift', torch.tensor(SHIFT).view(1, 3, 1, 1), persistent=False)
        self.register_buffer('scale', torch.tensor(SCALE).view(1, 3, 1, 1), persistent=False)

    def blocks(self):
        """[(index in torchvision's features, block)]: the thirteen convolutions of features[:30]"""
        head = [(index, block) for (index, _, _, _), block in zip(perceptual.LAYERS, self.features.blocks())]
        return head + [(index, self.tail[str(index)]) for index, _, _, _ in TAIL_LAYERS]

    def _walk(self, im, keep):
        """Yields (index, y) block by block: the image's network, one block per step.  keep = 'taps': y is the activated map at
        the five taps and whatever costs nothing elsewhere; 'all': at every block.  The walk holds no reference to a y it has
        handed over: a map dies when its reader drops it."""
        x = (im.detach() - self.shift) / self.scale             # not foldable into layer 0: its zero padding comes after
        for index, block in self.blocks():
            impl = SPLIT_K if x.shape[3] < SPLIT_K_BELOW else None
            y, x = block.activate(x, keep=keep == 'all' or index in TAPS, impl=impl)
            y = [y]                                             # popped as it is handed over: nothing of it stays in this frame
            yield index, y.pop()

    def _check(self, im0, im1, w):
        perceptual._check_images(self, {'im0': im0, 'im1': im1}, pools=4)
        for name, im in (('im0', im0), ('im1', im1)):
            if im.requires_grad and torch.is_grad_enabled():
                raise RuntimeError('rewriting_amd: LPIPS is forward only (the reference uses it under no_grad, as a metric): %s '
                                   'requires a gradient -- call it under torch.no_grad() or detach the image' % name)
        b, _, h, wd = im0.shape
        if tuple(im1.shape[1:]) != (3, h, wd) or im1.shape[0] not in (1, b) or im1.device != im0.device:
            raise ValueError('rewriting_amd: LPIPS: im1 is %s on %s, im0 %s on %s -- the sizes must match, im1\'s batch may be 1'
                             % (tuple(im1.shape), im1.device, tuple(im0.shape), im0.device))
        if w is not None:
            if not isinstance(w, torch.Tensor) or w.dim() != 4 or tuple(w.shape[1:]) != (1, h, wd) or w.shape[0] not in (1, b):
                raise ValueError('rewriting_amd: LPIPS: the weight must be (B or 1, 1, H, W) = (%d or 1, 1, %d, %d), not %s'
                                 % (b, h, wd, tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__))
            if not hip.on_device(w) or w.device != im0.device:
                raise RuntimeError('rewriting_amd: LPIPS: the weight is on %s, the images on %s (there is no CPU fallback)'
                                   % (w.device, im0.device))
            if w.dtype != torch.float32:
                raise RuntimeError('rewriting_amd: LPIPS: the weight is %s; the metric is fp32 only -- cast with .float()' % w.dtype)

    def forward(self, im0, im1, w=None, spatial=True, taps=None):
        """spatial=True: (B, 1, H, W), the per-pixel distance; spatial=False: (B, 1, 1, 1), the sum of the taps' means; with
        w (B or 1, 1, H, W): (B,), ``sum(out * w, [1, 2, 3]) / sum(w, [1, 2, 3])`` (metrics/distances.py:49-56) -- the map is
        then never written.  taps: a list that receives the five d_k (B, h_k, w_k)."""
        self._check(im0, im1, w)
        with torch.no_grad():
            ds, second = [], self._walk(im1, 'taps')
            for index, y0 in self._walk(im0, 'taps'):           # side by side, y0 then y1 (a zip would hold on to its last pair)
                y1 = next(second)[1]
                if index in TAPS:
                    ds.append(hip.lpips_tap(y0, y1, self.lins[len(ds)]))
                del y0, y1                                      # a tap lives until its d_k exists
            del second
            if taps is not None:
                taps.extend(ds)
            return _reduce(ds, (im0.shape[2], im0.shape[3]), w, spatial, want_map=w is None)[0]

    def target(self, im1):
        """The taps of im1 (B or 1, 3, H, W) as a ``Target``: its network runs here, once, under no_grad."""
        im1 = im1.detach() if isinstance(im1, torch.Tensor) else im1
        self._check(im1, im1, None)
        with torch.no_grad():
            taps = []
            for index, y1 in self._walk(im1, 'all'):
                if index in TAPS:
                    taps.append(y1)
                del y1
        return Target(taps, im1.shape[2:])

    def loss(self, im0, target, w=None, spatial=True, trace=None):
        """(B,): LPIPS of im0 against `target` -- a ``Target`` or an image (B or 1, 3, H, W), whose taps are then computed
        here -- per image: with w (B or 1, 1, H, W) ``sum(out * w) / sum(w)`` of the spatial map, without it the map's mean;
        spatial=False: the sum of the taps' means.  The value is ``forward``'s, bit for bit (the same ``_walk`` and the same
        ``_reduce``).  Differentiable to im0 and to nothing else: the target, w and the parameters may not require a gradient.
        Under no_grad, or when im0 requires none, nothing is saved.  trace: a list that receives im0's thirteen activated
        maps (the ReLU and pool decisions of the device) when a gradient is recorded."""
        for name, t in (('the target', target), ('the weight', w)):
            if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
                raise RuntimeError('rewriting_amd: LPIPS.loss is differentiable to im0 only: %s requires a gradient -- detach it'
                                   % name)
        if not isinstance(target, Target):
            target = self.target(target)
        plain = im0.detach() if isinstance(im0, torch.Tensor) else im0
        self._check(plain, plain, w)
        if target.size != tuple(im0.shape[2:]) or target.batch not in (1, im0.shape[0]) or target.device != im0.device:
            raise ValueError('rewriting_amd: LPIPS: the target holds %d image(s) of %d x %d on %s, im0 is %s on %s -- the sizes '
                             'must match, the target\'s batch may be 1'
                             % (target.batch, target.size[0], target.size[1], target.device, tuple(im0.shape), im0.device))
        if grad.records(im0):
            return _LossFunction.apply(im0, self, target, w, bool(spatial), trace)
        with torch.no_grad():
            return _evaluate(self, plain, target, w, bool(spatial), keep=False)[0]


class OverfitTerm:
    """``(gt, pred) -> weight * net.loss(pred, net.target(gt), spatial=spatial).mean()``: LPIPS as the perceptual term of
    ``all_weights_insert(..., perceptual=)``.  The target is kept for as long as gt stays the same memory at the same version
    and shape: the overfit loop hands the same image every iteration, and its network runs once."""

    def __init__(self, net, weight=1.0, spatial=False):
        if not isinstance(net, LPIPS):
            raise TypeError('rewriting_amd: OverfitTerm is built from an lpips.LPIPS, not %s' % type(net).__name__)
        self.net, self.weight, self.spatial = net, float(weight), bool(spatial)
        self._key = self._gt = self._target = None

    def __call__(self, gt, pred):
        key = (gt.data_ptr(), gt._version, tuple(gt.shape), tuple(gt.stride()))
        if key != self._key:
            self._key, self._gt, self._target = key, gt, self.net.target(gt)    # gt is held: its memory is not handed out again
        return self.weight * self.net.loss(pred, self._target, spatial=self.spatial).mean()


def _lin_weights(lin_sd):
    found = []
    for k, c in enumerate(CHANNELS):
        names = ('lin%d.model.1.weight' % k, 'lin%d' % k)
        have = [n for n in names if n in lin_sd]
        if not have:
            raise KeyError('rewriting_amd: the state dict lacks %s (or bare %s) of LPIPS v0.1' % names)
        value = lin_sd[have[0]]
        if tuple(value.shape) not in ((1, c, 1, 1), (c,)):
            raise ValueError('rewriting_amd: %r is %s, LPIPS (vgg) has (1, %d, 1, 1) there' % (have[0], tuple(value.shape), c))
        found.append(value.detach().to(torch.float32).reshape(c))
    return found


def from_state_dicts(vgg_sd, lin_sd):
    """An LPIPS with the convolutions of `vgg_sd` -- the keys ``0.weight`` ... ``28.bias``, bare or with torchvision's prefix
    ``features.`` (``classifier.*`` is ignored) -- and the lin layers of `lin_sd`: ``lin{k}.model.1.weight`` (1, C, 1, 1) as
    LPIPS v0.1 stores them, or bare ``lin{k}``."""
    net = LPIPS(perceptual.from_state_dict(vgg_sd))             # which leaves the layers past 20 to the line below
    tail = perceptual._layer_tensors(vgg_sd, TAIL_LAYERS, lambda index: index <= perceptual.LAST_LAYER, 'features[21:30]')
    for name, value in tail.items():
        index, kind = name.split('.')
        getattr(net.tail[index], kind).data.copy_(value)
    for p, value in zip(net.lins, _lin_weights(lin_sd)):
        p.data.copy_(value)
    return net.eval()


def default_weights():
    """The file RW_LPIPS_WEIGHTS names, or None when it is unset or names no readable file."""
    return perceptual.default_weights(WEIGHTS_ENV)


def lpips_vgg(vgg_path=None, lin_path=None):
    """from_state_dicts of two files, on the host: a torchvision VGG16 state dict (default: the file RW_VGG16_WEIGHTS names)
    and the lin layers of LPIPS v0.1 (default: RW_LPIPS_WEIGHTS).  No weights ship with the package."""
    vgg_path = vgg_path or perceptual.default_weights()
    lin_path = lin_path or default_weights()
    if not vgg_path or not lin_path:
        raise FileNotFoundError('rewriting_amd: LPIPS needs a torchvision VGG16 state dict and the lin layers of LPIPS v0.1; no '
                                'weights ship with the package -- pass both paths or set %s and %s to readable files'
                                % (perceptual.WEIGHTS_ENV, WEIGHTS_ENV))
    return from_state_dicts(torch.load(vgg_path, map_location='cpu', weights_only=True),
                            torch.load(lin_path, map_location='cpu', weights_only=True))
