"""The Inception-v3 pool3 feature extractor of the FID row on the HIP kernels.

The reference feeds its images to the 2015 TF Inception graph and takes the 2048 activations of ``pool_3``
(metrics/fid.py:67-84,90-131), from which ``calculate_activation_statistics`` (:40-62) forms the mean and the covariance.
This is that network in the layout of its public PyTorch port (torchvision ``Inception3`` key names, the FID variant's
poolings): 94 convolutions, each followed by a batch norm (eps = 1e-3) and a ReLU, the 3x3 poolings between them and the
global average at the end, with every product on librewriting_hip.so:

* ``hip.inception_input`` clamps float images to [-1, 1] (``fid.pt_to_np``, :190-193) or maps bytes by x / 127.5 - 1, and
  resizes to 299 x 299 with the arithmetic of ``F.interpolate(mode='bilinear', align_corners=False)``;
* every convolution is ``hip.conv2d`` (an implicit GEMM on the fp32-input MFMA) with the batch norm folded into its weight
  and bias and the ReLU in its epilogue; the last convolution of a branch writes its slice of the block's output, so a
  concatenation is no copy;
* ``hip.pool3x3`` is the three poolings (max stride 2; average with count_include_pad=False; max stride 1 -- the pool branch
  of ``Mixed_7c``, the FID variant's quirk), ``hip.global_avgpool`` the end.

The batch norms are folded once, in float64 on the host (``fold_batch_norm``), and rounded to float32; after that the module
is frozen and forward only: a parameter that requires a gradient is refused.  float32 on a HIP device only.  No weights
ship with the package: ``fid_inception(path)`` loads a state dict with torchvision's key names, and the environment variable
``RW_INCEPTION_WEIGHTS`` names such a file.
"""
import os
from collections import namedtuple

import torch
from torch import nn

from . import hip
from .utils.stylegan2.models import _DerivedWeights

WEIGHTS_ENV = 'RW_INCEPTION_WEIGHTS'
BN_EPS = 1e-3
MIN_SIZE = 75               # the smallest input whose last map is 1 x 1
FEATURES = 2048

Conv = namedtuple('Conv', 'name in_ch out_ch kernel stride padding')
Pool = namedtuple('Pool', 'mode')
Block = namedtuple('Block', 'name in_ch branches')     # branches: ((trunk ops, head ops), ...); the heads are concatenated


def _c(name, in_ch, out_ch, kernel, stride=1, padding=0):
    kernel = (kernel, kernel) if isinstance(kernel, int) else tuple(kernel)
    padding = (padding, padding) if isinstance(padding, int) else tuple(padding)
    return Conv(name, in_ch, out_ch, kernel, stride, padding)


STEM = (_c('Conv2d_1a_3x3', 3, 32, 3, 2), _c('Conv2d_2a_3x3', 32, 32, 3), _c('Conv2d_2b_3x3', 32, 64, 3, 1, 1),
        Pool('max_s2'), _c('Conv2d_3b_1x1', 64, 80, 1), _c('Conv2d_4a_3x3', 80, 192, 3), Pool('max_s2'))


def _block_a(name, i, pool_features):
    return Block(name, i, (
        ((), (_c('branch1x1', i, 64, 1),)),
        ((_c('branch5x5_1', i, 48, 1),), (_c('branch5x5_2', 48, 64, 5, 1, 2),)),
        ((_c('branch3x3dbl_1', i, 64, 1), _c('branch3x3dbl_2', 64, 96, 3, 1, 1)), (_c('branch3x3dbl_3', 96, 96, 3, 1, 1),)),
        ((Pool('avg'),), (_c('branch_pool', i, pool_features, 1),))))


def _block_b(name, i):
    return Block(name, i, (
        ((), (_c('branch3x3', i, 384, 3, 2),)),
        ((_c('branch3x3dbl_1', i, 64, 1), _c('branch3x3dbl_2', 64, 96, 3, 1, 1)), (_c('branch3x3dbl_3', 96, 96, 3, 2),)),
        ((), (Pool('max_s2'),))))


def _block_c(name, i, c):
    row, col = ((1, 7), (0, 3)), ((7, 1), (3, 0))
    return Block(name, i, (
        ((), (_c('branch1x1', i, 192, 1),)),
        ((_c('branch7x7_1', i, c, 1), _c('branch7x7_2', c, c, row[0], 1, row[1])),
         (_c('branch7x7_3', c, 192, col[0], 1, col[1]),)),
        ((_c('branch7x7dbl_1', i, c, 1), _c('branch7x7dbl_2', c, c, col[0], 1, col[1]),
          _c('branch7x7dbl_3', c, c, row[0], 1, row[1]), _c('branch7x7dbl_4', c, c, col[0], 1, col[1])),
         (_c('branch7x7dbl_5', c, 192, row[0], 1, row[1]),)),
        ((Pool('avg'),), (_c('branch_pool', i, 192, 1),))))


def _block_d(name, i):
    return Block(name, i, (
        ((_c('branch3x3_1', i, 192, 1),), (_c('branch3x3_2', 192, 320, 3, 2),)),
        ((_c('branch7x7x3_1', i, 192, 1), _c('branch7x7x3_2', 192, 192, (1, 7), 1, (0, 3)),
          _c('branch7x7x3_3', 192, 192, (7, 1), 1, (3, 0))), (_c('branch7x7x3_4', 192, 192, 3, 2),)),
        ((), (Pool('max_s2'),))))


def _block_e(name, i, pool):
    def fork(prefix, ch):
        return (_c(prefix + 'a', ch, 384, (1, 3), 1, (0, 1)), _c(prefix + 'b', ch, 384, (3, 1), 1, (1, 0)))
    return Block(name, i, (
        ((), (_c('branch1x1', i, 320, 1),)),
        ((_c('branch3x3_1', i, 384, 1),), fork('branch3x3_2', 384)),
        ((_c('branch3x3dbl_1', i, 448, 1), _c('branch3x3dbl_2', 448, 384, 3, 1, 1)), fork('branch3x3dbl_3', 384)),
        ((Pool(pool),), (_c('branch_pool', i, 192, 1),))))


BLOCKS = (_block_a('Mixed_5b', 192, 32), _block_a('Mixed_5c', 256, 64), _block_a('Mixed_5d', 288, 64),
          _block_b('Mixed_6a', 288),
          _block_c('Mixed_6b', 768, 128), _block_c('Mixed_6c', 768, 160), _block_c('Mixed_6d', 768, 160),
          _block_c('Mixed_6e', 768, 192),
          _block_d('Mixed_7a', 768),
          _block_e('Mixed_7b', 1280, 'avg'), _block_e('Mixed_7c', 2048, 'max_s1'))


def block_out_channels(block):
    """Channels of a block's concatenation: its heads' out-channels, a pool head passing the block's input through."""
    return sum(op.out_ch if isinstance(op, Conv) else block.in_ch for _, heads in block.branches for op in heads)


def conv_layers():
    """[(torchvision layer name, Conv)] of all 94 convolutions in the order they run."""
    rows = [(op.name, op) for op in STEM if isinstance(op, Conv)]
    for block in BLOCKS:
        for trunk, heads in block.branches:
            rows += [('%s.%s' % (block.name, op.name), op) for op in trunk + heads if isinstance(op, Conv)]
    return rows


def fold_batch_norm(weight, gamma, beta, mean, var, eps=BN_EPS):
    """(weight, bias) float32 of the convolution that equals conv(weight) followed by the frozen batch norm: in float64,
    scale = gamma / sqrt(var + eps), weight scale[:, None, None, None] and beta - mean scale, each rounded once."""
    scale = gamma.detach().double() / torch.sqrt(var.detach().double() + eps)
    w = weight.detach().double() * scale[:, None, None, None]
    b = beta.detach().double() - mean.detach().double() * scale
    return w.to(torch.float32), b.to(torch.float32)


def _op_out_size(op, h, w):
    if isinstance(op, Conv):
        return hip.conv2d_out_size(h, w, op.kernel, op.stride, op.padding)
    return ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if op.mode == 'max_s2' else (h, w)


class _FoldedConv(nn.Module):
    """A convolution with its batch norm folded in and its ReLU behind it."""

    def __init__(self, op):
        super().__init__()
        self.op = op
        self.weight = nn.Parameter(torch.zeros(op.out_ch, op.in_ch, *op.kernel), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(op.out_ch), requires_grad=False)
        self._derived = _DerivedWeights()

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_derived'] = _DerivedWeights()       # caches are not copied or pickled
        return state

    def forward(self, x, out=None, c_off=0):
        wp = self._derived.get('packed', self.weight, lambda: hip.conv2d_pack_weight(self.weight))
        return hip.conv2d(x, wp, self.weight.shape, self.bias, stride=self.op.stride, padding=self.op.padding, relu=True,
                          out=out, c_off=c_off)


def _run(op, module, x, out=None, c_off=0):
    if isinstance(op, Conv):
        return module(x, out=out, c_off=c_off)
    return hip.pool3x3(x, op.mode, out=out, c_off=c_off)


class _Mixed(nn.Module):
    """An Inception block: its branches read the same input, their heads write their slices of one output."""

    def __init__(self, block):
        super().__init__()
        self.block = block
        for trunk, heads in block.branches:
            for op in trunk + heads:
                if isinstance(op, Conv):
                    self.add_module(op.name, _FoldedConv(op))

    def _module(self, op):
        return getattr(self, op.name) if isinstance(op, Conv) else None

    def forward(self, x):
        b, _, h, w = x.shape
        first = self.block.branches[0]
        oh, ow = h, w
        for op in first[0] + first[1][:1]:
            oh, ow = _op_out_size(op, oh, ow)
        out = torch.empty(b, block_out_channels(self.block), oh, ow, device=x.device, dtype=torch.float32)
        c_off = 0
        for trunk, heads in self.block.branches:
            t = x
            for op in trunk:
                t = _run(op, self._module(op), t)
            for op in heads:
                _run(op, self._module(op), t, out=out, c_off=c_off)
                c_off += op.out_ch if isinstance(op, Conv) else self.block.in_ch
        return out


class FIDInception(nn.Module):
    """images -> (B, 2048) float32 pool3 features on the images' device.  images: float32 (B, 3, H, W) in [-1, 1] (values
    outside are clamped) or uint8 (B, H, W, 3).  ``resize=True`` resizes them to 299 x 299 first; ``resize=False`` feeds them
    as they are, anything from 75 x 75 up.  Its parameters are the folded ``<layer>.weight`` / ``<layer>.bias`` and are
    frozen."""

    def __init__(self):
        super().__init__()
        for op in STEM:
            if isinstance(op, Conv):
                self.add_module(op.name, _FoldedConv(op))
        for block in BLOCKS:
            self.add_module(block.name, _Mixed(block))

    def _check(self, images, resize):
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or 0 in images.shape:
            raise ValueError('rewriting_amd: FIDInception takes images float32 (B, 3, H, W) or uint8 (B, H, W, 3), not %s'
                             % (tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__,))
        is_bytes = images.dtype == torch.uint8
        if images.shape[3 if is_bytes else 1] != 3 or images.dtype not in (torch.uint8, torch.float32):
            raise ValueError('rewriting_amd: FIDInception takes images float32 (B, 3, H, W) or uint8 (B, H, W, 3), not %s %s '
                             '(nothing is converted)' % (images.dtype, tuple(images.shape)))
        h, w = (images.shape[1], images.shape[2]) if is_bytes else (images.shape[2], images.shape[3])
        if not resize and (h < MIN_SIZE or w < MIN_SIZE):
            raise ValueError('rewriting_amd: FIDInception(resize=False): images of %d x %d leave no map at the end of the '
                             'network, they must be at least %d x %d' % (h, w, MIN_SIZE, MIN_SIZE))
        if not hip.on_device(images):
            raise RuntimeError('rewriting_amd: FIDInception: the images are on %s; the HIP kernels need a GPU tensor (there '
                               'is no CPU fallback)' % images.device)
        for name, p in self.named_parameters():
            if p.requires_grad:
                raise RuntimeError('rewriting_amd: FIDInception is frozen and forward only: parameter %s requires a gradient '
                                   '-- call requires_grad_(False) on it' % name)
            if p.dtype != torch.float32 or p.device != images.device:
                raise RuntimeError('rewriting_amd: FIDInception: parameter %s is %s on %s, the images on %s -- move the '
                                   'network with .to(device)' % (name, p.dtype, p.device, images.device))

    def forward(self, images, resize=True):
        self._check(images, resize)
        x = hip.inception_input(images, size=hip.INCEPTION_SIZE if resize else None)
        for op in STEM:
            x = _run(op, getattr(self, op.name) if isinstance(op, Conv) else None, x)
        for block in BLOCKS:
            x = getattr(self, block.name)(x)
        return hip.global_avgpool(x)


_BN_KEYS = (('bn.weight', 'gamma'), ('bn.bias', 'beta'), ('bn.running_mean', 'mean'), ('bn.running_var', 'var'))


def from_state_dict(sd):
    """A FIDInception with the weights of `sd`, a state dict with torchvision ``Inception3`` key names:
    ``<layer>.conv.weight`` and ``<layer>.bn.{weight,bias,running_mean,running_var}`` for each of the 94 convolutions.
    ``fc.*``, ``AuxLogits.*`` and ``*.num_batches_tracked`` are ignored; any other key, a missing key, a wrong shape and a
    tensor that requires a gradient are refused by name.  The batch norms are folded here, once."""
    layers = conv_layers()
    shapes = {}
    for name, op in layers:
        shapes['%s.conv.weight' % name] = (op.out_ch, op.in_ch) + op.kernel
        for key, _ in _BN_KEYS:
            shapes['%s.%s' % (name, key)] = (op.out_ch,)
    found = {}
    for key, value in sd.items():
        if key.startswith('fc.') or key.startswith('AuxLogits.') or key.endswith('num_batches_tracked'):
            continue
        if key not in shapes:
            raise KeyError('rewriting_amd: %r is no parameter of the Inception-v3 feature extractor (expected '
                           '<layer>.conv.weight and <layer>.bn.{weight,bias,running_mean,running_var} of %s ... %s)'
                           % (key, layers[0][0], layers[-1][0]))
        if tuple(value.shape) != shapes[key]:
            raise ValueError('rewriting_amd: %r is %s, Inception-v3 has %s there' % (key, tuple(value.shape), shapes[key]))
        if value.requires_grad:
            raise RuntimeError('rewriting_amd: %r requires a gradient: the feature extractor is frozen and forward only '
                               '(the batch norms are folded into the weights) -- detach it' % key)
        found[key] = value
    missing = sorted(set(shapes) - set(found))
    if missing:
        raise KeyError('rewriting_amd: the state dict lacks %s of Inception-v3' % ', '.join(missing))
    folded = {}
    for name, _ in layers:
        w, b = fold_batch_norm(found['%s.conv.weight' % name], *(found['%s.%s' % (name, key)] for key, _ in _BN_KEYS))
        folded['%s.weight' % name], folded['%s.bias' % name] = w, b
    net = FIDInception()
    net.load_state_dict(folded)
    return net.eval()


def fid_inception(path):
    """from_state_dict of the file `path` (a state dict with torchvision Inception3 key names), on the host."""
    return from_state_dict(torch.load(path, map_location='cpu', weights_only=True))


def default_weights(env=WEIGHTS_ENV):
    """The file the environment variable `env` (RW_INCEPTION_WEIGHTS) names, or None when it is unset or names no readable
    file."""
    path = os.environ.get(env)
    return path if path and os.path.isfile(path) and os.access(path, os.R_OK) else None
