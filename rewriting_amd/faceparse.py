"""The face-parsing BiSeNet of the edit-distance rows for faces on the HIP kernels: label maps without a directory of .pth
files.

The reference's face rows ('smile', 'faces_clean', metrics/load_seg.py:49-54) take their segmentations from
``FaceSegementer.segment_batch`` (:24-35): the images resized to 512 x 512 (nearest), the BiSeNet of
metrics/face-parsing.PyTorch/model.py -- a ResNet-18 context path (resnet.py), two attention-refinement modules, a
feature-fusion module and a 19-class head --, the arg-max of its first output, and the labels resized back (nearest).  This
is that network in the layout of its checkpoint, with every product on librewriting_hip.so:

* all 32 convolutions are ``hip.conv2d`` / ``hip.conv2d_add`` (the implicit GEMM of the Inception extractor; the residual sum
  and the ReLU of a ``BasicBlock`` in the epilogue), their batch norms (eps = 1e-5) folded by ``inception.fold_batch_norm``;
* ``hip.maxpool3x3s2p1`` is the stem's pooling, ``hip.global_avgpool`` the pooled vectors, whose 1 x 1 convolutions run on
  (B, C, 1, 1) maps;
* ``hip.gate_resample`` is every element-wise step: the sigmoid gate, the sum with the pooled vector or the coarser map,
  the nearest-neighbour step to the next size, ``feat * atten + feat``, and the image's resize to the working size;
* ``hip.bilinear_ac`` up-samples the class scores (align_corners=True), ``hip.seg_labels`` takes their arg-max and reads
  it at the pixels of the nearest-neighbour resize without writing the scores.

The index arithmetic of the two resizes lives in ``nearest_table`` and ``align_corners_table`` and nowhere else.  The module
is frozen and forward only, float32 on a HIP device.  No weights ship with the package: ``face_parser(path)`` loads a state
dict with the checkpoint's key names, and the environment variable ``RW_FACEPARSE_WEIGHTS`` names such a file.
"""
import functools
from collections import namedtuple

import numpy
import torch
from torch import nn

from . import hip, inception

WEIGHTS_ENV = 'RW_FACEPARSE_WEIGHTS'
BN_EPS = 1e-5
WORKING_SIZE = (512, 512)           # load_seg.py:27
ATTRIBUTES = ('skin', 'l_brow', 'r_brow', 'l_eye', 'r_eye', 'eye_g', 'l_ear', 'r_ear', 'ear_r', 'nose', 'mouth', 'u_lip',
              'l_lip', 'neck', 'neck_l', 'cloth', 'hair', 'hat')          # load_seg.py:46; label = index + 1, 0 = background
SMILE_SRC = tuple(ATTRIBUTES.index(name) + 1 for name in ('u_lip', 'l_lip', 'mouth'))        # :47

# name: the layer's name here (the folded parameters are <name>.weight / <name>.bias); weight: its key in the checkpoint;
# bn: the prefix of its batch norm's keys there, or None; relu: the activation behind it (a block's second convolution: behind
# the sum with the shortcut); out_ch None: the head's width, read from the checkpoint
Layer = namedtuple('Layer', 'name weight bn in_ch out_ch kernel stride padding relu')
STAGES = (('layer1', 64, 64, 1), ('layer2', 64, 128, 2), ('layer3', 128, 256, 2), ('layer4', 256, 512, 2))   # resnet.py:65-68
HEAD = 'conv_out.conv_out'


def _layer(name, weight, bn, i, o, k, s=1, p=0, relu=True):
    return Layer(name, weight, bn, i, o, (k, k), s, (p, p), relu)


def _cbr(name, i, o, k, s=1, p=0):
    """a ConvBNReLU (model.py:14-29)"""
    return _layer(name, name + '.conv.weight', name + '.bn', i, o, k, s, p)


def has_downsample(i, o, stride):
    return i != o or stride != 1                    # resnet.py:29


def _basic_block(name, i, o, stride):
    rows = [_layer(name + '.conv1', name + '.conv1.weight', name + '.bn1', i, o, 3, stride, 1),
            _layer(name + '.conv2', name + '.conv2.weight', name + '.bn2', o, o, 3, 1, 1)]
    if has_downsample(i, o, stride):
        rows.append(_layer(name + '.downsample', name + '.downsample.0.weight', name + '.downsample.1', i, o, 1, stride, 0,
                           relu=False))
    return rows


def _arm(name, i, o):
    """an AttentionRefinementModule (model.py:67-83); the sigmoid behind bn_atten is the gate kernel's"""
    return [_cbr(name + '.conv', i, o, 3, 1, 1),
            _layer(name + '.conv_atten', name + '.conv_atten.weight', name + '.bn_atten', o, o, 1, relu=False)]


def _layers():
    rows = [_layer('cp.resnet.conv1', 'cp.resnet.conv1.weight', 'cp.resnet.bn1', 3, 64, 7, 2, 3)]
    for stage, i, o, stride in STAGES:
        rows += _basic_block('cp.resnet.%s.0' % stage, i, o, stride) + _basic_block('cp.resnet.%s.1' % stage, o, o, 1)
    rows += _arm('cp.arm16', 256, 128) + _arm('cp.arm32', 512, 128)
    rows += [_cbr('cp.conv_head32', 128, 128, 3, 1, 1), _cbr('cp.conv_head16', 128, 128, 3, 1, 1),
             _cbr('cp.conv_avg', 512, 128, 1)]
    rows += [_cbr('ffm.convblk', 256, 256, 1),
             _layer('ffm.conv1', 'ffm.conv1.weight', None, 256, 64, 1),                  # its ReLU: model.py:205
             _layer('ffm.conv2', 'ffm.conv2.weight', None, 64, 256, 1, relu=False)]      # its sigmoid: the gate kernel's
    rows += [_cbr('conv_out.conv', 256, 256, 3, 1, 1),
             _layer(HEAD, HEAD + '.weight', None, 256, None, 1, relu=False)]
    return tuple(rows)


LAYERS = _layers()
IGNORED_PREFIXES = ('conv_out16.', 'conv_out32.')       # the segmenter reads output 0 only (load_seg.py:30)
_BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')


def conv_layers(n_classes):
    """The 32 convolutions of the path in the table's order, the head n_classes wide."""
    return tuple(op._replace(out_ch=n_classes) if op.out_ch is None else op for op in LAYERS)


def checkpoint_shapes(n_classes):
    """{checkpoint key: shape} of everything the loader reads."""
    shapes = {}
    for op in conv_layers(n_classes):
        shapes[op.weight] = (op.out_ch, op.in_ch) + op.kernel
        if op.bn:
            shapes.update({'%s.%s' % (op.bn, key): (op.out_ch,) for key in _BN_KEYS})
    return shapes


# ---- the index arithmetic of the two resizes ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=256)
def nearest_table(n_in, n_out):
    """int32 (n_out,): the input index F.interpolate (mode 'nearest', a float32 tensor) reads for every output index --
    min(floor(o scale), n_in - 1) with scale = n_in / n_out and the product both in float32.  A read-only array."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError('nearest_table: sizes must be positive, not %d -> %d' % (n_in, n_out))
    scale = numpy.float32(n_in) / numpy.float32(n_out)
    src = numpy.floor(numpy.arange(n_out, dtype=numpy.float32) * scale)
    table = numpy.minimum(src.astype(numpy.int64), n_in - 1).astype(numpy.int32)
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=256)
def align_corners_table(n_in, n_out):
    """(i0 int32, i1 int32, lam float64), each (n_out,): F.interpolate(mode='bilinear', align_corners=True) along one axis
    reads (1 - lam) x[i0] + lam x[i1] -- src = o (n_in - 1) / (n_out - 1) (0 where n_out == 1), i0 = floor(src),
    i1 = min(i0 + 1, n_in - 1), lam = src - i0.  Read-only arrays."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError('align_corners_table: sizes must be positive, not %d -> %d' % (n_in, n_out))
    o = numpy.arange(n_out, dtype=numpy.float64)
    src = o * (n_in - 1) / (n_out - 1) if n_out > 1 else numpy.zeros(1)
    i0 = numpy.minimum(numpy.floor(src).astype(numpy.int64), n_in - 1)
    i1 = numpy.minimum(i0 + 1, n_in - 1)
    tables = (i0.astype(numpy.int32), i1.astype(numpy.int32), src - i0)
    for t in tables:
        t.setflags(write=False)
    return tables


_device_cache = {}


def _on_device(kind, key, device, build):
    """build()'s arrays as tensors on `device`: copied once per (kind, sizes, device) and kept, 64 entries -- then the cache
    starts again."""
    device = torch.device(device)
    key = (kind, key, device.type, device.index)
    tables = _device_cache.get(key)
    if tables is None:
        tables = tuple(torch.from_numpy(numpy.array(a)).to(device) for a in build())
        if len(_device_cache) >= 64:
            _device_cache.clear()
        _device_cache[key] = tables
    return tables


def device_nearest_table(n_in, n_out, device):
    """nearest_table on `device`, or None where the axis keeps its size (the kernels' "no table")."""
    if int(n_in) == int(n_out):
        return None
    return _on_device('nearest', (int(n_in), int(n_out)), device, lambda: (nearest_table(n_in, n_out),))[0]


def device_ac_tables(in_size, out_size, device):
    """(idx int32 (2 H + 2 W), lam float32 (H + W)) on `device` for maps of in_size = (h, w) up-sampled to out_size = (H, W),
    as rw_bilinear_ac_f32 and rw_seg_labels_i64 read them: the rows' i0 and i1, then the columns'; the rows' lam, then the
    columns' -- rounded to float32 here, once."""
    (h, w), (H, W) = (int(v) for v in in_size), (int(v) for v in out_size)

    def build():
        y0, y1, ly = align_corners_table(h, H)
        x0, x1, lx = align_corners_table(w, W)
        return numpy.concatenate([y0, y1, x0, x1]), numpy.concatenate([ly, lx]).astype(numpy.float32)
    return _on_device('align_corners', (h, w, H, W), device, build)


# ---- the network ----------------------------------------------------------------------------------------------------------

class _Conv(inception._FoldedConv):
    """A convolution of the table: its batch norm folded in where it has one (no bias otherwise), the activation the
    table names, the shortcut of a residual block added in the epilogue."""

    def forward(self, x, res=None, out=None, c_off=0):
        op = self.op
        wp = self._derived.get('packed', self.weight, lambda: hip.conv2d_pack_weight(self.weight))
        bias = self.bias if op.bn else None
        if res is not None:
            return hip.conv2d_add(x, wp, self.weight.shape, bias, res, stride=op.stride, padding=op.padding, relu=op.relu,
                                  out=out)
        return hip.conv2d(x, wp, self.weight.shape, bias, stride=op.stride, padding=op.padding, relu=op.relu, out=out,
                          c_off=c_off)


def _attr(name):
    return name.replace('.', '_')


def _as_map(vec):
    """(B, C) -> (B, C, 1, 1): the map a 1 x 1 convolution of a pooled vector reads"""
    return vec.view(vec.shape[0], vec.shape[1], 1, 1)


class FaceParser(nn.Module):
    """images float32 (B, 3, H, W) as the checkpoint's network takes them -> the (B, n_classes, H, W) class scores at the
    images' own size, ``model(x)[0]`` of model.py:241-254 (``forward``), or their arg-max (``labels``).  Its parameters are
    the folded ``<layer>.weight`` / ``<layer>.bias`` (dots as underscores) and are frozen."""

    def __init__(self, n_classes=19):
        super().__init__()
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= hip.SEG_MAX_CLASSES:
            raise ValueError('rewriting_amd: FaceParser: n_classes must be in 1 .. %d, not %r' % (hip.SEG_MAX_CLASSES, n_classes))
        for op in conv_layers(self.n_classes):
            self.add_module(_attr(op.name), _Conv(op))

    def _check(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or 0 in x.shape:
            raise ValueError('rewriting_amd: FaceParser takes images float32 (B, 3, H, W), not %s'
                             % (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__,))
        if x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError('rewriting_amd: FaceParser takes images float32 (B, 3, H, W), not %s %s (nothing is converted)'
                             % (x.dtype, tuple(x.shape)))
        if not hip.on_device(x):
            raise RuntimeError('rewriting_amd: FaceParser: the images are on %s; the HIP kernels need a GPU tensor (there is '
                               'no CPU fallback)' % x.device)
        for name, p in self.named_parameters():
            if p.requires_grad:
                raise RuntimeError('rewriting_amd: FaceParser is frozen and forward only: parameter %s requires a gradient '
                                   '-- call requires_grad_(False) on it' % name)
            if p.dtype != torch.float32 or p.device != x.device:
                raise RuntimeError('rewriting_amd: FaceParser: parameter %s is %s on %s, the images on %s -- move the '
                                   'network with .to(device)' % (name, p.dtype, p.device, x.device))

    def _conv(self, name, x, **kw):
        return getattr(self, _attr(name))(x, **kw)

    def _block(self, name, x, i, o, stride):
        """a BasicBlock (resnet.py:36-48); the sum and its ReLU in the second convolution's epilogue, written over the
        shortcut, which nothing else reads"""
        t = self._conv(name + '.conv1', x)
        shortcut = self._conv(name + '.downsample', x) if has_downsample(i, o, stride) else x
        return self._conv(name + '.conv2', t, res=shortcut, out=shortcut)

    def _gate(self, name, feat):
        """(the module's convolution of feat, the logits of its channel gate) of an AttentionRefinementModule"""
        feat = self._conv(name + '.conv', feat)
        return feat, self._conv(name + '.conv_atten', _as_map(hip.global_avgpool(feat)))

    def _logits(self, x):
        """(B, n_classes, H8, W8): the head's scores before the up-sampling"""
        dev = x.device
        x = hip.maxpool3x3s2p1(self._conv('cp.resnet.conv1', x))
        feats = []
        for stage, i, o, stride in STAGES:
            # a block writes over its shortcut: the pooled map (layer1.0), the block before's output (every block 1) or a
            # fresh down-sampled map (block 0 of layers 2 - 4, whose input feat8 / feat16 is read again later)
            x = self._block('cp.resnet.%s.0' % stage, x, i, o, stride)
            x = self._block('cp.resnet.%s.1' % stage, x, o, o, 1)
            feats.append(x)
        _, feat8, feat16, feat32 = feats
        (h8, w8), (h16, w16), (h32, w32) = feat8.shape[2:], feat16.shape[2:], feat32.shape[2:]
        # the context path (model.py:104-125)
        avg = self._conv('cp.conv_avg', _as_map(hip.global_avgpool(feat32)))
        arm32, gate32 = self._gate('cp.arm32', feat32)
        up32 = hip.gate_resample(arm32, gate=gate32, add_vec=avg, rows=device_nearest_table(h32, h16, dev),
                                 cols=device_nearest_table(w32, w16, dev))
        feat32_up = self._conv('cp.conv_head32', up32)
        arm16, gate16 = self._gate('cp.arm16', feat16)
        up16 = hip.gate_resample(arm16, gate=gate16, add_map=feat32_up, rows=device_nearest_table(h16, h8, dev),
                                 cols=device_nearest_table(w16, w8, dev))
        # the fusion module (model.py:200-210); the concatenation: conv_head16 writes its half
        fcat = torch.empty(feat8.shape[0], 256, h8, w8, device=dev, dtype=torch.float32)
        fcat[:, :128].copy_(feat8)
        self._conv('cp.conv_head16', up16, out=fcat, c_off=128)
        feat = self._conv('ffm.convblk', fcat)
        atten = self._conv('ffm.conv2', self._conv('ffm.conv1', _as_map(hip.global_avgpool(feat))))
        fused = hip.gate_resample(feat, gate=atten, add_map=feat)
        return self._conv(HEAD, self._conv('conv_out.conv', fused))

    def forward(self, x):
        self._check(x)
        logits = self._logits(x)
        size = tuple(x.shape[2:])
        return hip.bilinear_ac(logits, size, *device_ac_tables(logits.shape[2:], size, x.device))

    def labels(self, x, out_size=None):
        """(B, 1, OH, OW) int64: the arg-max of forward(x) over the classes, read at the pixels a nearest-neighbour resize
        from x's size to out_size reads (None: x's size)."""
        self._check(x)
        logits = self._logits(x)
        size = tuple(x.shape[2:])
        oh, ow = size if out_size is None else (int(out_size[0]), int(out_size[1]))
        return hip.seg_labels(logits, size, *device_ac_tables(logits.shape[2:], size, x.device),
                              pick_rows=device_nearest_table(size[0], oh, x.device),
                              pick_cols=device_nearest_table(size[1], ow, x.device))


class FaceSegmenter:
    """``segment_batch`` of load_seg.py:24-35 with the whole batch at once: the images resized to ``size`` (nearest; None:
    parsed at their own size), parsed, the arg-max resized back (nearest)."""

    def __init__(self, net, size=WORKING_SIZE):
        self.net = net
        self.size = None if size is None else (int(size[0]), int(size[1]))

    def segment_batch(self, xs):
        """(B, 1, H, W) int64 labels on xs' device for images xs float32 (B, 3, H, W)."""
        self.net._check(xs)
        og_size = tuple(xs.shape[2:])
        if self.size is not None and self.size != og_size:
            xs = hip.gate_resample(xs, rows=device_nearest_table(og_size[0], self.size[0], xs.device),
                                   cols=device_nearest_table(og_size[1], self.size[1], xs.device))
        return self.net.labels(xs, out_size=og_size)


def from_state_dict(sd):
    """A FaceParser with the weights of `sd`, a state dict with the key names of the face-parsing checkpoint (the table
    LAYERS).  ``conv_out16.*``, ``conv_out32.*`` and ``*.num_batches_tracked`` are ignored; any other key, a missing key, a
    wrong shape and a tensor that requires a gradient are refused by name.  The head's width is read from
    ``conv_out.conv_out.weight``.  The batch norms are folded here, once."""
    head = sd.get(HEAD + '.weight')
    if head is None:
        raise KeyError('rewriting_amd: the state dict lacks %s.weight of the face-parsing network' % HEAD)
    if head.dim() != 4 or tuple(head.shape[1:]) != (256, 1, 1) or not 1 <= head.shape[0] <= hip.SEG_MAX_CLASSES:
        raise ValueError('rewriting_amd: %r is %s, the face-parsing network has (n_classes <= %d, 256, 1, 1) there'
                         % (HEAD + '.weight', tuple(head.shape), hip.SEG_MAX_CLASSES))
    n_classes = head.shape[0]
    shapes = checkpoint_shapes(n_classes)
    found = {}
    for key, value in sd.items():
        if key.startswith(IGNORED_PREFIXES) or key.endswith('num_batches_tracked'):
            continue
        if key not in shapes:
            raise KeyError('rewriting_amd: %r is no parameter of the face-parsing network (expected the keys of cp.resnet, '
                           'cp.arm16, cp.arm32, cp.conv_head16, cp.conv_head32, cp.conv_avg, ffm and conv_out)' % key)
        if tuple(value.shape) != shapes[key]:
            raise ValueError('rewriting_amd: %r is %s, the face-parsing network has %s there'
                             % (key, tuple(value.shape), shapes[key]))
        if value.requires_grad:
            raise RuntimeError('rewriting_amd: %r requires a gradient: the network is frozen and forward only (the batch '
                               'norms are folded into the weights) -- detach it' % key)
        found[key] = value
    missing = sorted(set(shapes) - set(found))
    if missing:
        raise KeyError('rewriting_amd: the state dict lacks %s of the face-parsing network' % ', '.join(missing))
    folded = {}
    for op in conv_layers(n_classes):
        if op.bn:
            w, b = inception.fold_batch_norm(found[op.weight], *(found['%s.%s' % (op.bn, key)] for key in _BN_KEYS),
                                             eps=BN_EPS)
        else:
            w, b = found[op.weight].detach().to(torch.float32), torch.zeros(op.out_ch)
        folded[_attr(op.name) + '.weight'], folded[_attr(op.name) + '.bias'] = w, b
    net = FaceParser(n_classes)
    net.load_state_dict(folded)
    return net.eval()


def face_parser(path):
    """from_state_dict of the file `path` (a state dict with the checkpoint's key names), on the host."""
    return from_state_dict(torch.load(path, map_location='cpu', weights_only=True))


def default_weights():
    """The file the environment variable RW_FACEPARSE_WEIGHTS names, or None when it is unset or names no readable file."""
    return inception.default_weights(WEIGHTS_ENV)
