"""The perceptual network of the overfit loss on the HIP kernels.

The reference builds ``VF = nethook.subsequence(torchvision.models.vgg16(pretrained=True).features, last_layer='20')``
(rewrite/ganrewrite.py:303-304) and adds ``1e-2 * mse_loss(VF(gt), VF(pred))`` to the image loss (:316-317).  This is that
network -- VGG16 up to the ReLU after conv4_2: nine stride-1 3x3 convolutions, each followed by a bias and a ReLU, three of
them also by a 2x2 max-pool -- with every product on librewriting_hip.so:

* layer 0 (3 -> 64 channels) is ``hip.conv3x3_rgb`` with bias and ReLU fused, its adjoint ``hip.conv3x3_rgb_input_grad``;
* the eight convolutions after it are the PLAIN forms of the generator's kernels (``w_scale = 1``, no style, demodulation,
  noise, bias or activation in their epilogue): Winograd F(2x2,3x3) in fp32 (``hip.conv3x3_wino``) wherever
  ``hip.wino_supported`` holds, the direct fp32 MFMA sum (``hip.conv3x3``, impl 0) elsewhere -- odd sizes come from
  ``bounds=`` crops; ``hip.bias_relu_pool`` follows each, in place on the convolution's result;
* the network is frozen: the only adjoint is the one to the input, the same route on the transposed, tap-flipped weight (as
  ``grad.DemodConv.backward``) behind ``hip.bias_relu_pool_grad``.  Weight gradients are out of scope: a parameter that
  requires one is refused.

The packed forms of a weight (each route's, forward and transposed) are made at their first use and kept on the weight's
version (``_DerivedWeights``).  float32 on a HIP device only; no ImageNet normalisation, as the reference applies none.
No weights ship with the package: ``vgg16_features(path)`` loads a torchvision VGG16 state dict, and the environment
variable ``RW_VGG16_WEIGHTS`` names such a file for ``apply_overfit`` / ``all_weights_insert`` without a ``feature_net``.
"""
import os

import torch
from torch import nn
from torch.autograd import Function

from . import hip
from .utils.stylegan2 import grad
from .utils.stylegan2.models import _DerivedWeights

WEIGHTS_ENV = 'RW_VGG16_WEIGHTS'

# (index in torchvision's vgg16().features, in_ch, out_ch, a MaxPool2d(2, 2) follows its ReLU)
LAYERS = ((0, 3, 64, False), (2, 64, 64, True),
          (5, 64, 128, False), (7, 128, 128, True),
          (10, 128, 256, False), (12, 256, 256, False), (14, 256, 256, True),
          (17, 256, 512, False), (19, 512, 512, False))
LAST_LAYER = 20


class _Block(nn.Module):
    """One convolution of VF with what follows it: bias, ReLU and, where `pool`, the 2x2 max-pool."""

    def __init__(self, in_ch, out_ch, pool):
        super().__init__()
        self.in_ch, self.out_ch, self.pool = in_ch, out_ch, pool
        self.weight = nn.Parameter(torch.zeros(out_ch, in_ch, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(out_ch), requires_grad=False)
        self._derived = _DerivedWeights()

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_derived'] = _DerivedWeights()       # caches are not copied or pickled
        return state

    def _conv(self, x, name, out_ch, weight, impl=None):
        """The plain stride-1 convolution of x to out_ch channels with `weight()` (1, out_ch, in_ch, 3, 3), on the route
        its shape takes -- or, with impl, on that form of the direct sum (``hip.conv3x3``'s impl); the packing is cached as
        `name`."""
        _, i, h, w = x.shape
        if impl is not None:
            wp = self._derived.get(name + '/direct', self.weight, lambda: hip.pack_conv_weight(weight(), 0))
            return hip.conv3x3(x, wp, out_ch, 1.0, impl=impl)
        if hip.wino_supported(out_ch, i, h, w):
            uf = self._derived.get(name + '/wino', self.weight, lambda: hip.pack_conv_weight_wino(weight()))
            return hip.conv3x3_wino(x, uf, out_ch, 1.0)
        wp = self._derived.get(name + '/direct', self.weight, lambda: hip.pack_conv_weight(weight(), 0))
        return hip.conv3x3(x, wp, out_ch, 1.0, impl=0)

    def activate(self, x, keep, impl=None):
        """(y or None, what the next block reads) of the convolution of x; keep: the full-size activated map y is wanted;
        impl: the form of the direct sum to take instead of the route the shape takes (lpips.py)."""
        if self.in_ch == 3:
            y = hip.conv3x3_rgb(x, self.weight, self.bias)
            return y, y
        pre = self._conv(x, 'forward', self.out_ch, lambda: self.weight.detach()[None], impl)
        y, pooled = hip.bias_relu_pool(pre, self.bias, pool=self.pool, keep=keep or not self.pool, out=pre)
        return y, (pooled if self.pool else y)

    def input_grad(self, g, y):
        """d input of the block from g, the gradient at what the next block read, and the saved y."""
        return self.conv_input_grad(hip.bias_relu_pool_grad(g, y, pooled=self.pool))

    def conv_input_grad(self, g):
        """d input of the convolution alone from g, the gradient at y already routed through the pool and masked by the ReLU
        (lpips.py adds a tap's own gradient there first)."""
        if self.in_ch == 3:
            return hip.conv3x3_rgb_input_grad(g, self.weight)
        return self._conv(g, 'adjoint', self.in_ch, lambda: grad.transposed_weight(self.weight[None], flip=True))


class _BlockFunction(Function):
    """A block with its adjoint to the input; saves its activated map y and nothing else."""

    @staticmethod
    def forward(ctx, x, block, trace):
        y, out = block.activate(x, keep=True)
        if trace is not None:
            trace.append(y.detach())
        ctx.block = block
        ctx.save_for_backward(y)
        return out

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return ctx.block.input_grad(g.contiguous(), y), None, None


def _check_images(module, images, pools):
    """What VGG16Features and lpips.LPIPS ask before their first launch: every one of images = {name: tensor} is (B, 3, H, W),
    on a HIP device, float32 and large enough for `pools` 2x2 pools; every parameter of `module` is frozen, float32 and on
    the images' device."""
    who, least = type(module).__name__, 2 ** pools
    for name, im in images.items():
        if not isinstance(im, torch.Tensor) or im.dim() != 4 or im.shape[1] != 3 or 0 in im.shape:
            raise ValueError('rewriting_amd: %s takes images (B, 3, H, W), %s is %s'
                             % (who, name, tuple(im.shape) if isinstance(im, torch.Tensor) else type(im).__name__))
        if not hip.on_device(im):
            raise RuntimeError('rewriting_amd: %s: %s is on %s; the HIP kernels need a GPU tensor (there is no CPU fallback)'
                               % (who, name, im.device))
        if im.dtype != torch.float32:
            raise RuntimeError('rewriting_amd: %s: %s is %s; the network is fp32 only -- cast with .float() (nothing is '
                               'converted)' % (who, name, im.dtype))
        if im.shape[2] < least or im.shape[3] < least:
            raise ValueError('rewriting_amd: %s halves its maps %d times: %s (an image, or a bounds= crop) of %d x %d leaves '
                             'nothing, it must be at least %d x %d' % (who, pools, name, im.shape[2], im.shape[3], least, least))
    device = next(iter(images.values())).device
    for name, p in module.named_parameters():
        if p.requires_grad:
            raise RuntimeError('rewriting_amd: %s is frozen: parameter %s requires a gradient, and the network has an adjoint '
                               'to its input only (weight gradients are not implemented) -- call requires_grad_(False) on it'
                               % (who, name))
        if p.dtype != torch.float32 or p.device != device:
            raise RuntimeError('rewriting_amd: %s: parameter %s is %s on %s, the images float32 on %s -- move the network '
                               'with .to(device)' % (who, name, p.dtype, p.device, device))


class VGG16Features(nn.Module):
    """torchvision's ``vgg16().features[:21]`` (VF of rewrite/ganrewrite.py:303-304): (B, 3, H, W) float32 on a HIP device
    -> (B, 512, H // 8, W // 8), the ReLU after conv4_2.  Its parameters carry torchvision's names (``0.weight`` ...
    ``19.bias``) and are frozen."""

    def __init__(self):
        super().__init__()
        for index, in_ch, out_ch, pool in LAYERS:
            self.add_module(str(index), _Block(in_ch, out_ch, pool))

    def blocks(self):
        return [getattr(self, str(index)) for index, _, _, _ in LAYERS]

    def forward(self, x, trace=None):
        """trace: a list that receives every block's activated map before its pool (the decisions of the device)."""
        _check_images(self, {'the input': x}, pools=3)
        for block in self.blocks():
            if grad.records(x):
                x = _BlockFunction.apply(x, block, trace)
            else:
                y, x = block.activate(x.detach(), keep=trace is not None)
                if trace is not None:
                    trace.append(y)
        return x


def from_state_dict(sd):
    """A VGG16Features with the weights of `sd`: the bare keys ``0.weight`` ... ``19.bias``, or a whole torchvision VGG16
    state dict (``features.N.*``; its ``classifier.*`` entries and the layers past 20 are ignored)."""
    net = VGG16Features()
    net.load_state_dict(_layer_tensors(sd, LAYERS, lambda index: index > LAST_LAYER, 'features[:21]'))
    return net.eval()


def _layer_tensors(sd, layers, elsewhere, part):
    """{'N.weight', 'N.bias': float32 tensor} of the convolutions `layers` (rows as LAYERS) out of the state dict `sd`, whose
    keys are bare or carry torchvision's prefix ``features.``.  ``classifier.*`` and a convolution N with elsewhere(N) belong to
    others and are skipped; any other key is refused, and so are a missing key and a wrong shape, by name.  part: what the
    messages call the layers."""
    shapes = {'%d.%s' % (index, kind): (out_ch, in_ch, 3, 3) if kind == 'weight' else (out_ch,)
              for index, in_ch, out_ch, _ in layers for kind in ('weight', 'bias')}
    found = {}
    for key, value in sd.items():
        name = key[len('features.'):] if key.startswith('features.') else key
        index = name.split('.')[0]
        if key.startswith('classifier.') or (index.isdigit() and elsewhere(int(index))):
            continue
        if name not in shapes:
            raise KeyError('rewriting_amd: %r is no parameter of VGG16 %s (expected %s, bare or with the prefix "features.")'
                           % (key, part, ', '.join(shapes)))
        if tuple(value.shape) != shapes[name]:
            raise ValueError('rewriting_amd: %r is %s, VGG16 has %s there' % (key, tuple(value.shape), shapes[name]))
        found[name] = value.detach().to(torch.float32)
    missing = sorted(set(shapes) - set(found))
    if missing:
        raise KeyError('rewriting_amd: the state dict lacks %s of VGG16 %s' % (', '.join(missing), part))
    return found


def vgg16_features(path):
    """from_state_dict of the file `path` (a torchvision VGG16 state dict, or its features[:21] alone), on the host."""
    return from_state_dict(torch.load(path, map_location='cpu', weights_only=True))


def default_weights(env=WEIGHTS_ENV):
    """The file the environment variable `env` (RW_VGG16_WEIGHTS) names, or None when it is unset or names no readable file."""
    path = os.environ.get(env)
    return path if path and os.path.isfile(path) and os.access(path, os.R_OK) else None
