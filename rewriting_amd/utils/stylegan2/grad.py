"""torch.autograd through the modules of a styled convolution, on the HIP kernels.

The reference's ``insert`` is plain autograd over whatever ``target_model`` a rewriter defines
(rewrite/ganrewrite.py:254-298): ``loss.backward()`` runs through ApplyStyle, DemodulatedConv2dF
(utils/stylegan2/models.py:313-329 -- whose demodulation factor is recomputed from the weight and is part of
the graph, quirk Q3), BlurF, NoiseInjectionF and FusedLeakyReLUF.  The fused HIP solver (rewrite/hipsolve.py)
restates that arithmetic for the three targets the reference's rewriters define; everything else -- a target
spanning several layers, a hooked module, a goal batch larger than one -- takes this path: the same loop, the
same torch.optim.Adam, with every forward AND backward product on the kernels of librewriting_hip.so:

* d fmap of the convolution = the forward kernels on the transposed weights (stride 1: flipped taps,
  ``conv3x3``; the stride-2 transposed convolution: the stride-1 correlation of the gradient map sampled at the
  odd positions -- four times the minimal multiply count, accepted on this fallback path);
* d weight = ``rw_conv_wgrad_f32`` (the split-K MFMA GEMM of the solver's K3 without its Adam epilogue) minus the
  demodulation term  s^2 W sigma^2 demod^2 sum_p g y  (``rw_rowdot_f32`` for the per-(image, channel) sums);
* the blur and the leaky ReLU already carry their adjoints (op/upfirdn2d.py, op/fused_act.py).

Gradients the reference computes and never uses (noise strength, activation bias, modulation weights: quirk
Q5) are produced only when autograd asks for them.

A loss on the IMAGE (``all_weights_insert`` / ``apply_overfit``, rewrite/ganrewrite.py:300-331; projecting a picture
into the latent space) needs the rest of the generator as well -- the second half of this file:

* ``ToRGB`` (models.py:394-425, 639-655): d fmap by ``rw_to_rgb_input_grad_f32``, d weight and d style from the
  per-image sums of ``rw_to_rgb_weight_sums_f32`` (one deterministic pass over the feature map), d bias by
  ``rw_bias_grad_f32``, d skip = the incoming gradient;
* ``EqualLinear`` (the mapping network, every modulation, ToRGB's modulation): the leaky ReLU through
  ``fused_bias_act`` with the output as its reference, d input by the forward kernel on the transposed weight, d weight
  and d bias as torch expressions on latent-sized tensors;
* ``PixelNorm`` and ``AdjustLatent``: torch expressions on at most batch x n_latent x style_dim elements.

``records(...)`` is the one test the modules make before they enter one of these: under ``torch.no_grad()``, or when
nothing they are given requires a gradient, they call the kernel wrapper directly, exactly as before.  float32 only:
the double path stays forward only.
"""
import torch
from torch.autograd import Function

from ... import hip


def records(*tensors):
    """True when autograd would record an operation on these tensors (None = absent)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class StyleMul(Function):
    """ApplyStyle: fmap * style[:, :, None, None]  (models.py:616-620)."""

    @staticmethod
    def forward(ctx, fmap, style):
        ctx.save_for_backward(fmap, style)
        return hip.style_mul(fmap, style)

    @staticmethod
    def backward(ctx, g):
        fmap, style = ctx.saved_tensors
        g = g.contiguous()
        gf = hip.style_mul(g, style) if ctx.needs_input_grad[0] else None
        gs = hip.rowdot(g, fmap) if ctx.needs_input_grad[1] else None
        return gf, gs


class NoiseAdd(Function):
    """NoiseInjectionF: fmap + weight * noise  (models.py:539-546); noise is a constant of the graph."""

    @staticmethod
    def forward(ctx, fmap, noise, weight):
        ctx.save_for_backward(noise)
        return hip.noise_add(fmap, noise, weight)

    @staticmethod
    def backward(ctx, g):
        noise, = ctx.saved_tensors
        gw = None
        if ctx.needs_input_grad[2]:
            b = g.shape[0]
            gw = (g.sum(1).reshape(b, -1) * noise.reshape(b, -1)).sum().reshape(1)
        return (g if ctx.needs_input_grad[0] else None), None, gw


def transposed_weight(weight, flip):
    """(1, O, I, 3, 3) -> (1, I, O, 3, 3), taps flipped for the stride-1 backward-to-input."""
    w = weight.detach()[0].transpose(0, 1)
    if flip:
        w = w.flip(2, 3)
    return w.contiguous()[None]


class DemodConv(Function):
    """DemodulatedConv2dF.forward (models.py:313-329): y = conv(x, s W) * rsqrt(sum (s W sigma)^2 + eps), with x the
    already modulated map.  `module` supplies the kernels' dispatch (algorithm, packed weights) and the constants."""

    @staticmethod
    def forward(ctx, fmap, weight, style, module):
        y = module.run(fmap, style, style_on_load=False, weight_changes=bool(weight.requires_grad))
        ctx.module = module
        ctx.save_for_backward(fmap, weight, style, y)
        return y

    @staticmethod
    def backward(ctx, g):
        fmap, weight, style, y = ctx.saved_tensors
        m = ctx.module
        g = g.contiguous()
        s = m.scale
        demod = hip.demod(hip.weight_sqsum(weight, s), style) if m.demodulate else None
        gx = gw = gs = None
        if ctx.needs_input_grad[0]:
            wt = hip.pack_conv_weight(transposed_weight(weight, flip=not m.upsample), 0)
            # the MFMA kernels take in_ch % 16 == 0 and out_ch % 32 == 0 (every layer of the generators); odd test
            # shapes go to the one-thread-per-output kernel
            impl = 0 if (m.out_channel % 16 == 0 and m.in_channel % 32 == 0) else 1
            c = hip.conv3x3(g, wt, m.in_channel, s, style=demod, impl=impl)   # demod rides in as the on-load factor of g
            gx = c[:, :, 1::2, 1::2].contiguous() if m.upsample else c
        need_r = m.demodulate and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        if need_r:
            rd = hip.rowdot(g, y) * demod * demod                         # (B, O): sum_p g conv * demod^3, conv = y / demod
        if ctx.needs_input_grad[1]:
            dw = hip.conv_wgrad(g, fmap, m.upsample, scale=s, gscale=demod)
            if m.demodulate:
                dw = dw - (s * s) * weight.detach()[0] * torch.mm(rd.t(), style.detach() ** 2)[:, :, None, None]
            gw = dw[None]
        if ctx.needs_input_grad[2] and m.demodulate:
            gs = -style.detach() * torch.mm(rd, hip.weight_sqsum(weight, s))
        return gx, gw, gs, None


class ToRGB(Function):
    """ToRGBF's projection (models.py:394-425, 639-655): hip.to_rgb of (fmap, weight (3, C), style (B, C), bias (3) or
    None, skip (B, 3, H, W) or None)."""

    @staticmethod
    def forward(ctx, fmap, weight, style, bias, skip, scale):
        ctx.scale = scale
        ctx.save_for_backward(fmap, weight, style)
        return hip.to_rgb(fmap, weight, style, bias, skip, scale)

    @staticmethod
    def backward(ctx, g):
        fmap, weight, style = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = g.contiguous()
        s = ctx.scale
        gf = hip.to_rgb_input_grad(g, weight, style, s) if need[0] else None
        gw = gs = None
        if need[1] or need[2]:
            t = hip.to_rgb_weight_sums(g, fmap)                         # (B, 3, C): sum_p g x
            if need[1]:
                gw = s * (t * style.detach()[:, None, :]).sum(0)
            if need[2]:
                gs = s * (t * weight.detach()[None]).sum(1)
        gb = hip.bias_grad(g) if need[3] else None
        return gf, gw, gs, gb, (g if need[4] else None), None


class EqualLinear(Function):
    """EqualLinear.forward (models.py:487-517): act(x (scale W)^T + lr_mul b), act = sqrt(2) leaky_relu(., 0.2) or the
    identity.  x may be the strided row view latent[:, index].  `module` supplies scale, lr_mul and the activation."""

    @staticmethod
    def forward(ctx, x, weight, bias, module):
        act = bool(module.activation)
        y = hip.equal_linear(x, weight, bias, module.scale, module.lr_mul, act=act)
        ctx.module = module
        ctx.save_for_backward(x, weight, y if act else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        m = ctx.module
        g = g.contiguous()
        # through the activation: (y > 0 ? g : 0.2 g) sqrt(2), the reference's own backward (op/fused_act.py:19-39)
        gpre = hip.fused_bias_act(g, None, y, 3, 1, 0.2, hip.SQRT2) if y is not None else g
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = hip.equal_linear(gpre, weight.detach().t().contiguous(), None, m.scale, 1.0).view(x.shape)
        if ctx.needs_input_grad[1]:
            gw = torch.mm(gpre.t(), x.detach().reshape(gpre.shape[0], -1)) * m.scale
        if ctx.needs_input_grad[2]:
            gb = gpre.sum(0) * m.lr_mul
        return gx, gw, gb, None


class PixelNorm(Function):
    """PixelNormL (models.py:609-614): x rsqrt(mean(x^2, 1) + eps) on the (B, style_dim) latent."""

    @staticmethod
    def forward(ctx, x, eps):
        ctx.eps = eps
        ctx.save_for_backward(x)
        return hip.pixel_norm(x, eps)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        x = x.detach()
        r = torch.rsqrt(torch.mean(x * x, dim=1, keepdim=True) + ctx.eps)
        return g * r - x * (r * r * r) * torch.mean(g * x, dim=1, keepdim=True), None


class AdjustLatent(Function):
    """AdjustLatent (models.py:570-583): avg + psi (w - avg) where avg is given, one copy per layer."""

    @staticmethod
    def forward(ctx, w, avg, n_latent, psi):
        ctx.factor = float(psi) if avg is not None else 1.0
        return hip.adjust_latent(w, avg, n_latent, psi)

    @staticmethod
    def backward(ctx, g):
        return g.sum(1) * ctx.factor, None, None, None
