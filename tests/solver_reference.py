"""TEST INFRASTRUCTURE -- a float64 reference of ONE iteration of the rank-constrained solve (rw_solve.hip), on the host.

The arithmetic is that of ``hip_emulation._solve_iteration``: torch autograd over oracle/restatement.py's ``demod_conv``,
``upfirdn2d``, ``noise_rows`` and the leaky ReLU, then torch.optim.Adam's single-tensor update with the bias corrections
``hipsolve.Solver`` tabulates -- in double precision by default, in float32 on request (the yardstick the device is
measured against).  It never imports ``rewriting_amd.hip``.

One iteration is a well-conditioned function of (W, m, v, t) as long as no position sits on a kink of the L1 loss or of
the leaky ReLU.  ``make_problem`` puts the L1 kink out of reach by construction; ``undecided`` states how far the leaky
ReLU's is, and a problem is used only when ``admissible`` says that it is out of reach of float32 rounding too."""
import math
import types

import torch

from oracle import restatement as R

LR = 0.05
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def make_problem(O, I, h, w, rank, upsample, plain, seed):
    """float32 tensors of one target.  ``val`` is the float64 output at W0 plus, per element, a random sign times a
    random magnitude in [0.25, 1.25], rounded to float32: |out - val| >= 0.25 whatever rounds the output."""
    gen = torch.Generator().manual_seed(seed)
    p = types.SimpleNamespace(O=O, I=I, h=h, w=w, rank=rank, upsample=bool(upsample), plain=bool(plain), seed=seed)
    p.W0 = torch.randn(1, O, I, 3, 3, generator=gen)
    p.key = torch.randn(1, I, h, w, generator=gen)
    p.style = 1 + 0.3 * torch.randn(1, I, generator=gen)
    p.bias = None if plain else 0.1 * torch.randn(O, generator=gen)
    p.noise_w = None if plain else torch.tensor([0.1])
    p.context = None
    if rank:
        p.context = torch.linalg.qr(torch.randn(I, rank, generator=gen))[0].t().contiguous()   # orthonormal rows
    p.blur_k = R.make_kernel([1, 3, 3, 1]) * 4 if (upsample and not plain) else None
    out, _ = forward(p, p.W0, torch.float64)
    sign = torch.randint(0, 2, out.shape, generator=gen).double() * 2 - 1
    p.val = (out + sign * (0.25 + torch.rand(out.shape, generator=gen).double())).float()
    return p


def forward(p, W, dtype):
    """(output of the target, the leaky ReLU's input or None for a plain target) at weight W, in ``dtype``."""
    out = R.demod_conv(p.key.to(dtype), p.style.to(dtype), W.to(dtype), p.upsample)
    if p.plain:
        return out, None
    if p.upsample:
        out = R.upfirdn2d(out, p.blur_k.to(dtype), pad=(1, 1))
    hh, ww = out.shape[2:]
    pre = out + p.noise_w.to(dtype) * R.noise_rows(1, hh * ww).to(dtype).view(1, 1, hh, ww)
    pre = pre + p.bias.to(dtype).view(1, -1, 1, 1)
    return R.fused_leaky_relu(pre, None), pre


def undecided(p, W=None):
    """(min |pre64|, max |pre32 - pre64|) of the leaky ReLU's input at W (default W0); (inf, 0) for a plain target."""
    if p.plain:
        return math.inf, 0.0
    W = p.W0 if W is None else W
    with torch.no_grad():
        pre64, pre32 = forward(p, W, torch.float64)[1], forward(p, W, torch.float32)[1]
    return pre64.abs().min().item(), (pre32.double() - pre64).abs().max().item()


def admissible(p, W=None):
    """No position may be undecided: the nearest one is 16 float32 deviations from the kink.  A condition on the
    problem, not a tolerance on the result."""
    nearest, dev = undecided(p, W)
    return nearest > 16 * dev


def tables(it):
    """(step_size, bc2_sqrt) of iteration ``it``: python doubles, as hipsolve.Solver tabulates them (t = it + 1)."""
    t = it + 1
    return LR / (1 - BETA1 ** t), math.sqrt(1 - BETA2 ** t)


def adam(x, m, v, g, step_size, bc2_sqrt):
    """torch.optim.Adam's single-tensor update in the dtype of its operands: (x', m', v')."""
    m = m + (g - m) * (1 - BETA1)
    v = v * BETA2 + (1 - BETA2) * g * g
    return x - step_size * m / (v.sqrt() / bc2_sqrt + EPS), m, v


def _wgrad(p, x, cot, dtype):
    """sum over the positions of cot[o][pos] x[i][pos + tap]: the weight gradient of the scaled convolution alone."""
    V = torch.zeros(1, p.O, p.I, 3, 3, dtype=dtype, requires_grad=True)
    s = 1 / math.sqrt(p.I * 9)
    if p.upsample:
        y = torch.nn.functional.conv_transpose2d(x, s * V.transpose(1, 2).squeeze(0), stride=2)
    else:
        y = torch.nn.functional.conv2d(x, s * V.squeeze(0), padding=1)
    (y * cot).sum().backward()
    return V.grad


def reference_iteration(p, W, m, v, it, low_rank_gradient=False, linear=False, lam=None, dtype=torch.float64):
    """One iteration at weight W with moments m, v (of W; of Lambda, shape (O, rank, 9), for ``linear``).

    Returns loss, pre, raw (the gradient of the loss), g (what Adam sees: raw, projected_conv(raw, context), or the
    (O, rank, 9) cosines), m, v, W (and lam) after the update.  In float64 also ``mag``: per element of g the sum of the
    magnitudes of the terms it is the sum of -- the products over the positions, the demodulation term, and the
    products of the projection -- which is what an element's error is to be held against."""
    W, m, v = W.to(dtype), m.to(dtype), v.to(dtype)
    Wg = W.clone().requires_grad_(True)
    dc = R.demod_conv(p.key.to(dtype), p.style.to(dtype), Wg, p.upsample)
    dc.retain_grad()
    out = dc
    pre = None
    if not p.plain:
        if p.upsample:
            out = R.upfirdn2d(out, p.blur_k.to(dtype), pad=(1, 1))
        hh, ww = out.shape[2:]
        pre = out + p.noise_w.to(dtype) * R.noise_rows(1, hh * ww).to(dtype).view(1, 1, hh, ww)
        pre = pre + p.bias.to(dtype).view(1, -1, 1, 1)
        out = R.fused_leaky_relu(pre, None)
    loss = (p.val.to(dtype) - out).abs().mean()
    loss.backward()
    raw = Wg.grad
    res = types.SimpleNamespace(loss=loss.item(), pre=None if pre is None else pre.detach(), raw=raw)
    mag = None
    if dtype == torch.float64:
        s = 1 / math.sqrt(p.I * 9)
        demod = torch.rsqrt(((s * W * p.style.to(dtype).view(1, 1, -1, 1, 1)) ** 2).sum([2, 3, 4]) + 1e-8)
        cot = dc.grad * demod[:, :, None, None]                     # d loss / d (the scaled convolution)
        first = _wgrad(p, p.key.to(dtype), cot, dtype)
        mag = _wgrad(p, p.key.to(dtype).abs(), cot.abs(), dtype) + (raw - first).abs()
    step_size, bc2_sqrt = tables(it)
    if linear:
        ctx = p.context.to(dtype)
        g = torch.einsum('goiyx,di->godyx', raw, ctx)[0].reshape(p.O, -1, 9)
        if mag is not None:
            mag = torch.einsum('goiyx,di->godyx', mag, ctx.abs())[0].reshape(p.O, -1, 9)
        res.lam, res.m, res.v = adam(lam.to(dtype), m, v, g, step_size, bc2_sqrt)
        res.W = p.W0.to(dtype) + torch.einsum('ody,di->oiy', res.lam, ctx).reshape(W.shape)
    else:
        g = raw
        if low_rank_gradient:
            ctx = p.context.to(dtype)
            g = R.projected_conv(raw, ctx)
            if mag is not None:
                mag = R.projected_conv(mag, ctx.abs())
        res.W, res.m, res.v = adam(W, m, v, g, step_size, bc2_sqrt)
        res.lam = None
    res.g, res.mag = g, mag
    return res
