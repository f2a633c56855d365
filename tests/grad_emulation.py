"""TEST INFRASTRUCTURE -- what the tests of the whole-generator gradients share (tests/test_generator_gradients.py on the
emulated path, tests/test_gpu_generator_gradients.py on the device):

* torch statements of the two wrappers that ``grad.ToRGB.backward`` alone calls (``hip.to_rgb_input_grad``,
  ``hip.to_rgb_weight_sums``), installed ON TOP of the ``emulated_hip`` fixture -- tests/hip_emulation.py patches the
  wrappers that existed before them and stays as it is;
* the recipe of the gradient tests (latent, target, smooth loss) and its oracle: torch.autograd over
  ``oracle.restatement.generator_forward`` on the host, in float64 (the truth) or float32 (the reference's own
  arithmetic, whose distance from the truth is the yardstick ``d_ref``);
* the convolution-free perceptual network of the ``all_weights_insert`` tests and that loop's oracle.
"""
import torch
import torch.nn.functional as F

from oracle import restatement as R


def to_rgb_input_grad(g, weight, style, w_scale):
    return w_scale * style.detach()[:, :, None, None] * torch.einsum('ci,bchw->bihw', weight.detach(), g.detach())


def to_rgb_weight_sums(g, x):
    return torch.einsum('bchw,bihw->bci', g.detach(), x.detach())


def install(monkeypatch):
    """After the emulated_hip fixture: the two wrappers of ToRGB's backward as torch statements."""
    from rewriting_amd import hip
    monkeypatch.setattr(hip, 'to_rgb_input_grad', to_rgb_input_grad)
    monkeypatch.setattr(hip, 'to_rgb_weight_sums', to_rgb_weight_sums)


# ---- the recipe -----------------------------------------------------------------------------------------------------

def recipe(size, seed, batch=2):
    """(z, T): the latent and the target of the smooth loss, on the host."""
    z = torch.randn(batch, 512, generator=torch.Generator().manual_seed(seed))
    target = torch.randn(batch, 3, size, size, generator=torch.Generator().manual_seed(1000 + seed))
    return z, target


def smooth_loss(out, target):
    """Smooth on purpose: an L1 loss adds sign ties to the leaky ReLU's kinks."""
    return (out * target).mean() + 0.5 * out.pow(2).mean()


def oracle_gradients(sd, param_names, z, target, size, truncation, dtype, loss_fn=smooth_loss, decisions=None):
    """torch.autograd over the restatement on the host in `dtype`: (loss, image, {name: gradient} with 'z' for the
    latent).  sd: the model's state dict on the host (float32), param_names: its parameters; decisions: the branch of
    every leaky ReLU, pinned (oracle.restatement.Decisions)."""
    sd = {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
    for name in param_names:
        sd[name].requires_grad_(True)
    z = z.detach().to(dtype).requires_grad_(True)
    out = R.generator_forward(sd, z, size, truncation=truncation, decisions=decisions)
    loss = loss_fn(out, target.to(dtype))
    loss.backward()
    grads = {name: sd[name].grad for name in param_names}
    grads['z'] = z.grad
    return loss.detach(), out.detach(), grads


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def worst_relative_error(grads, truth):
    """max over the tensors of |g - truth| / |truth| (2-norms), and the tensor it is reached on."""
    worst = max(truth, key=lambda name: rel(grads[name], truth[name]))
    return rel(grads[worst], truth[worst]), worst


def model_gradients(model, z, target, loss_fn=smooth_loss):
    """The package's side of the recipe on `model` (any device): (loss, image, {name: gradient} with 'z')."""
    dev = next(model.parameters()).device
    z = z.to(dev).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        out = model(z)
        loss = loss_fn(out, target.to(dev))
        loss.backward()
    grads = {name: p.grad for name, p in model.named_parameters()}
    grads['z'] = z.grad
    return loss.detach(), out.detach(), grads


# ---- all_weights_insert ----------------------------------------------------------------------------------------------

class PooledMix(torch.nn.Module):
    """A perceptual network without a convolution: 2x2 average pooling, then a fixed-seed 1x1 mix of the three colours
    into `features` channels, written as an einsum."""

    def __init__(self, features=8, seed=5):
        super().__init__()
        self.register_buffer('mix', torch.randn(features, 3, generator=torch.Generator().manual_seed(seed)))

    def forward(self, image):
        return torch.einsum('fc,bchw->bfhw', self.mix.to(image.dtype), F.avg_pool2d(image, 2))


def overfit_oracle(sd, param_names, x, z, bounds, size, truncation, niter, lr, feature_net, dtype=torch.float64):
    """The reference's all_weights_insert (rewrite/ganrewrite.py:300-331) over the restatement on the host in `dtype`:
    the losses of its `niter` iterations."""
    sd = {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
    params = [sd[name].requires_grad_(True) for name in param_names]
    x, z = x.detach().to(dtype), z.detach().to(dtype)
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    t, l, b, r = bounds
    for _ in range(niter):
        out = R.generator_forward(sd, z, size, truncation=truncation)
        gt, pred = x[:, :, t:b, l:r], out[:, :, t:b, l:r]
        loss = F.l1_loss(gt, pred) + 1e-2 * F.mse_loss(feature_net(gt), feature_net(pred))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses
