"""TEST INFRASTRUCTURE for rewriting_amd/perceptual.py (tests/test_perceptual_host.py, tests/test_gpu_perceptual.py):

* seeded weights of VGG16 features[:21] -- He-scaled normal weights, small biases; no file from outside;
* the TWIN: the same network written from torch.nn.functional in any dtype, on the host.  It is not the module under test.
  ``forced=`` makes it take given ReLU and max-pool decisions instead of its own (a decision within rounding of a tie
  flips a gradient by far more than rounding): the decisions are read from the ``trace=`` of the
  device's forward with ``decisions()``;
* CPU stand-ins for the four wrappers of rw_percept.hip, installed ON TOP of the ``emulated_hip`` fixture.
"""
import json
import os

import torch
import torch.nn.functional as F

from rewriting_amd.perceptual import LAYERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_state_dict(seed=0, prefix=''):
    """He-scaled normal weights (std sqrt(2 / (9 in_ch))) and biases of std 0.05, float32, under torchvision's names."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for index, in_ch, out_ch, _ in LAYERS:
        sd['%s%d.weight' % (prefix, index)] = torch.randn(out_ch, in_ch, 3, 3, generator=gen) * (2.0 / (9 * in_ch)) ** 0.5
        sd['%s%d.bias' % (prefix, index)] = torch.randn(out_ch, generator=gen) * 0.05
    return sd


def torchvision_style(sd, seed=1):
    """`sd` as a whole torchvision VGG16 state dict would carry it: features.N.*, the three convolutions past layer 20 and
    the classifier (small stand-ins of the right rank: they are ignored by name)."""
    gen = torch.Generator().manual_seed(seed)
    full = {'features.' + k: v for k, v in sd.items()}
    for index in (21, 24, 26, 28):
        full['features.%d.weight' % index] = torch.randn(8, 8, 3, 3, generator=gen)
        full['features.%d.bias' % index] = torch.randn(8, generator=gen)
    for index in (0, 3, 6):
        full['classifier.%d.weight' % index] = torch.randn(4, 4, generator=gen)
        full['classifier.%d.bias' % index] = torch.randn(4, generator=gen)
    return full


def windows(y):
    """(B, C, H // 2, W // 2, 4): the 2x2 windows of y, their positions in row-major order."""
    b, c, h, w = y.shape
    oh, ow = h // 2, w // 2
    return y[:, :, :2 * oh, :2 * ow].reshape(b, c, oh, 2, ow, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, oh, ow, 4)


def first_max(y):
    """index (0 .. 3) of the first maximum of every window in row-major order (torch.argmax returns the first)"""
    return windows(y).argmax(-1)


def decisions(trace):
    """[(y > 0, first maximum of every window or None)] per block, from the activated maps a forward left in trace=."""
    return [(y.cpu() > 0, first_max(y.cpu()) if pool else None) for y, (_, _, _, pool) in zip(trace, LAYERS)]


def twin(sd, x, dtype, forced=None, outputs=None, own=None):
    """VF(x) in `dtype` on the host.  outputs: a list that receives every block's output (after its pool); own: a list
    that receives the decisions this run would have made itself; forced: the decisions it takes instead."""
    h = x.to(dtype)
    for n, (index, _, _, pool) in enumerate(LAYERS):
        pre = F.conv2d(h, sd['%d.weight' % index].to(dtype), sd['%d.bias' % index].to(dtype), padding=1)
        if own is not None:
            act = F.relu(pre.detach())
            own.append((act > 0, first_max(act) if pool else None))
        if forced is None:
            y = F.relu(pre)
            h = F.max_pool2d(y, 2, 2) if pool else y
        else:
            mask, index_of = forced[n]
            y = pre * mask.to(dtype)
            h = windows(y).gather(-1, index_of[..., None])[..., 0] if pool else y
        if outputs is not None:
            outputs.append(h)
    return h


class Twin(torch.nn.Module):
    """twin() as a feature_net (float64 by default): what tests/generator_gradient_checks.overfit_loss takes."""

    def __init__(self, sd, dtype=torch.float64):
        super().__init__()
        self.sd, self.dtype = sd, dtype

    def forward(self, x):
        return twin(self.sd, x, self.dtype)


def rel(a, want):
    """2-norm relative error of a against want (float64)"""
    want = want.detach().double()
    return ((a.detach().double() - want).norm() / want.norm()).item()


def differing_share(got, own):
    """share of the decisions `got` that differ from `own`: (ReLU, pool)"""
    relu_n = relu_d = pool_n = pool_d = 0
    for (gm, gi), (om, oi) in zip(got, own):
        relu_n += gm.numel()
        relu_d += int((gm != om).sum())
        if gi is not None:
            pool_n += gi.numel()
            pool_d += int((gi != oi).sum())
    return relu_d / max(relu_n, 1), pool_d / max(pool_n, 1)


def report(file_name, section, figures):
    """figures as `section` of file_name (perceptual.json here; lpips_checks and lpips_grad_checks name their own) in the
    directory RW_REPORT_DIR names (default: test_reports/, which git ignores)"""
    directory = os.environ.get('RW_REPORT_DIR') or os.path.join(ROOT, 'test_reports')
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, file_name)
    data = {}
    if os.path.isfile(path):
        with open(path) as f:
            data = json.load(f)
    data[section] = figures
    with open(path, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---- CPU stand-ins for the wrappers of rw_percept.hip ------------------------------------------------------------------

def bias_relu_pool(x, bias, pool=False, keep=True, out=None):
    y = F.relu(x.detach() + bias.detach()[None, :, None, None])
    pooled = F.max_pool2d(y, 2, 2) if pool else None
    if keep and out is not None:
        out.detach().copy_(y)
        y = out.detach()
    return (y if keep else None), pooled


def bias_relu_pool_grad(g, y, pooled=False):
    y = y.detach()
    if not pooled:
        return g.detach() * (y > 0)
    with torch.enable_grad():
        leaf = y.clone().requires_grad_(True)
        F.max_pool2d(leaf, 2, 2).backward(g.detach())
    return leaf.grad * (y > 0)


def conv3x3_rgb(x, weight, bias):
    return F.relu(F.conv2d(x.detach(), weight.detach(), bias.detach(), padding=1))


def conv3x3_rgb_input_grad(g, weight):
    return F.conv_transpose2d(g.detach(), weight.detach(), padding=1)


STAND_INS = ('bias_relu_pool', 'bias_relu_pool_grad', 'conv3x3_rgb', 'conv3x3_rgb_input_grad')


def install(monkeypatch, log=None):
    """After the emulated_hip fixture: the four wrappers as torch statements; log: a list that receives
    (name, positional arguments, keyword arguments) of every call."""
    from rewriting_amd import hip

    def logged(name, fn):
        def call(*args, **kwargs):
            if log is not None:
                log.append((name, args, kwargs))
            return fn(*args, **kwargs)
        return call
    for name in STAND_INS:
        monkeypatch.setattr(hip, name, logged(name, globals()[name]))
