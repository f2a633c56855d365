"""TEST INFRASTRUCTURE for LPIPS as a loss (rewriting_amd/lpips.py: LPIPS.loss, OverfitTerm; tests/test_lpips_grad_host.py,
tests/test_gpu_lpips_grad.py), on top of tests/lpips_checks.py and tests/perceptual_checks.py:

* the TWIN of tests/lpips_checks.py under torch autograd, with two changes: ``forced=`` makes all thirteen layers take given
  ReLU and max-pool decisions (read from the ``trace=`` of the device's ``loss`` with ``decisions()``), as
  perceptual_checks.twin does for nine; and the norm's gradient at an all-zero pixel is 0, not NaN;
* the dense matrices of the up-sampling tables, for the adjoint of the combine step in float64;
* CPU stand-ins for the two wrappers of the adjoint kernels, written from the formulas of include/rewriting_hip.h.
"""
import json
import os

import torch
import torch.nn.functional as F

from rewriting_amd import lpips
from tests import lpips_checks as L
from tests import perceptual_checks as P

MARGIN = 8                              # d_hip <= MARGIN * d_ref
D_REF_MAX = 1e-5                        # the condition on the reference alone (DESIGN sections 8.1, 8.6)


def safe_norm(f):
    """|f| over the channels, (B, 1, H, W), with gradient 0 where the vector is zero"""
    s = torch.sum(f ** 2, dim=1, keepdim=True)
    pos = s > 0
    return torch.sqrt(torch.where(pos, s, torch.ones_like(s))) * pos


def tap_distance(f0, f1, lin, dtype):
    """lpips_checks.tap_distance with the zero-safe norm: the same values"""
    f0, f1, lin = f0.to(dtype), f1.to(dtype), lin.to(dtype)
    n0 = f0 / (safe_norm(f0) + 1e-10)
    n1 = f1 / (safe_norm(f1) + 1e-10)
    return (lin[None, :, None, None] * (n0 - n1) ** 2).sum(dim=1, keepdim=True)


def decisions(trace):
    """[(y > 0, first maximum of every window or None)] of the thirteen blocks, from the maps ``loss(trace=)`` left"""
    return [(y.cpu() > 0, P.first_max(y.cpu()) if pool else None) for y, (_, _, _, pool) in zip(trace, L.ALL_LAYERS)]


def tap_features(sd, x, dtype, forced=None, own=None):
    """lpips_checks.tap_features; forced: the decisions it takes instead of its own; own: receives its own"""
    shift = torch.tensor(lpips.SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(lpips.SCALE, dtype=dtype).view(1, 3, 1, 1)
    h = (x.to(dtype) - shift) / scale
    taps = []
    for n, (index, _, _, pool) in enumerate(L.ALL_LAYERS):
        pre = F.conv2d(h, sd['%d.weight' % index].to(dtype), sd['%d.bias' % index].to(dtype), padding=1)
        if own is not None:
            act = F.relu(pre.detach())
            own.append((act > 0, P.first_max(act) if pool else None))
        if forced is None:
            y = F.relu(pre)
            h = F.max_pool2d(y, 2, 2) if pool else y
        else:
            mask, index_of = forced[n]
            y = pre * mask.to(dtype)
            h = P.windows(y).gather(-1, index_of[..., None])[..., 0] if pool else y
        if index in lpips.TAPS:
            taps.append(y)
    return taps


def twin(sd, lins, im0, im1, dtype, w=None, spatial=True, forced=None, own=None):
    """(B,): what LPIPS.loss returns, in `dtype` on the host; im0's network takes `forced`, im1's its own decisions"""
    size = tuple(im0.shape[2:])
    with torch.no_grad():
        taps1 = tap_features(sd, im1, dtype)
    ds = [tap_distance(f0, f1, lin, dtype)
          for f0, f1, lin in zip(tap_features(sd, im0, dtype, forced, own), taps1, L.lin_list(lins))]
    if spatial:
        out = sum(F.interpolate(d, size=size, mode='bilinear', align_corners=False) for d in ds)
    else:
        out = sum(d.mean(dim=(2, 3), keepdim=True) for d in ds).expand(im0.shape[0], 1, *size)
    w = torch.ones(1, 1, *size, dtype=dtype) if w is None else w.to(dtype)
    w = w.expand(im0.shape[0], 1, *size)
    return torch.sum(out * w, [1, 2, 3]) / torch.sum(w, [1, 2, 3])


def twin_gradient(im0, im1, dtype, forced, w=None, spatial=True, upstream=None, own=None):
    """(value (B,), d (sum_b upstream_b value_b) / d im0) of the twin on lpips_checks.weights(); upstream: ones"""
    sd, lins = L.weights()
    leaf = im0.clone().to(dtype).requires_grad_(True)
    value = twin(sd, lins, leaf, im1, dtype, w=w, spatial=spatial, forced=forced, own=own)
    up = torch.ones_like(value) if upstream is None else upstream.to(dtype)
    (value * up).sum().backward()
    return value.detach(), leaf.grad


def axis_matrix(n_in, n_out, dtype=torch.float64, lam=None):
    """(n_out, n_in): the up-sampling along one axis as a matrix, from lpips.upsample_table (lam: another weight row, e.g.
    the float32 one the device reads)"""
    i0, i1, lam64 = (torch.from_numpy(t.copy()) for t in lpips.upsample_table(n_in, n_out))
    lam = lam64 if lam is None else lam
    m = torch.zeros(n_out, n_in, dtype=dtype)
    rows = torch.arange(n_out)
    m.index_put_((rows, i0.long()), (1 - lam.to(dtype)), accumulate=True)
    m.index_put_((rows, i1.long()), lam.to(dtype), accumulate=True)
    return m


def report(section, figures):
    """into lpips_grad.json of perceptual_checks.report"""
    P.report('lpips_grad.json', section, figures)


# ---- CPU stand-ins for the two adjoint wrappers --------------------------------------------------------------------------

def lpips_tap_grad(f0, f1, lin, gd, acc=None, relu_mask=False, out=None):
    f0, f1, lin, gd = f0.detach(), f1.detach(), lin.detach()[None, :, None, None], gd.detach()[:, None]
    r0 = torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True))
    den0 = r0 + 1e-10
    den1 = torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10
    t = f0 / den0 - f1 / den1
    s = torch.sum(lin * t * f0, dim=1, keepdim=True)
    live = r0 > 0
    safe = torch.where(live, r0, torch.ones_like(r0))
    own = gd * (2 / den0) * (lin * t - f0 * (s / safe / den0)) * live
    if relu_mask:
        own = own * (f0 > 0)
    result = own if acc is None else acc.detach() + own
    if out is not None:
        out.detach().copy_(result)
        return out.detach()
    return result


def lpips_combine_grad(tap_sizes, tables, ranges, size, gscale, weight=None):
    idx, lam = tables
    h, w = size
    b = gscale.shape[0]
    wt = torch.ones(b, h, w, dtype=gscale.dtype) if weight is None else weight.detach()[:, 0].expand(b, h, w)
    grads, at = [], 0
    for k, (hk, wk) in enumerate(tap_sizes):
        my = axis_matrix(hk, h, gscale.dtype, lam[k, :h])
        mx = axis_matrix(wk, w, gscale.dtype, lam[k, h:])
        # the ranges hold every non-zero of the two matrices
        for m, n in ((my, hk), (mx, wk)):
            lo, hi = ranges[at:at + n], ranges[at + n:at + 2 * n]
            o = torch.arange(m.shape[0])[:, None]
            assert not bool((m != 0)[(o < lo[None]) | (o >= hi[None])].any())
            at += 2 * n
        grads.append(gscale.detach()[:, None, None] * torch.einsum('oi,bop,pj->bij', my, wt, mx))
    assert at == ranges.numel()
    return grads


STAND_INS = ('lpips_tap_grad', 'lpips_combine_grad')


def install(monkeypatch, log=None):
    """After the emulated_hip fixture: lpips_checks.install and the two adjoint wrappers as torch statements"""
    from rewriting_amd import hip
    L.install(monkeypatch, log)

    def logged(name, fn):
        def call(*args, **kwargs):
            if log is not None:
                log.append((name, args, kwargs))
            return fn(*args, **kwargs)
        return call
    for name in STAND_INS:
        monkeypatch.setattr(hip, name, logged(name, globals()[name]))
