"""TEST INFRASTRUCTURE for rewriting_amd/lpips.py and rewriting_amd/distances.py (tests/test_lpips_host.py,
tests/test_gpu_lpips.py):

* seeded weights of VGG16 features[:30] -- tests/perceptual_checks.random_state_dict for the layers up to 19, its rule (He-scaled
  normal weights, biases of std 0.05) for 21 .. 28 -- and of the lin layers, ``lin_k = rand(C) * (rand(C) < 0.7)``: nonnegative,
  three in ten zero; no file from outside;
* the TWIN: LPIPS v0.1 written from torch.nn.functional in any dtype, on the host.  It is not the module under test;
* the inputs both test files use, and the twin's results on them (computed once, shared, never changed);
* CPU stand-ins for the three wrappers of rw_lpips.hip, installed ON TOP of ``emulated_hip`` and perceptual_checks.install.
"""
import functools
import json
import os

import torch
import torch.nn.functional as F

from rewriting_amd import lpips
from rewriting_amd.perceptual import LAYERS
from tests import perceptual_checks as P

ALL_LAYERS = LAYERS + lpips.TAIL_LAYERS
EPS = 2.0 ** -24
# the longest chain of additions a term of a per-image sum passes through (rw_lpips.hip: 28 per thread, 6 + 3 in the workgroup,
# 16 per thread of the finishing workgroup, 6 + 3 again)
CHAIN = 62


def random_state_dict(seed=0):
    sd = P.random_state_dict(seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    for index, in_ch, out_ch, _ in lpips.TAIL_LAYERS:
        sd['%d.weight' % index] = torch.randn(out_ch, in_ch, 3, 3, generator=gen) * (2.0 / (9 * in_ch)) ** 0.5
        sd['%d.bias' % index] = torch.randn(out_ch, generator=gen) * 0.05
    return sd


def random_lins(seed=0):
    """{'lin{k}.model.1.weight': (1, C, 1, 1)} as LPIPS v0.1 stores them"""
    gen = torch.Generator().manual_seed(seed + 2000)
    out = {}
    for k, c in enumerate(lpips.CHANNELS):
        lin = torch.rand(c, generator=gen) * (torch.rand(c, generator=gen) < 0.7)
        out['lin%d.model.1.weight' % k] = lin.view(1, c, 1, 1)
    return out


def lin_list(lins):
    return [lins['lin%d.model.1.weight' % k].reshape(-1) for k in range(len(lpips.CHANNELS))]


def tap_distance(f0, f1, lin, dtype):
    """one tap, (B, 1, H, W): the formula as LPIPS writes it"""
    f0, f1, lin = f0.to(dtype), f1.to(dtype), lin.to(dtype)
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    return (lin[None, :, None, None] * (n0 - n1) ** 2).sum(dim=1, keepdim=True)


def tap_features(sd, x, dtype):
    """the five taps of features[:30] of the scaled image"""
    shift = torch.tensor(lpips.SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(lpips.SCALE, dtype=dtype).view(1, 3, 1, 1)
    h = (x.to(dtype) - shift) / scale
    taps = []
    for index, _, _, pool in ALL_LAYERS:
        y = F.relu(F.conv2d(h, sd['%d.weight' % index].to(dtype), sd['%d.bias' % index].to(dtype), padding=1))
        if index in lpips.TAPS:
            taps.append(y)
        h = F.max_pool2d(y, 2, 2) if pool else y
    return taps


def twin(sd, lins, im0, im1, dtype, w=None, spatial=True, taps=None):
    """LPIPS v0.1 (vgg) in `dtype` on the host; taps: a list that receives the five d_k (B, 1, h_k, w_k)"""
    size = tuple(im0.shape[2:])
    ds = [tap_distance(f0, f1, lin, dtype)
          for f0, f1, lin in zip(tap_features(sd, im0, dtype), tap_features(sd, im1, dtype), lin_list(lins))]
    if taps is not None:
        taps.extend(ds)
    if spatial:
        out = sum(F.interpolate(d, size=size, mode='bilinear', align_corners=False) for d in ds)
    else:
        out = sum(d.mean(dim=(2, 3), keepdim=True) for d in ds)
    if w is None:
        return out
    w = w.to(dtype)
    return torch.sum(out * w, [1, 2, 3]) / torch.sum(w, [1, 2, 3])


# ---- the inputs of the kernel tests (tests/test_gpu_lpips.py, tests/test_gpu_lpips_grad.py) ----------------------------------
def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def on_device(t, offset=0):
    """t on the device, `offset` floats past an allocation's start (a contiguous view: the wrappers read it in place)"""
    flat = torch.empty(t.numel() + offset, device='cuda', dtype=t.dtype)
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * offset
    return view


# The tap kernel's and its adjoint's cases: (shape of f0, batch of f1, offset of f0 in floats).  (2,64,8,8): 16-byte loads (and,
# in the adjoint, stores), one tile per image; with f1 of batch 1; with f0 at a 4-byte offset (the scalar staging); (1,512,2,2):
# 16 pixels per tile narrowed to 4, 64 channel groups; (1,128,5,7): an odd map, two tiles of 32 pixels, the second with three;
# (1,256,1,1): one pixel, 256 channel groups; (1,5,3,3): fewer channels than groups; (1,64,12,12): three tiles per image, the
# last one short; (1,8200,2,2): more channels than LDS holds -- the form that reads global memory twice
TAP_CASES = [((2, 64, 8, 8), 2, 0), ((2, 64, 8, 8), 1, 0), ((2, 64, 8, 8), 2, 1), ((1, 512, 2, 2), 1, 0), ((1, 128, 5, 7), 1, 0),
             ((1, 256, 1, 1), 1, 0), ((1, 5, 3, 3), 1, 0), ((1, 64, 12, 12), 1, 0), ((1, 8200, 2, 2), 1, 0)]


# ---- the inputs of the module tests -------------------------------------------------------------------------------------
SHAPES = [(2, 3, 32, 32), (1, 3, 20, 28), (1, 3, 16, 16)]
KINDS = ('independent', 'near', 'box')


def pair(shape, kind):
    """(im0, im1) in [-1, 1]: independent; near (+ 0.02 noise, clamped); box (an 8 x 8 region changed by 0.3 noise)"""
    gen = torch.Generator().manual_seed(100 * shape[2] + shape[3] + KINDS.index(kind))
    im0 = torch.rand(*shape, generator=gen) * 2 - 1
    if kind == 'independent':
        im1 = torch.rand(*shape, generator=gen) * 2 - 1
    elif kind == 'near':
        im1 = (im0 + 0.02 * torch.randn(*shape, generator=gen)).clamp(-1, 1)
    else:
        im1 = im0.clone()
        im1[:, :, 4:12, 6:14] = (im0[:, :, 4:12, 6:14] + 0.3 * torch.randn(shape[0], 3, 8, 8, generator=gen)).clamp(-1, 1)
    return im0, im1


def mask(shape):
    """(B, 1, H, W) of zeros and ones: everything but a box that differs per image"""
    w = torch.ones(shape[0], 1, shape[2], shape[3])
    for b in range(shape[0]):
        w[b, :, 2 + b:10 + b, 5:13 + b] = 0
    return w


def edit_set(n=4, size=32):
    """(before, after, seg): n images, a 12 x 12 region changed by 0.3 noise, a segmentation of classes 0 .. 3 with the region in class 1"""
    gen = torch.Generator().manual_seed(77)
    before = torch.rand(n, 3, size, size, generator=gen) * 2 - 1
    after = before.clone()
    after[:, :, 8:20, 10:22] = (before[:, :, 8:20, 10:22] + 0.3 * torch.randn(n, 3, 12, 12, generator=gen)).clamp(-1, 1)
    seg = torch.randint(0, 4, (n, size, size), generator=gen)
    seg[:, 8:20, 10:22] = 1
    return before, after, seg


@functools.lru_cache(maxsize=None)
def weights():
    return random_state_dict(0), random_lins(0)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """{dtype: (spatial map, [d_k], masked scalar)} of the twin on pair(shape, kind) with mask(shape)"""
    sd, lins = weights()
    im0, im1 = pair(shape, kind)
    out = {}
    for dtype in (torch.float64, torch.float32):
        taps = []
        spatial = twin(sd, lins, im0, im1, dtype, taps=taps)
        w = mask(shape).to(dtype)
        out[dtype] = (spatial, taps, torch.sum(spatial * w, [1, 2, 3]) / torch.sum(w, [1, 2, 3]))
    return out


rel = P.rel


def report(section, figures):
    """into lpips.json of perceptual_checks.report"""
    P.report('lpips.json', section, figures)


# ---- CPU stand-ins for the wrappers of rw_lpips.hip ----------------------------------------------------------------------

def lpips_tap(f0, f1, lin):
    return tap_distance(f0.detach(), f1.detach(), lin.detach(), f0.dtype)[:, 0]


def apply_tables(d, idx, lam, size):
    """the bilinear up-sampling of d (B, h, w) to `size` with one tap's rows of the tables of lpips.device_tables"""
    h, w = size
    y0, y1, x0, x1 = (t.long() for t in (idx[:h], idx[h:2 * h], idx[2 * h:2 * h + w], idx[2 * h + w:]))
    ly, lx = lam[:h].to(d.dtype)[None, :, None], lam[h:].to(d.dtype)[None, None, :]
    top = (1 - lx) * d[:, y0][:, :, x0] + lx * d[:, y0][:, :, x1]
    bot = (1 - lx) * d[:, y1][:, :, x0] + lx * d[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def lpips_combine(taps, tables, size, weight=None, want_map=True, want_sums=False):
    idx, lam = tables
    out = sum(apply_tables(d.detach(), idx[k], lam[k], size) for k, d in enumerate(taps))[:, None]
    sums = None
    if want_sums:
        wt = torch.ones_like(out) if weight is None else weight.detach().expand_as(out)
        sums = torch.stack([(out * wt).sum((1, 2, 3)), wt.sum((1, 2, 3))], dim=1)
    return (out if want_map else None), sums


def masked_l1(a, b, mask):
    diff = (a.detach() - b.detach()).abs().sum(dim=1)
    m = mask.detach().expand_as(diff)
    return torch.stack([(diff * m).sum((1, 2)), m.sum((1, 2))], dim=1)


STAND_INS = ('lpips_tap', 'lpips_combine', 'masked_l1')


def install(monkeypatch, log=None):
    """After the emulated_hip fixture: the wrappers of rw_percept.hip and rw_lpips.hip as torch statements; log: a list that
    receives (name, positional arguments, keyword arguments) of every call."""
    from rewriting_amd import hip
    P.install(monkeypatch, log)

    def logged(name, fn):
        def call(*args, **kwargs):
            if log is not None:
                log.append((name, args, kwargs))
            return fn(*args, **kwargs)
        return call
    for name in STAND_INS:
        monkeypatch.setattr(hip, name, logged(name, globals()[name]))
