"""What LPIPS costs on the device (GPU only, one process): rewriting_amd/lpips.py beside a torch.nn twin of the same weights,
interleaved round by round; per tap, the tap kernel's bytes over its time beside a device copy measured in the same run; and
compute_dl over a directory of PNG pairs.

    python scripts/lpips_bench.py [--out profiles/lpips_vgg.json] [--sizes 256,1024] [--batches 1,8] [--pairs 1000]

Per size and batch: one pair's spatial map and its masked scalar, both routes (host clock around synchronises, median of
--runs after --warmup rounds; a round runs the HIP route, then the twin).  Per tap of that size and batch: hip.lpips_tap on
seeded maps by HIP events; its rate is the 2 B C HW 4 bytes it must read over that time.  The copy beside it moves a buffer
of the same number of bytes with Tensor.copy_ (it reads them AND writes them: its rate is quoted as bytes copied per second,
so a tap kernel at the copy's rate reads memory half as fast as the copy touches it).  Weights are seeded random tensors
(no file from outside), which changes no time.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rewriting_amd import distances, hip, lpips, perceptual          # noqa: E402

ALL_LAYERS = perceptual.LAYERS + lpips.TAIL_LAYERS


def seeded_weights(seed=0):
    gen = torch.Generator().manual_seed(seed)
    sd, lins = {}, {}
    for index, in_ch, out_ch, _ in ALL_LAYERS:
        sd['%d.weight' % index] = torch.randn(out_ch, in_ch, 3, 3, generator=gen) * (2.0 / (9 * in_ch)) ** 0.5
        sd['%d.bias' % index] = torch.randn(out_ch, generator=gen) * 0.05
    for k, c in enumerate(lpips.CHANNELS):
        lins['lin%d' % k] = torch.rand(c, generator=gen) * (torch.rand(c, generator=gen) < 0.7)
    return sd, lins


class TorchTwin(torch.nn.Module):
    """LPIPS v0.1 (vgg) from torch.nn.functional on the device: the route a caller had before"""

    def __init__(self, sd, lins, dev):
        super().__init__()
        self.sd = {k: v.to(dev) for k, v in sd.items()}
        self.lins = [lins['lin%d' % k].to(dev) for k in range(5)]
        self.shift = torch.tensor(lpips.SHIFT, device=dev).view(1, 3, 1, 1)
        self.scale = torch.tensor(lpips.SCALE, device=dev).view(1, 3, 1, 1)

    def taps(self, x):
        h = (x - self.shift) / self.scale
        out = []
        for index, _, _, pool in ALL_LAYERS:
            y = F.relu(F.conv2d(h, self.sd['%d.weight' % index], self.sd['%d.bias' % index], padding=1))
            if index in lpips.TAPS:
                out.append(y)
            h = F.max_pool2d(y, 2, 2) if pool else y
        return out

    def forward(self, im0, im1, w=None):
        out = 0
        for f0, f1, lin in zip(self.taps(im0), self.taps(im1), self.lins):
            n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
            n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
            d = (lin[None, :, None, None] * (n0 - n1) ** 2).sum(dim=1, keepdim=True)
            out = out + F.interpolate(d, size=im0.shape[2:], mode='bilinear', align_corners=False)
        if w is None:
            return out
        return torch.sum(out * w, [1, 2, 3]) / torch.sum(w, [1, 2, 3])


def interleaved(fns, runs, warmup):
    """{name: times}: every round runs each of fns once, in order, each between synchronises"""
    times = {name: [] for name in fns}
    for i in range(warmup + runs):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(time.perf_counter() - t0)
    return {name: dict(median_ms=1e3 * statistics.median(t), min_ms=1e3 * min(t), max_ms=1e3 * max(t)) for name, t in times.items()}


def events(fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def measure_pair(size, batch, nets, runs, warmup, dev):
    gen = torch.Generator().manual_seed(size + batch)
    im0 = (torch.rand(batch, 3, size, size, generator=gen) * 2 - 1).to(dev)
    im1 = (im0 + 0.05 * torch.randn(batch, 3, size, size, generator=gen).to(dev)).clamp(-1, 1)
    w = (torch.rand(batch, 1, size, size, generator=gen) > 0.2).float().to(dev)
    res = dict(size=size, batch=batch)
    with torch.no_grad():
        res['spatial_map'] = interleaved({name: (lambda net=net: net(im0, im1)) for name, net in nets.items()}, runs, warmup)
        res['masked_scalar'] = interleaved({name: (lambda net=net: net(im0, im1, w=w)) for name, net in nets.items()}, runs, warmup)
        a, b = nets['hip'](im0, im1, w=w), nets['torch_nn'](im0, im1, w=w)
    res['masked_scalar_rel_difference'] = ((a - b).norm() / b.norm()).item()
    print(json.dumps(res), flush=True)
    return res


def measure_taps(size, batch, runs, warmup, dev):
    rows = []
    for k, c in enumerate(lpips.CHANNELS):
        h = size >> k
        gen = torch.Generator().manual_seed(k)
        f0 = torch.rand(batch, c, h, h, generator=gen).to(dev)
        f1 = (f0 + 0.01 * torch.rand(batch, c, h, h, generator=gen).to(dev))
        lin = torch.rand(c, generator=gen).to(dev)
        nbytes = 2 * batch * c * h * h * 4
        src = torch.empty(nbytes // 4, device=dev)
        dst = torch.empty_like(src)
        tap_ms = events(lambda: hip.lpips_tap(f0, f1, lin), runs, warmup)
        copy_ms = events(lambda: dst.copy_(src), runs, warmup)
        rows.append(dict(tap=k, channels=c, map=[h, h], batch=batch, bytes_read=nbytes, tap_ms=tap_ms,
                         tap_read_GBps=nbytes / tap_ms * 1e-6, copy_ms=copy_ms, copy_GBps_bytes_copied=nbytes / copy_ms * 1e-6))
        print(json.dumps(rows[-1]), flush=True)
        del f0, f1, src, dst
    return rows


def measure_compute_dl(pairs, size, net, dev):
    """seconds of compute_dl over `pairs` PNG pairs of size^2 written here with PIL, per mode"""
    import numpy
    import PIL.Image
    res = dict(pairs=pairs, size=size)
    with tempfile.TemporaryDirectory() as root:
        dirs = {name: os.path.join(root, name) for name in ('before', 'after', 'seg')}
        for d in dirs.values():
            os.makedirs(d)
        rng = numpy.random.RandomState(0)
        base = rng.randint(0, 256, (size, size, 3)).astype(numpy.uint8)
        seg = torch.stack([torch.zeros(size, size, dtype=torch.long), torch.randint(0, 4, (size, size))])
        for k in range(pairs):
            before = numpy.roll(base, k, axis=0)
            after = before.copy()
            after[size // 4:size // 2, size // 4:size // 2] = rng.randint(0, 256, (size // 4, size // 4, 3))
            PIL.Image.fromarray(before).save(os.path.join(dirs['before'], '%d.png' % k))
            PIL.Image.fromarray(after).save(os.path.join(dirs['after'], '%d.png' % k))
            torch.save(seg, os.path.join(dirs['seg'], '%d.pth' % k))
        for mode in distances.MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            total, count = distances.compute_dl(dirs['before'], dirs['after'], dirs['seg'], range(pairs), src=(1,), srcc=1, mode=mode,
                                                batch_size=100, net=net, device=dev)
            torch.cuda.synchronize()
            res[mode] = dict(seconds=time.perf_counter() - t0, total=total, count=count)
            print('compute_dl', mode, json.dumps(res[mode]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips_vgg.json'))
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--batches', default='1,8')
    ap.add_argument('--pairs', type=int, default=1000)
    ap.add_argument('--png-size', type=int, default=256)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sd, lins = seeded_weights()
    nets = dict(hip=lpips.from_state_dicts(sd, lins).to(dev), torch_nn=TorchTwin(sd, lins, dev))
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, warmup=args.warmup, pairs=[], taps=[],
               compute_dl=None)

    def save():
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    for size in (int(s) for s in args.sizes.split(',') if s):
        for batch in (int(b) for b in args.batches.split(',') if b):
            out['taps'].append(measure_taps(size, batch, args.runs, args.warmup, dev))
            save()
            out['pairs'].append(measure_pair(size, batch, nets, args.runs, args.warmup, dev))
            save()
    if args.pairs:
        out['compute_dl'] = measure_compute_dl(args.pairs, args.png_size, nets['hip'], dev)
    save()
    print('wrote', args.out)


if __name__ == '__main__':
    main()
