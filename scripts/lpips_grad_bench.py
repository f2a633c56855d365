"""What LPIPS costs as a LOSS on the device (GPU only, one process): ``LPIPS.loss`` + ``backward`` of rewriting_amd/lpips.py
beside the torch.nn twin of scripts/lpips_bench.py under torch autograd, interleaved round by round; the same iteration with
a reused ``target``; one backward with every wrapper call timed by itself; and, per tap, the tap adjoint's bytes over its time beside a device copy of as many bytes.

    python scripts/lpips_grad_bench.py [--out profiles/lpips_grad.json] [--cases 256x1,256x8,1024x1]

Per case (size x batch): one pair's masked scalar, forward and backward to im0 (host clock around synchronises, median of
--runs after --warmup rounds; a round runs the HIP route, the HIP route on a reused target, then the twin).  The backward
alone is timed the same way on a graph recorded before the clock starts.  Per tap at the --tap-size: hip.lpips_tap_grad with
acc and relu_mask by HIP events; its bytes are the two maps it reads, acc, and the map it writes (4 B C HW 4), the copy
beside it moves a buffer of that many bytes counted once (Tensor.copy_ reads AND writes them).  Weights are seeded random
tensors, which changes no time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import lpips_bench as LB                                             # noqa: E402
from rewriting_amd import hip, lpips                                 # noqa: E402


def measure_case(size, batch, nets, runs, warmup, dev):
    gen = torch.Generator().manual_seed(size + batch)
    im0 = (torch.rand(batch, 3, size, size, generator=gen) * 2 - 1).to(dev)
    im1 = (im0 + 0.05 * torch.randn(batch, 3, size, size, generator=gen).to(dev)).clamp(-1, 1)
    w = (torch.rand(batch, 1, size, size, generator=gen) > 0.2).float().to(dev)
    target = nets['hip'].target(im1)
    grads = {}

    def iteration(name, value_of):
        leaf = im0.clone().requires_grad_(True)
        value_of(leaf).sum().backward()
        grads[name] = leaf.grad

    routes = {'hip': lambda x: nets['hip'].loss(x, im1, w=w), 'hip_reused_target': lambda x: nets['hip'].loss(x, target, w=w),
              'torch_nn': lambda x: nets['torch_nn'](x, im1, w=w)}
    res = dict(size=size, batch=batch)
    res['loss_and_backward'] = LB.interleaved({name: (lambda name=name, fn=fn: iteration(name, fn)) for name, fn in routes.items()},
                                              runs, warmup)
    # the backward alone: a fresh graph per run, recorded outside the clock
    alone = {name: [] for name in ('hip', 'torch_nn')}
    for i in range(warmup + runs):
        for name in alone:
            leaf = im0.clone().requires_grad_(True)
            value = routes[name](leaf).sum()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value.backward()
            torch.cuda.synchronize()
            if i >= warmup:
                alone[name].append(time.perf_counter() - t0)
            del leaf, value
    res['backward_alone'] = {name: dict(median_ms=1e3 * statistics.median(t), min_ms=1e3 * min(t), max_ms=1e3 * max(t))
                             for name, t in alone.items()}
    res['gradient_rel_difference'] = ((grads['hip'] - grads['torch_nn']).norm() / grads['torch_nn'].norm()).item()
    res['reused_target_same_bits'] = bool(torch.equal(grads['hip'], grads['hip_reused_target']))
    print(json.dumps(res), flush=True)
    return res


BACKWARD_LAUNCHES = ('lpips_combine_grad', 'lpips_tap_grad', 'bias_relu_pool_grad', 'conv3x3', 'conv3x3_wino', 'conv3x3_rgb_input_grad')


def backward_breakdown(size, batch, net, dev):
    """{wrapper: (calls, ms)} of ONE backward of the HIP route with a synchronise around every wrapper call: which launches
    carry the time (the sum exceeds the un-instrumented backward by the synchronises)"""
    gen = torch.Generator().manual_seed(size + batch)
    im0 = (torch.rand(batch, 3, size, size, generator=gen) * 2 - 1).to(dev)
    target = net.target((im0 + 0.05 * torch.randn(batch, 3, size, size, generator=gen).to(dev)).clamp(-1, 1))
    spent = {name: [0, 0.0] for name in BACKWARD_LAUNCHES}
    plain = {name: getattr(hip, name) for name in BACKWARD_LAUNCHES}

    def timed(name):
        def call(*args, **kwargs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = plain[name](*args, **kwargs)
            torch.cuda.synchronize()
            spent[name][0] += 1
            spent[name][1] += 1e3 * (time.perf_counter() - t0)
            return result
        return call
    for _ in range(2):                                              # the second run is the one reported (packed weights exist)
        leaf = im0.clone().requires_grad_(True)
        value = net.loss(leaf, target).sum()
        for name in spent:
            spent[name] = [0, 0.0]
            setattr(hip, name, timed(name))
        try:
            value.backward()
        finally:
            for name in plain:
                setattr(hip, name, plain[name])
    res = dict(size=size, batch=batch, launches={name: dict(calls=c, ms=ms) for name, (c, ms) in spent.items()})
    print(json.dumps(res), flush=True)
    return res


def measure_tap_grads(size, batch, runs, warmup, dev):
    rows = []
    for k, c in enumerate(lpips.CHANNELS):
        h = size >> k
        gen = torch.Generator().manual_seed(k)
        f0 = torch.relu(torch.randn(batch, c, h, h, generator=gen)).to(dev)
        f1 = torch.relu(f0 + 0.01 * torch.randn(batch, c, h, h, generator=gen).to(dev))
        lin = torch.rand(c, generator=gen).to(dev)
        gd = torch.rand(batch, h, h, generator=gen).to(dev)
        acc = torch.randn(batch, c, h, h, generator=gen).to(dev)
        nbytes = 4 * batch * c * h * h * 4
        src = torch.empty(nbytes // 4, device=dev)
        dst = torch.empty_like(src)
        grad_ms = LB.events(lambda: hip.lpips_tap_grad(f0, f1, lin, gd, acc=acc, relu_mask=True, out=acc), runs, warmup)
        copy_ms = LB.events(lambda: dst.copy_(src), runs, warmup)
        rows.append(dict(tap=k, channels=c, map=[h, h], batch=batch, bytes_moved=nbytes, tap_grad_ms=grad_ms,
                         tap_grad_GBps=nbytes / grad_ms * 1e-6, copy_ms=copy_ms, copy_GBps_bytes_copied=nbytes / copy_ms * 1e-6))
        print(json.dumps(rows[-1]), flush=True)
        del f0, f1, acc, src, dst
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips_grad.json'))
    ap.add_argument('--cases', default='256x1,256x8,1024x1')
    ap.add_argument('--tap-size', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sd, lins = LB.seeded_weights()
    nets = dict(hip=lpips.from_state_dicts(sd, lins).to(dev), torch_nn=LB.TorchTwin(sd, lins, dev))
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, warmup=args.warmup, cases=[], breakdown=[], taps=[])

    def save():
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    for case in (c for c in args.cases.split(',') if c):
        size, batch = (int(v) for v in case.split('x'))
        out['cases'].append(measure_case(size, batch, nets, args.runs, args.warmup, dev))
        save()
        out['breakdown'].append(backward_breakdown(size, batch, nets['hip'], dev))
        save()
    if args.tap_size:
        out['taps'] = measure_tap_grads(args.tap_size, 1, args.runs, args.warmup, dev)
    save()
    print('wrote', args.out)


if __name__ == '__main__':
    main()
