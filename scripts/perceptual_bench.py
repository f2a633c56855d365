"""What the perceptual network costs (GPU only, one process): VGG16 features[:21] on the HIP kernels
(rewriting_amd/perceptual.py) beside a plain torch.nn VGG of the same weights -- the route a caller had before, through
feature_net= -- timed in the same process.

    python scripts/perceptual_bench.py [--out profiles/perceptual_vgg16.json] [--sizes 256,1024] [--loop-size 256]

Per size, batch 1: the forward under no_grad and the forward with the input gradient of 1e-2 * mse(VF(gt), VF(pred)) (VF
twice forward, once backward: the perceptual term of one overfit iteration), both routes; per block of the HIP route the
forward time by HIP events, the route its convolution takes (F(2x2,3x3) or the direct sum) and the share of the fp32 MFMA
rate its matrix products reach (multiplications the route really does -- a direct sum's divided by 2.25 for F(2x2,3x3) --
over the time of the whole block, bias + ReLU + pool included, against 157.3 TFLOP/s).  Then one all_weights_insert
iteration of the --loop-size generator with either network.  Host clock around synchronises, median of --runs after
--warmup steps; weights are seeded random tensors (no file from outside), which changes no time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                            # noqa: E402
from rewriting_amd import hip, perceptual               # noqa: E402
from rewriting_amd.rewrite import ganrewrite            # noqa: E402
from rewriting_amd.utils import zdataset                # noqa: E402

FP32_MFMA_TFLOPS = 157.3


def seeded_weights(seed=0):
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for index, in_ch, out_ch, _ in perceptual.LAYERS:
        sd['%d.weight' % index] = torch.randn(out_ch, in_ch, 3, 3, generator=gen) * (2.0 / (9 * in_ch)) ** 0.5
        sd['%d.bias' % index] = torch.randn(out_ch, generator=gen) * 0.05
    return sd


def torch_vgg(sd, dev):
    """torchvision's vgg16().features[:21] as plain torch.nn modules with the weights of sd, frozen"""
    layers = []
    for index, in_ch, out_ch, pool in perceptual.LAYERS:
        conv = torch.nn.Conv2d(in_ch, out_ch, 3, padding=1)
        conv.weight.data.copy_(sd['%d.weight' % index])
        conv.bias.data.copy_(sd['%d.bias' % index])
        layers += [conv, torch.nn.ReLU()] + ([torch.nn.MaxPool2d(2, 2)] if pool else [])
    net = torch.nn.Sequential(*layers).to(dev).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def wall(fn, runs, warmup):
    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * statistics.median(times), min_ms=1e3 * min(times), max_ms=1e3 * max(times))


def block_times(net, x, runs, warmup):
    """per block: median forward milliseconds by HIP events (no_grad, nothing kept), route, share of the MFMA rate"""
    blocks = net.blocks()
    samples = [[] for _ in blocks]
    shapes = []
    with torch.no_grad():
        for i in range(warmup + runs):
            h = x
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(blocks) + 1)]
            marks[0].record()
            for n, block in enumerate(blocks):
                if i == 0:
                    shapes.append(tuple(h.shape))
                _, h = block.activate(h, keep=False)
                marks[n + 1].record()
            torch.cuda.synchronize()
            if i >= warmup:
                for n in range(len(blocks)):
                    samples[n].append(marks[n].elapsed_time(marks[n + 1]))
    rows = []
    for (index, in_ch, out_ch, pool), shape, ms in zip(perceptual.LAYERS, shapes, samples):
        b, _, hh, ww = shape
        t = statistics.median(ms)
        direct_flop = 2.0 * 9 * in_ch * out_ch * hh * ww * b
        if in_ch == 3:
            route, done = 'conv3x3_rgb (vector pipe)', direct_flop
        elif hip.wino_supported(out_ch, in_ch, hh, ww):
            route, done = 'conv3x3_wino F(2x2,3x3)', direct_flop / 2.25
        else:
            route, done = 'conv3x3 direct', direct_flop
        rows.append(dict(layer=index, in_ch=in_ch, out_ch=out_ch, map=[hh, ww], pool=pool, route=route, ms=t,
                         direct_gflop=direct_flop * 1e-9, tflops_direct_equivalent=direct_flop / t * 1e-9,
                         share_of_fp32_mfma_rate=None if in_ch == 3 else done / t * 1e-9 / FP32_MFMA_TFLOPS))
    return rows


def perceptual_term(net, gt, pred):
    """the perceptual term of one overfit iteration and its gradient to pred"""
    pred.grad = None
    (1e-2 * F.mse_loss(net(gt), net(pred))).backward()


def measure_size(size, nets, runs, warmup, dev):
    gen = torch.Generator().manual_seed(size)
    gt = torch.randn(1, 3, size, size, generator=gen).to(dev)
    pred = torch.randn(1, 3, size, size, generator=gen).to(dev).requires_grad_(True)
    res = dict(size=size, batch=1)
    for name, net in nets.items():
        def forward(net=net):
            with torch.no_grad():
                net(gt)
        res[name] = dict(forward_no_grad=wall(forward, runs, warmup),
                         two_forwards_and_input_gradient=wall(lambda net=net: perceptual_term(net, gt, pred), runs, warmup))
        print(size, name, json.dumps(res[name]), flush=True)
    res['hip_blocks'] = block_times(nets['hip'], gt, runs, warmup)
    for row in res['hip_blocks']:
        print(size, json.dumps(row), flush=True)
    return res


def measure_loop(size, nets, runs, warmup, dev):
    """milliseconds of one all_weights_insert iteration (crop: the middle half), per network, and without one"""
    res = dict(size=size, bounds=[size // 4, size // 4, 3 * size // 4, 3 * size // 4])
    for name, net in nets.items():
        g = bench.build_generator(size, dev)
        gw = ganrewrite.SeqStyleGanRewriter(g, zdataset.z_dataset_for_model(g, size=4), 8, cachedir=None)
        z = gw.get_z(0)
        with torch.no_grad():
            x = gw.model(gw.get_z(1))
        stamps = []

        def after_step(it, loss):
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        gw.all_weights_insert(x, z, bounds=tuple(res['bounds']), niter=warmup + runs, lr=0.01, feature_net=net,
                              update_callback=after_step)
        steps = [1e3 * (b - a) for a, b in zip(stamps, stamps[1:])][warmup:]
        res[name] = dict(median_ms=statistics.median(steps), min_ms=min(steps), max_ms=max(steps))
        print('all_weights_insert', size, name, json.dumps(res[name]), flush=True)
        del gw, g
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'perceptual_vgg16.json'))
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--loop-size', type=int, default=256)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sd = seeded_weights()
    nets = dict(hip=perceptual.from_state_dict(sd).to(dev), torch_nn=torch_vgg(sd, dev))
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, warmup=args.warmup,
               fp32_mfma_tflops=FP32_MFMA_TFLOPS, sizes=[], loop=None)
    for size in (int(s) for s in args.sizes.split(',') if s):
        out['sizes'].append(measure_size(size, nets, args.runs, args.warmup, dev))
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if args.loop_size:
        out['loop'] = measure_loop(args.loop_size, nets, args.runs, args.warmup, dev)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
