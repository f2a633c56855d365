"""What a repaint of the UI's twelve result tiles costs (GPU only, one process): render_image_batch of 12 seeds with a
key, a level and border_color=[255, 255, 255] -- repaint_canvas_array's call -- on the host route (utils/imgviz.py, one
image at a time on the CPU) and on the device route (device_render=True: hip.render_bytes, one copy to the host), and
the overlay kernel alone with the bytes it moves over its time.

    python scripts/render_bench.py [--out profiles/render_overlay.json] [--sizes 256,1024]

Layer 8 of the 256^2 and of the 1024^2 generator.  The two routes alternate in one process; every figure is the median
of --runs (>= 7) runs after --warmup runs.  A repaint ends on the host, so it is timed with a clock around a
synchronise; the kernel by HIP events.  Byte counts come from the shapes: the kernel reads 12 bytes and writes 3 per
pixel (the heat map is a few KiB).  There is no fallback: without a GPU the script fails.
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
import bench                                            # noqa: E402
from rewriting_amd import hip                           # noqa: E402
from rewriting_amd.rewrite import ganrewrite            # noqa: E402
from rewriting_amd.utils import zdataset                # noqa: E402

LAYER = 8
SEEDS = list(range(12))
BORDER = [255, 255, 255]


def spread(times):
    return dict(median_s=statistics.median(times), min_s=min(times), max_s=max(times))


def alternate(routes, runs, warmup):
    """routes: name -> fn.  Each run times every route once, in turn; synchronised at both ends."""
    times = {name: [] for name in routes}
    for i in range(warmup + runs):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(time.perf_counter() - t0)
    return {name: spread(t) for name, t in times.items()}


def device_time(fn, runs, warmup):
    times = []
    for i in range(warmup + runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= warmup:
            times.append(start.elapsed_time(stop) * 1e-3)
    return spread(times)


def measure(size, runs, warmup, dev):
    res = dict(size=size, layer=LAYER, seeds=len(SEEDS))
    g = bench.build_generator(size, dev)
    zds = zdataset.z_dataset_for_model(g, size=max(SEEDS) + 1)
    gw = ganrewrite.SeqStyleGanRewriter(g, zds, LAYER)
    res['key_map_shape'] = list(gw.k_shape)
    torch.manual_seed(0)
    key = torch.randn(gw.k_shape[1], device=dev)
    key = key / key.norm()
    with torch.no_grad():
        zb = torch.cat([gw.get_z(n) for n in SEEDS[:3]])
        images = gw.rendered_image(gw.sample_image_from_latent(zb)).contiguous()
        heat = (gw.context_acts(gw.context_model(zb)) * key[None, :, None, None]).sum(dim=1).contiguous()
    level = heat.reshape(-1).sort()[0][int(heat.numel() * 0.97)].item()
    res['level'] = level

    def repaint(flag):
        def fn():
            gw.device_render = flag
            return gw.render_image_batch(SEEDS, key, level, border_color=BORDER)
        return fn
    res.update(alternate(dict(repaint_host_route=repaint(False), repaint_device_route=repaint(True)), runs, warmup))
    res['host_over_device'] = res['repaint_host_route']['median_s'] / res['repaint_device_route']['median_s']

    # the share of a repaint that is not the overlay: the generator's forwards and the heat maps of the four batches
    def forwards():
        with torch.no_grad():
            for i in range(0, len(SEEDS), 3):
                z = torch.cat([gw.get_z(n) for n in SEEDS[i:i + 3]])
                gw.rendered_image(gw.sample_image_from_latent(z))
                (gw.context_acts(gw.context_model(z)) * key[None, :, None, None]).sum(dim=1)
    res.update(alternate(dict(forwards_and_heat_maps=forwards), runs, warmup))

    # the kernel alone, one batch of three (a launch of a repaint) and the bytes it moves
    pixels = images.shape[0] * images.shape[2] * images.shape[3]
    moved = dict(bytes_read=12 * pixels + 4 * heat.numel(), bytes_written=3 * pixels)
    for name, kw in (('kernel_heat_thickness_1', dict(activations=heat, level=level, border_color=BORDER)),
                     ('kernel_heat_thickness_8', dict(activations=heat, level=level, border_color=BORDER, thickness=8)),
                     ('kernel_plain_bytes', dict())):
        t = device_time(lambda: hip.render_bytes(images, **kw), runs, warmup)
        res[name] = dict(t, **moved, total_GBps=(moved['bytes_read'] + moved['bytes_written']) / t['median_s'] / 1e9)

    # one launch of a repaint is a few tens of microseconds, mostly the launch itself: the kernel's rate is taken on 48
    # megapixel-sized images' worth of tiles per launch (0.75 GB moved, past the Infinity Cache), ten launches per timing
    copies = max(1, 16 * 1024 * 1024 // (size * size))
    many, many_heat = images.repeat(copies, 1, 1, 1), heat.repeat(copies, 1, 1)
    pixels = many.shape[0] * many.shape[2] * many.shape[3]
    moved = dict(images=many.shape[0], bytes_read=12 * pixels + 4 * many_heat.numel(), bytes_written=3 * pixels)
    for name, kw in (('stream_heat_thickness_1', dict(activations=many_heat, level=level, border_color=BORDER)),
                     ('stream_heat_thickness_8', dict(activations=many_heat, level=level, border_color=BORDER,
                                                      thickness=8)),
                     ('stream_plain_bytes', dict())):
        t = device_time(lambda: [hip.render_bytes(many, **kw) for _ in range(10)], runs, warmup)
        t = {k: v / 10 for k, v in t.items()}
        res[name] = dict(t, **moved, total_GBps=(moved['bytes_read'] + moved['bytes_written']) / t['median_s'] / 1e9)
    scratch = torch.empty_like(many)
    t = device_time(lambda: [scratch.copy_(many) for _ in range(10)], runs, warmup)
    t = {k: v / 10 for k, v in t.items()}
    res['stream_torch_copy'] = dict(t, bytes_read=many.numel() * 4, bytes_written=many.numel() * 4,
                                    total_GBps=2 * many.numel() * 4 / t['median_s'] / 1e9)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_overlay.json'))
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'render_bench.py measures on the GPU; there is nothing to measure without one'
    assert args.runs >= 7
    dev = torch.device('cuda', 0)
    out = dict(device=torch.cuda.get_device_name(dev), runs=args.runs, warmup=args.warmup, models=[])
    for size in (int(v) for v in args.sizes.split(',')):
        out['models'].append(measure(size, args.runs, args.warmup, dev))
        torch.cuda.empty_cache()
        print(json.dumps(out['models'][-1]), flush=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
