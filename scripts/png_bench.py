"""What the PNG step costs (GPU only, one process): the twelve result tiles of a repaint as data URLs, and a sample set
written to files, on the device route (hip.render_bytes + hip.png_encode: pngwriter, gw.render_urls) and on the route
before it (PIL's img.save on the host, one picture at a time or in a 16-thread pool).

    python scripts/png_bench.py [--out profiles/png_encode.json] [--sizes 256,1024] [--images 1000]

Twelve tiles, at layer 8 of the 256^2 and of the 1024^2 generator:
  tiles_*      from twelve float images that are resident on the device to twelve data URLs: pngwriter.as_urls against
               hip.render_bytes + one copy + renormalize.as_url per tile (what device_render=True leaves for the host);
  repaint_*    the whole call, forwards and heat maps included: gw.render_urls against render_image_batch + as_url;
  stages_ms    hip.png_encode's stages by HIP events (filter / host tables / encode / compaction / copy), and the sizes.
Files: --images seeds of the 1024^2 generator through pngwriter.save_image_set against samples.generate +
renormalize.as_image(...).save in a pool of 16 threads: images per second and the bytes each route wrote.
The routes alternate in one process; every figure is the median of --runs (>= 7) runs after --warmup runs, a clock around
a synchronise (both routes end on the host).  There is no fallback: without a GPU the script fails.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                            # noqa: E402
from rewriting_amd import hip, pngwriter, samples       # noqa: E402
from rewriting_amd.rewrite import ganrewrite            # noqa: E402
from rewriting_amd.utils import renormalize, zdataset   # noqa: E402

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


def tiles(size, runs, warmup, dev):
    res = dict(size=size, layer=LAYER, tiles=len(SEEDS))
    g = bench.build_generator(size, dev)
    zds = zdataset.z_dataset_for_model(g, size=max(SEEDS) + 1)
    gw = ganrewrite.SeqStyleGanRewriter(g, zds, LAYER, device_render=True)
    torch.manual_seed(0)
    key = torch.randn(gw.k_shape[1], device=dev)
    key = key / key.norm()
    with torch.no_grad():
        images, heats = [], []
        for i in range(0, len(SEEDS), 3):
            zb = torch.cat([gw.get_z(n) for n in SEEDS[i:i + 3]])
            images.append(gw.rendered_image(gw.sample_image_from_latent(zb)))
            heats.append((gw.context_acts(gw.context_model(zb)) * key[None, :, None, None]).sum(dim=1))
        images, heat = torch.cat(images).contiguous(), torch.cat(heats).contiguous()
    level = heat.reshape(-1).sort()[0][int(heat.numel() * 0.97)].item()
    overlay = dict(activations=heat, level=level, border_color=BORDER)

    def host_urls():
        return [renormalize.as_url(p) for p in gw._as_images(hip.render_bytes(images, **overlay))]
    res.update(alternate(dict(tiles_device_route=lambda: pngwriter.as_urls(images, **overlay),
                              tiles_host_png_route=host_urls), runs, warmup))
    res['tiles_host_over_device'] = res['tiles_host_png_route']['median_s'] / res['tiles_device_route']['median_s']
    res.update(alternate(dict(
        repaint_device_route=lambda: gw.render_urls(SEEDS, key, level, border_color=BORDER),
        repaint_host_png_route=lambda: [renormalize.as_url(p)
                                        for p in gw.render_image_batch(SEEDS, key, level, border_color=BORDER)]),
        runs, warmup))
    res['repaint_host_over_device'] = (res['repaint_host_png_route']['median_s']
                                       / res['repaint_device_route']['median_s'])

    tile_bytes = hip.render_bytes(images, **overlay)
    stages = {}
    for i in range(warmup + runs):
        t = {}
        hip.png_encode(tile_bytes, timings=t)
        if i >= warmup:
            for k, v in t.items():
                stages.setdefault(k, []).append(v)
    res['stages_ms'] = {k: statistics.median(v) for k, v in stages.items()}
    res['bytes_device_route'] = sum(len(f) for f in hip.png_encode(tile_bytes))
    res['bytes_host_png_route'] = sum(len(u) for u in host_urls()) * 3 // 4      # base64 back to bytes, near enough
    res['bytes_raw'] = tile_bytes.numel()
    return res


def files(count, batch, runs, warmup, dev):
    g = bench.build_generator(1024, dev)
    res = dict(size=1024, images=count, batch=batch, host_pool_threads=16)
    root = tempfile.mkdtemp(prefix='png_bench_')

    def device_route():
        pngwriter.save_image_set(g, g, range(count), os.path.join(root, 'device'), batch=batch, shard=None)

    def save(img, path):
        renormalize.as_image(img).save(path)

    def host_route():
        os.makedirs(os.path.join(root, 'host'), exist_ok=True)
        with ThreadPoolExecutor(max_workers=16) as pool:
            jobs = []
            for chunk, images in samples.generate(g, g, range(count), batch=batch, shard=None):
                images = images.cpu()                    # one copy per batch; the pool converts and saves
                jobs += [pool.submit(save, img, os.path.join(root, 'host', 'image_%d.png' % s))
                         for s, img in zip(chunk, images)]
            for job in jobs:
                job.result()
    try:
        res.update(alternate(dict(files_device_route=device_route, files_host_pool_route=host_route), runs, warmup))
        for name in ('device', 'host'):
            folder = os.path.join(root, name)
            res['bytes_written_%s' % name] = sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    for name in ('files_device_route', 'files_host_pool_route'):
        res[name]['images_per_s'] = count / res[name]['median_s']

    def generate_only():
        for _ in samples.generate(g, g, range(count), batch=batch, shard=None):
            pass
    res.update(alternate(dict(generate_only=generate_only), runs, warmup))
    res['generate_only']['images_per_s'] = count / res['generate_only']['median_s']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_encode.json'))
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--images', type=int, default=1000, help='files of the sample set (0: skip that part)')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'png_bench.py measures on the GPU; there is nothing to measure without one'
    assert args.runs >= 7
    dev = torch.device('cuda', 0)
    out = dict(device=torch.cuda.get_device_name(dev), runs=args.runs, warmup=args.warmup,
               segment_bytes=hip.png_segment_bytes(), tiles=[], files=None)

    def keep(result):
        print(json.dumps(result), flush=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    for size in (int(v) for v in args.sizes.split(',')):
        out['tiles'].append(tiles(size, args.runs, args.warmup, dev))
        torch.cuda.empty_cache()
        keep(out['tiles'][-1])
    if args.images:
        out['files'] = files(args.images, args.batch, args.runs, args.warmup, dev)
        keep(out['files'])
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
