"""What tiles at the UI's size cost (GPU only, one process): the twelve result tiles of a repaint of the 1024^2 generator
at layer 8 as 256^2 data URLs, by three routes, and the two passes of rw_resize_bilinear_u8 alone.

    python scripts/resize_bench.py [--out profiles/resize_bilinear.json] [--size 1024] [--tile 256]

  repaint_host_route         render_image_batch + renormalize.as_url(size=...): one copy of the full-size bytes, then a PIL
                             resize and a PIL save per tile, on the host;
  repaint_device_full_size   gw.render_urls(...): full-size PNGs coded on the device, the one device route before
                             hip.resize_bytes (the browser scales them, with its own filter);
  repaint_device_resized     gw.render_urls(..., size=(tile, tile)): hip.render_bytes, hip.resize_bytes, hip.png_encode.
The routes alternate in one process; every figure is the median of --runs (>= 7) runs after --warmup runs, a clock around
a synchronise (every route ends on the host).  url_bytes_*: the characters of the twelve URLs.
kernel: rw_resize_bilinear_u8 on twelve pictures by HIP events (twenty launches between two events, buffers allocated
once), --size -> --tile and --tile -> --size, x only / y only / both, in bytes read + written per second (what the passes
must move: each pass reads its source once and writes its result once), beside a torch device-to-device copy of the
same byte count.  There is no fallback: without a GPU the script
fails.
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


def repaint(size, tile, runs, warmup, dev):
    res = dict(size=size, tile=tile, layer=LAYER, tiles=len(SEEDS))
    g = bench.build_generator(size, dev)
    zds = zdataset.z_dataset_for_model(g, size=max(SEEDS) + 1)
    gw = ganrewrite.SeqStyleGanRewriter(g, zds, LAYER, device_render=True)
    torch.manual_seed(0)
    key = torch.randn(gw.k_shape[1], device=dev)
    key = key / key.norm()
    with torch.no_grad():
        heat = torch.cat([gw._heat(torch.cat([gw.get_z(n) for n in SEEDS[i:i + 3]]), key, 0.0)
                          for i in range(0, len(SEEDS), 3)])
    level = heat.reshape(-1).sort()[0][int(heat.numel() * 0.97)].item()
    shape = (tile, tile)

    def host_route():
        return [renormalize.as_url(p, size=shape) for p in gw.render_image_batch(SEEDS, key, level, border_color=BORDER)]

    def device_full_size():
        return gw.render_urls(SEEDS, key, level, border_color=BORDER)

    def device_resized():
        return gw.render_urls(SEEDS, key, level, size=shape, border_color=BORDER)

    def forwards_only():
        gw._picture_batches(SEEDS, key, level, border_color=BORDER)
    res.update(alternate(dict(repaint_host_route=host_route, repaint_device_full_size=device_full_size,
                              repaint_device_resized=device_resized, forwards_and_bytes_only=forwards_only), runs, warmup))
    res['url_bytes_device_full_size'] = sum(len(u) for u in device_full_size())
    res['url_bytes_device_resized'] = sum(len(u) for u in device_resized())
    res['url_bytes_host_route'] = sum(len(u) for u in host_route())
    res['resized_costs_less_than_full_size'] = (res['repaint_device_resized']['median_s']
                                                < res['repaint_device_full_size']['median_s'])
    return res


REPS = 20             # launches between two events: one launch is tens of microseconds


def events_ms(fn, runs, warmup):
    """milliseconds per call of fn, REPS calls between two HIP events"""
    times = []
    for i in range(warmup + runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(REPS):
            fn()
        stop.record()
        stop.synchronize()
        if i >= warmup:
            times.append(start.elapsed_time(stop) / REPS)
    return statistics.median(times)


def entry_call(src, size):
    """hip.resize_bytes(src, size) as a closure over buffers allocated once: the entry alone, no allocation per call"""
    from rewriting_amd import resample
    b, h, w, _ = src.shape
    ow, oh = size
    kx, bx = resample.device_coefficients(w, ow, src.device) if ow != w else (None, None)
    ky, by = resample.device_coefficients(h, oh, src.device) if oh != h else (None, None)
    scratch = torch.empty(b, h, ow, 3, dtype=torch.uint8, device=src.device) if kx is not None and ky is not None else None
    out = torch.empty(b, oh, ow, 3, dtype=torch.uint8, device=src.device)
    entry, p = hip.lib().rw_resize_bilinear_u8, hip._p
    args = (p(src), p(kx), p(bx), p(ky), p(by), p(scratch), p(out), b, h, w, oh, ow,
            0 if kx is None else kx.shape[1], 0 if ky is None else ky.shape[1], hip._stream())

    def call():
        hip.check(entry(*args))
    call()
    assert torch.equal(out, hip.resize_bytes(src, size))
    return call, out


def passes(n, m, runs, warmup, dev):
    """rw_resize_bilinear_u8 on twelve n x n pictures: along x only (n x n -> n x m), along y only (n x m -> m x m: what
    the y pass of the square resize reads), and both.  bytes_moved: every pass reads its source once and writes its
    result once."""
    images = len(SEEDS)
    torch.manual_seed(1)
    full = torch.randint(0, 256, (images, n, n, 3), dtype=torch.uint8, device=dev)
    half = hip.resize_bytes(full, (m, n))                  # (images, n, m, 3)
    res = dict(images=images, source=n, result=m, launches_per_event_pair=REPS, passes={})
    for name, src, size in (('x', full, (m, n)), ('y', half, (m, m)), ('both', full, (m, m))):
        call, out = entry_call(src, size)
        moved = src.numel() + out.numel()
        if name == 'both':
            moved = full.numel() + 2 * half.numel() + out.numel()
        ms = events_ms(call, runs, warmup)
        a, b = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_ms = events_ms(lambda: b.copy_(a), runs, warmup)      # reads moved / 2, writes moved / 2
        res['passes'][name] = dict(ms=ms, bytes_moved=moved, gb_per_s=moved / ms / 1e6, copy_same_bytes_ms=copy_ms,
                                   copy_gb_per_s=2 * (moved // 2) / copy_ms / 1e6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resize_bilinear.json'))
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'resize_bench.py measures on the GPU; there is nothing to measure without one'
    assert args.runs >= 7
    dev = torch.device('cuda', 0)
    out = dict(device=torch.cuda.get_device_name(dev), runs=args.runs, warmup=args.warmup)
    out['repaint'] = repaint(args.size, args.tile, args.runs, args.warmup, dev)
    print(json.dumps(out['repaint']), flush=True)
    torch.cuda.empty_cache()
    out['kernel'] = [passes(args.size, args.tile, args.runs, args.warmup, dev),
                     passes(args.tile, args.size, args.runs, args.warmup, dev)]
    print(json.dumps(out['kernel']), flush=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
