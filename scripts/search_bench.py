"""What a Search costs (GPU only, one process): ranking_for_key as the torch expression (device_search=False), search()
without and with the resident key-map index, the index build, and the key-response kernel's byte rate beside a torch
device-to-device copy timed in the same process.

    python scripts/search_bench.py [--out profiles/search_key_response.json] [--models 256:1000,1024:10000]

Layer 8 of the 256^2 generator with 1000 seeds and of the 1024^2 generator with 10 000 seeds (the 21 GB index; skipped
with a note if the device has not twice that free).  Every figure is the median of --runs (>= 7) runs after --warmup
runs; device work is timed with HIP events, whole queries (which end on the host) with a clock around a synchronise.
Byte counts come from the shapes: the kernel reads the key maps once and writes K / C of that; a copy reads and writes
its bytes.
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


def wall(fn, runs, warmup):
    """Median seconds of fn(), synchronised at both ends."""
    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def device_time(fn, runs, warmup):
    """Median seconds of the device work fn() enqueues, by HIP events."""
    times = []
    for i in range(warmup + runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= warmup:
            times.append(start.elapsed_time(stop) * 1e-3)
    return statistics.median(times), min(times), max(times)


def spread(t):
    return dict(median_s=t[0], min_s=t[1], max_s=t[2])


def measure(size, nseeds, runs, warmup, dev):
    res = dict(size=size, layer=LAYER, seeds=nseeds)
    g = bench.build_generator(size, dev)
    zds = zdataset.z_dataset_for_model(g, size=nseeds)
    gw = ganrewrite.SeqStyleGanRewriter(g, zds, LAYER)
    res['key_map_shape'] = list(gw.k_shape)
    res['launch_seeds'] = gw._sweep_batch()
    torch.manual_seed(0)
    keys = torch.randn(8, gw.k_shape[1], device=dev)
    keys = keys / keys.norm(dim=1, keepdim=True)

    res['ranking_for_key_torch'] = spread(wall(lambda: gw.ranking_for_key(keys[0], k=12), runs, warmup))
    res['search_unindexed_1key'] = spread(wall(lambda: gw.search(keys[0], k=12), runs, warmup))
    res['search_unindexed_8keys'] = spread(wall(lambda: gw.search(keys, k=12), runs, warmup))

    need = 4 * nseeds * gw.k_shape[1] * gw.k_shape[2] * gw.k_shape[3]
    free = torch.cuda.mem_get_info(dev)[0]
    res['index_bytes'] = need
    if free < 2 * need:
        res['index'] = 'skipped: %d bytes free on the device, the index needs %d' % (free, need)
        return res
    res['index_build'] = spread(wall(lambda: gw.build_search_index(), 3, 1))
    index = gw.search_index
    res['search_indexed_1key'] = spread(wall(lambda: gw.search(keys[0], k=12), runs, warmup))
    res['search_indexed_8keys'] = spread(wall(lambda: gw.search(keys, k=12), runs, warmup))
    assert gw.search_index is index

    # the split of an indexed query: the kernel's passes alone, and the statistics (RunningTopK.add and
    # RunningQuantile.add / compress_ -- the device sort of N * H * W values per key) on heat maps already computed
    pieces = list(index.pieces())
    for nk in (1, 8):
        kk = keys[:nk].contiguous()
        t = device_time(lambda: [hip.key_response(p, kk) for p in pieces], runs, warmup)
        read, written = need, need // gw.k_shape[1] * nk
        res['kernel_%dkeys_by_launch' % nk] = dict(spread(t), bytes_read=read, bytes_written=written,
                                                   read_GBps=read / t[0] / 1e9, total_GBps=(read + written) / t[0] / 1e9)
        t = device_time(lambda: hip.key_response(index.maps, kk), runs, warmup)
        res['kernel_%dkeys_one_launch' % nk] = dict(spread(t), bytes_read=read, bytes_written=written,
                                                    read_GBps=read / t[0] / 1e9, total_GBps=(read + written) / t[0] / 1e9)
        t = device_time(lambda: hip.key_response(index.maps, kk, want_peak=False), runs, warmup)
        res['kernel_%dkeys_one_launch_no_peak' % nk] = dict(spread(t), read_GBps=read / t[0] / 1e9)

        def statistics_only(heats):
            from rewriting_amd.utils import runningstats
            rtk, rq = runningstats.RunningTopK(k=12), runningstats.RunningQuantile()
            for heat, peak in heats:
                rtk.add(peak)
                rq.add(heat.permute(1, 0, 2, 3).reshape(heat.shape[1], -1).t())
            rtk.to_('cpu')
            rq.compress_()
            rq.to_('cpu')
        heats = [hip.key_response(p, kk) for p in pieces]
        res['statistics_%dkeys' % nk] = spread(wall(lambda: statistics_only(heats), runs, warmup))
        del heats

    # a device-to-device copy of the same bytes, piece by piece into one buffer (reads and writes them once each)
    scratch = torch.empty_like(pieces[0])
    t = device_time(lambda: [scratch[:p.shape[0]].copy_(p) for p in pieces], runs, warmup)
    res['torch_copy'] = dict(spread(t), bytes_read=need, bytes_written=need, read_GBps=need / t[0] / 1e9,
                             total_GBps=2 * need / t[0] / 1e9)
    res['kernel_read_rate_over_copy_read_rate'] = res['kernel_8keys_by_launch']['read_GBps'] / res['torch_copy']['read_GBps']
    res['kernel_read_rate_over_copy_total_rate'] = res['kernel_8keys_by_launch']['read_GBps'] / res['torch_copy']['total_GBps']
    gw.drop_search_index()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'search_key_response.json'))
    ap.add_argument('--models', default='256:1000,1024:10000')
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'search_bench.py measures on the GPU; there is nothing to measure without one'
    assert args.runs >= 7
    dev = torch.device('cuda', 0)
    out = dict(device=torch.cuda.get_device_name(dev), runs=args.runs, warmup=args.warmup, models=[])
    for spec in args.models.split(','):
        size, nseeds = (int(v) for v in spec.split(':'))
        out['models'].append(measure(size, nseeds, args.runs, args.warmup, dev))
        torch.cuda.empty_cache()
        print(json.dumps(out['models'][-1]), flush=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
