"""Times the Inception-v3 pool3 feature extractor (rewriting_amd/inception.py) on one GPU and writes
profiles/inception_fid.json:

  forward   ms per batch of FIDInception at 299 x 299 for batch 1, 8 and 50, and from a 1024 x 1024 input (batch 8, resized
            on the device), random weights; device events around --repeat forwards after a warm one, the median
  twin      the torch.nn twin of tests/inception_checks.py with the same weights on the same box (F.interpolate in front of
            it for the 1024 x 1024 input): MIOpen's convolutions, batch norms unfolded -- the plumbing yardstick
  families  one more forward per case with a pair of device events around every wrapper call: the share of the four kernel
            families (conv2d with its packing cached, pool3x3, global_avgpool, inception_input).  An event pair also spans
            the gap to the next launch, so at batch 1 the shares are of launch-bound time
  row       generate -> features -> statistics -> distance for two sets of --row-images images of the 256 x 256 model
            (samples.generate, FIDInception, samples.activation_statistics, samples.fid), host clock, synchronised

The twin arms run last and the file is rewritten after every measurement: a slow first call of the twin's convolution
library loses nothing.

    python scripts/inception_bench.py [--repeat 5] [--row-images 1000] [--no-twin] [--row-only] [--out PATH]
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
from rewriting_amd import hip, inception, samples, workloads  # noqa: E402
from tests import inception_checks as K                         # noqa: E402

CASES = (('b1_299', 1, 299), ('b8_299', 8, 299), ('b50_299', 50, 299), ('b8_1024', 8, 1024))
GFLOP_PER_IMAGE = 11.4          # 2 x 5.7 G multiply-adds of the 94 convolutions at 299 x 299


def event_ms(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(ms=times, median_ms=statistics.median(times))


def families(net, x):
    """ms per wrapper family of one forward: device events around every call."""
    spans = {name: [] for name in ('conv2d', 'pool3x3', 'global_avgpool', 'inception_input')}
    originals = {name: getattr(hip, name) for name in spans}

    def wrap(name):
        def call(*args, **kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = originals[name](*args, **kw)
            b.record()
            spans[name].append((a, b))
            return out
        return call
    try:
        for name in spans:
            setattr(hip, name, wrap(name))
        net(x)
        torch.cuda.synchronize()
    finally:
        for name, fn in originals.items():
            setattr(hip, name, fn)
    ms = {name: sum(a.elapsed_time(b) for a, b in pairs) for name, pairs in spans.items()}
    total = sum(ms.values())
    return dict(ms=ms, calls={name: len(pairs) for name, pairs in spans.items()},
                share={name: v / total for name, v in ms.items()})


def row(net, device, images, batch=50):
    """The FID row for two sets of `images` images of the 256 x 256 model (seeds offset by 0 and 10 000)."""
    model = workloads.build_model(256, 0.5, device)
    out = {}

    def clock(name, fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        out[name] = time.perf_counter() - t
        return value
    # warm both networks
    list(samples.generate(model, model, range(batch), batch=batch, device=device, shard=None))
    net(torch.zeros(batch, 3, 256, 256, device=device))
    clock('generate_only_s', lambda: [im for _, im in samples.generate(model, model, range(images), batch=batch, device=device)])
    sets = [clock('generate_features_statistics_s_set%d' % i,
                  lambda: samples.activation_statistics(
                      samples.generate(model, model, range(images), batch=batch, offset=offset, device=device), net))
            for i, offset in enumerate((0, 10000))]
    out['images_per_set'], out['batch'] = images, batch
    out['trace'] = [float(s.mean_cov(device=True)[1].diagonal().sum()) for s in sets]
    try:
        out['fid'] = clock('distance_s', lambda: samples.fid(*sets))
    except RuntimeError as e:       # the Jacobi solver's sweep limit: reported, then once more with a higher one
        out['distance_error'] = str(e)
        (mu_a, s_a), (mu_b, s_b) = (s.mean_cov(device=True) for s in sets)
        parts = {}
        try:
            out['fid'] = clock('distance_s', lambda: hip.frechet_distance_f64(mu_a, s_a, mu_b, s_b, max_sweeps=200, parts=parts))
            out['distance_max_sweeps'], out['distance_sweeps'] = 200, parts.get('sweeps')
        except RuntimeError as e2:
            out['distance_error_200_sweeps'] = str(e2)
        # the same sets through the fp32 block of FeatureStatistics' default route: noise of 2^-24 |f|^2 in every eigenvalue
        blocks = []
        for offset in (0, 10000):
            st = samples.FeatureStatistics()
            with torch.no_grad():
                for _, im in samples.generate(model, model, range(images), batch=batch, offset=offset, device=device):
                    st.add(net(im))
            blocks.append(st)
        parts = {}
        (mu_a, s_a), (mu_b, s_b) = (s.mean_cov(device=True) for s in blocks)
        try:
            out['fid_fp32_block_statistics'] = clock(
                'distance_fp32_block_statistics_s', lambda: hip.frechet_distance_f64(mu_a, s_a, mu_b, s_b, parts=parts))
            out['distance_fp32_block_statistics_sweeps'] = parts.get('sweeps')
        except RuntimeError as e3:
            out['distance_error_fp32_block_statistics'] = str(e3)
    if 'distance_s' in out:
        out['row_s'] = (out['generate_features_statistics_s_set0'] + out['generate_features_statistics_s_set1']
                        + out['distance_s'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--row-images', type=int, default=1000)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--row-only', action='store_true', help='measure the row alone and replace it in the file --out names')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'inception_fid.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'inception_bench.py needs the GPU'
    device = torch.device('cuda', 0)
    twin32, sd, _ = K.shared_twin()
    net = inception.from_state_dict(sd).to(device)
    doc = dict(device=torch.cuda.get_device_name(0), repeat=args.repeat, gflop_per_image=GFLOP_PER_IMAGE, cases={})

    def dump():
        with open(args.out, 'w') as fh:
            json.dump(doc, fh, indent=1)
    if args.row_only:
        if os.path.isfile(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        with torch.no_grad():
            doc['row'] = row(net, device, args.row_images)
        print('row', json.dumps(doc['row']), flush=True)
        dump()
        return
    inputs = {name: K.images((batch, 3, size, size), batch + size).to(device) for name, batch, size in CASES}
    with torch.no_grad():
        for name, batch, size in CASES:
            r = event_ms(lambda: net(inputs[name]), args.repeat)
            r['tflops'] = GFLOP_PER_IMAGE * batch / r['median_ms']
            r['families'] = families(net, inputs[name])
            doc['cases'][name] = dict(batch=batch, input=size, device=r)
            print(name, json.dumps(r), flush=True)
            dump()
        doc['row'] = row(net, device, args.row_images)
        print('row', json.dumps(doc['row']), flush=True)
        dump()
        if not args.no_twin:
            twin = twin32.to(device)

            def twin_forward(x):
                if x.shape[2] != 299:
                    x = F.interpolate(x.clamp(-1, 1), size=(299, 299), mode='bilinear', align_corners=False)
                return twin(x)
            for name, batch, size in CASES:
                t = time.perf_counter()
                r = event_ms(lambda: twin_forward(inputs[name]), args.repeat)
                r['first_call_and_timing_s'] = time.perf_counter() - t
                case = doc['cases'][name]
                case['torch_twin'] = r
                case['device_over_twin'] = case['device']['median_ms'] / r['median_ms']
                print(name, 'twin', json.dumps(r), flush=True)
                dump()


if __name__ == '__main__':
    main()
