"""Times the face parser (rewriting_amd/faceparse.py) on one GPU and writes profiles/faceparse_bisenet.json:

  segment   ms per batch of FaceSegmenter.segment_batch at the 512 x 512 working size for batch 1, 8 and 32 of 256 x 256
            images (resize, network, arg-max, labels resized back), random weights; device events around --repeat calls
            after a warm one, the median
  forward   the same for FaceParser.forward at 512 x 512 (the up-sampled scores written instead of the labels)
  families  one more segment_batch per case with a pair of device events around every wrapper call: the share of the kernel
            families (conv2d and conv2d_add with their packing cached, maxpool3x3s2p1, global_avgpool, gate_resample,
            seg_labels).  An event pair also spans the gap to the next launch, so at batch 1 the shares are of launch-bound
            time
  twin      the torch.nn twin of tests/faceparse_checks.py with the same weights on the same box, its arg-max and the two
            F.interpolate around it: MIOpen's convolutions, batch norms unfolded -- the plumbing yardstick

The twin arms run last and the file is rewritten after every measurement: a slow first call of the twin's convolution
library loses nothing.

    python scripts/faceparse_bench.py [--repeat 5] [--no-twin] [--out PATH]
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
from rewriting_amd import faceparse, hip         # noqa: E402
from tests import faceparse_checks as K           # noqa: E402

CASES = (('b1', 1), ('b8', 8), ('b32', 32))
IMAGE = 256
FAMILIES = ('conv2d', 'conv2d_add', 'maxpool3x3s2p1', 'global_avgpool', 'gate_resample', 'seg_labels')


def gflop_per_image(size):
    """2 x the multiply-adds of the 32 convolutions at a size x size input"""
    stem = (size + 6 - 7) // 2 + 1
    s = (stem - 1) // 2 + 1                          # layer1's maps; layer k's are s >> (k - 1)
    total = 0.0
    for op in faceparse.conv_layers(19):
        if op.name == 'cp.resnet.conv1':
            out = stem
        elif op.name.startswith('cp.resnet.'):
            stage = int(op.name.split('layer')[1][0])
            out = s >> (stage - 1)
        elif 'conv_atten' in op.name or op.name in ('cp.conv_avg', 'ffm.conv1', 'ffm.conv2'):
            out = 1
        elif op.name in ('cp.arm32.conv',):
            out = s >> 3
        elif op.name in ('cp.arm16.conv', 'cp.conv_head32'):
            out = s >> 2
        else:
            out = s >> 1
        total += 2.0 * op.in_ch * op.out_ch * op.kernel[0] * op.kernel[1] * out * out
    return total / 1e9


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


def families(fn):
    """ms per wrapper family of one call of fn: device events around every wrapper call."""
    spans = {name: [] for name in FAMILIES}
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
        fn()
        torch.cuda.synchronize()
    finally:
        for name, fn in originals.items():
            setattr(hip, name, fn)
    ms = {name: sum(a.elapsed_time(b) for a, b in pairs) for name, pairs in spans.items()}
    total = sum(ms.values())
    return dict(ms=ms, calls={name: len(pairs) for name, pairs in spans.items()},
                share={name: v / total for name, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'faceparse_bisenet.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'faceparse_bench.py needs the GPU'
    device = torch.device('cuda', 0)
    twin32, sd, _ = K.shared_twin()
    net = faceparse.from_state_dict(sd).to(device)
    seg = faceparse.FaceSegmenter(net)
    gflop = gflop_per_image(faceparse.WORKING_SIZE[0])
    doc = dict(device=torch.cuda.get_device_name(0), repeat=args.repeat, image=IMAGE, working_size=list(faceparse.WORKING_SIZE),
               gflop_per_image=gflop, cases={})

    def dump():
        with open(args.out, 'w') as fh:
            json.dump(doc, fh, indent=1)
    inputs = {name: K.images((batch, 3, IMAGE, IMAGE), batch).to(device) for name, batch in CASES}
    with torch.no_grad():
        for name, batch in CASES:
            x = inputs[name]
            r = event_ms(lambda: seg.segment_batch(x), args.repeat)
            r['tflops'] = gflop * batch / r['median_ms']
            r['families'] = families(lambda: seg.segment_batch(x))
            big = F.interpolate(x, size=faceparse.WORKING_SIZE)
            doc['cases'][name] = dict(batch=batch, segment=r, forward=event_ms(lambda: net(big), args.repeat))
            print(name, json.dumps(doc['cases'][name]), flush=True)
            dump()
        if not args.no_twin:
            twin = twin32.to(device)

            def twin_segment(x):
                scores = twin(F.interpolate(x, size=faceparse.WORKING_SIZE))
                return F.interpolate(scores.argmax(1, keepdim=True).float(), size=x.shape[2:]).long()
            for name, batch in CASES:
                t = time.perf_counter()
                r = event_ms(lambda: twin_segment(inputs[name]), args.repeat)
                r['first_call_and_timing_s'] = time.perf_counter() - t
                case = doc['cases'][name]
                case['torch_twin'] = r
                case['device_over_twin'] = case['segment']['median_ms'] / r['median_ms']
                print(name, 'twin', json.dumps(r), flush=True)
                dump()


if __name__ == '__main__':
    main()
