"""Times the half, fp32 and double forms of two L1 ops on one GPU, in one process and alternated:

  fused_leaky_relu forward on a 64 x 512 x 64 x 64 map (the op layer: rw_fused_bias_act_*, 16-byte vector path);
  upfirdn2d up 2 with the generator's 4 x 4 kernel on a 64 x 3 x 512 x 512 image (the skip upsampling of the RGB image:
  upfirdn2d_up2k4_kernel).

Device events around --reps back-to-back calls after --warmup calls of every case; --rounds rounds, each running every
(op, dtype) in turn, so that a slow stretch of the box lands on all three dtypes.  Bytes are the algorithmic ones (each
input read once, each output written once), the bandwidth bar the ~6.3 TB/s a float4 copy reaches (MI355X_MICROARCH.md).

    python scripts/l1_dtype_timing.py --out profiles/<name>.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TB_S = 6.3
DTYPES = [('f16', torch.float16), ('f32', torch.float32), ('f64', torch.float64)]


def cases(dev):
    from rewriting_amd.utils.stylegan2 import op
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(64, 512, 64, 64, device=dev, generator=gen)
    b = torch.randn(512, device=dev, generator=gen)
    img = torch.randn(64, 3, 512, 512, device=dev, generator=gen)
    k = torch.tensor([1., 3., 3., 1.], device=dev)
    k = k[None, :] * k[:, None] / 16 * 4
    out = {}
    for name, dt in DTYPES:
        xd, bd, imgd, kd = x.to(dt), b.to(dt), img.to(dt), k.to(dt)
        size = torch.tensor([], dtype=dt).element_size()
        out[('fused_leaky_relu_64x512x64x64', name)] = (
            lambda xd=xd, bd=bd: op.fused_leaky_relu(xd, bd), (2 * xd.numel() + bd.numel()) * size)
        out[('upfirdn2d_up2_k4_64x3x512x512', name)] = (
            lambda imgd=imgd, kd=kd: op.upfirdn2d(imgd, kd, up=2, pad=(2, 1)), (5 * imgd.numel() + kd.numel()) * size)
    return out


def time_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='write the JSON here as well as to stdout')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the GPU kernels: it needs the MI355X'
    dev = torch.device('cuda', 0)
    with torch.no_grad():
        work = cases(dev)
        for fn, _ in work.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        samples = {key: [] for key in work}
        for _ in range(args.rounds):
            for key, (fn, _) in work.items():
                samples[key].append(time_ms(fn, args.reps))
    result = {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__, 'reps': args.reps,
              'rounds': args.rounds, 'warmup': args.warmup, 'hbm_tb_s_bar': HBM_TB_S, 'ops': {}}
    for (op_name, dt), ms in samples.items():
        med = statistics.median(ms)
        nbytes = work[(op_name, dt)][1]
        result['ops'].setdefault(op_name, {})[dt] = {
            'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'bytes': nbytes,
            'tb_per_s': round(nbytes / med / 1e9, 3), 'frac_of_hbm_bar': round(nbytes / med / 1e9 / HBM_TB_S, 3)}
    for op_name, per in result['ops'].items():
        per['f16_over_f32'] = round(per['f16']['ms_median'] / per['f32']['ms_median'], 3)
        per['f64_over_f32'] = round(per['f64']['ms_median'] / per['f32']['ms_median'], 3)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
