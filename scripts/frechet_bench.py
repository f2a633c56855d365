"""Times the Frechet distance of two synthetic feature sets three ways on one GPU and writes profiles/frechet_distance.json:

  device    samples.frechet_distance on device tensors (rw_frechet.hip), at block widths 8 and 16, end to end
  host      today's host route (scipy.linalg.sqrtm of S1 S2) at the box's thread count
  torch     the same three steps with torch.linalg.eigh on the device -- the plumbing yardstick

F in {512, 2048}; covariances of 1 000 samples (rank-deficient at 2048) and of 50 000.  Every time is a host clock around
work that ends in a copy to the host (a synchronise); each arm is warmed once, then timed --repeat times; the device arm
also times its pieces (first solve, the two products, second solve) with synchronises of their own in a separate pass.

    python scripts/frechet_bench.py [--sizes 512 2048] [--samples 1000 50000] [--repeat 3] [--no-host] [--out PATH]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rewriting_amd import hip, samples  # noqa: E402


def synthetic_sets(f, count, seed):
    """Two (mu, sigma) of `count` samples of f features with a decaying scale and one shared direction."""
    rng = numpy.random.RandomState(seed)
    scale = 1.0 / numpy.sqrt(1.0 + numpy.arange(f))
    out = []
    for shift in (0.0, 0.05):
        x = rng.standard_normal((count, f)).astype(numpy.float64) * scale + 0.1 * rng.standard_normal((count, 1)) + shift
        out.append((x.mean(0), numpy.cov(x, rowvar=False)))
    return out


def clock(fn, repeat):
    fn()                                                    # warm: code objects, allocator
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return value, times


def torch_twin(mu1, s1, mu2, s2):
    lam, v = torch.linalg.eigh(s1)
    f = v * lam.clamp_min(0).sqrt()
    mu = torch.linalg.eigvalsh(f.t() @ s2 @ f)
    return float((mu1 - mu2).square().sum() + s1.trace() + s2.trace() - 2 * mu.clamp_min(0).sqrt().sum())


def pieces(mu1, s1, mu2, s2, block):
    """The device route step by step with a synchronise after each (ms), and its launches."""
    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t)
    n = s1.shape[0]
    npad = hip.jacobi_padded_order(n, block)
    blocks = npad // block
    m = blocks + (blocks & 1)
    g = hip._padded(s1, npad)
    (v, sw1), t1 = timed(lambda: hip._jacobi_solve(g, True, 100, block))
    root = hip.colnorm_f64(g, 2)
    bmat, t2 = timed(lambda: hip.gemm_f64(hip.gemm_f64(v, hip._padded(s2, npad), row_scale=root), v, trans_b=True, col_scale=root))
    (_, sw2), t3 = timed(lambda: hip._jacobi_solve(bmat, False, 100, block))
    # per solve: one norm launch, (m - 1) steps + one slot reduction per sweep; then norms, two products, the final sums
    launches = 2 + (sw1 + sw2) * m + 5
    return dict(first_solve_ms=t1, products_ms=t2, second_solve_ms=t3, sweeps=[sw1, sw2], steps_per_sweep=m - 1,
                workgroups_per_step=m // 2, launches=launches,
                ms_per_step=[t1 / (sw1 * (m - 1)), t3 / (sw2 * (m - 1))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 2048])
    ap.add_argument('--samples', type=int, nargs='+', default=[1000, 50000])
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frechet_distance.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'frechet_bench.py needs the GPU'
    dev = torch.device('cuda', 0)
    doc = dict(device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), repeat=args.repeat,
               default_block=hip.JACOBI_BLOCK, cases=[])
    for f in args.sizes:
        for count in args.samples:
            (mu1, s1), (mu2, s2) = synthetic_sets(f, count, seed=f + count)
            d = [torch.from_numpy(x).to(dev) for x in (mu1, s1, mu2, s2)]
            row = dict(features=f, samples=count, device={})
            for block in (8, 16):
                parts = {}
                value, times = clock(lambda: hip.frechet_distance_f64(*d, max_sweeps=100, block=block, parts=parts), args.repeat)
                row['device']['b%d' % block] = dict(d2=value, seconds=times, median=float(numpy.median(times)),
                                                    pieces=pieces(*d, block))
            value, times = clock(lambda: torch_twin(*d), args.repeat)
            row['torch_eigh_twin'] = dict(d2=value, seconds=times, median=float(numpy.median(times)))
            if not args.no_host:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    t = time.perf_counter()
                    value = float(samples.frechet_distance(mu1, s1, mu2, s2))
                    row['host_sqrtm'] = dict(d2=value, seconds=[time.perf_counter() - t])
                best = min(r['median'] for r in row['device'].values())
                row['host_over_device'] = row['host_sqrtm']['seconds'][0] / best
            row['device_over_torch_twin'] = min(r['median'] for r in row['device'].values()) / row['torch_eigh_twin']['median']
            doc['cases'].append(row)
            print(json.dumps(row), flush=True)
            with open(args.out, 'w') as fh:                 # after every case: a long host step must not lose the rest
                json.dump(doc, fh, indent=1)


if __name__ == '__main__':
    main()
