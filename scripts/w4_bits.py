"""Same bits from two builds of the library on the F(4x4,3x3) kernels: SHA-256 of every output of conv3x3_wino4,
conv_transpose3x3s2_blur_wino4 and conv3x3_wino4_to_rgb over the WINO4_CASES of tests/test_gpu_kernels.py, on fp32 MFMAs
and on the 16-bit pipe, with and without style, with the point split forced off and on (RW_W4H_PS).  One child process per
library (RW_HIP_LIB), run one after the other.

    python scripts/w4_bits.py OUT.json name=path/to/lib.so name=default
"""
import hashlib
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker():
    sys.path.insert(0, ROOT)
    import numpy
    import torch
    from rewriting_amd import hip
    from tests.test_gpu_kernels import WINO4_CASES
    dev = 'cuda'
    out = {}

    def put(name, t):
        torch.cuda.synchronize()
        out[name] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    k1 = torch.tensor([1., 3., 3., 1.])
    k4 = k1[:, None] * k1[None, :]
    k4 = (k4 / k4.sum() * 4).to(dev)
    for case in WINO4_CASES:
        b, i, o, h, w = case
        rs = numpy.random.RandomState(77)
        x = torch.from_numpy(rs.randn(b, i, h, w).astype('float32')).to(dev)
        wt = torch.from_numpy(rs.randn(1, o, i, 3, 3).astype('float32')).to(dev)
        style = torch.from_numpy((1 + 0.5 * rs.randn(b, i)).astype('float32')).to(dev)
        noise = torch.from_numpy(rs.randn(b, h * w).astype('float32')).to(dev)
        bias = torch.from_numpy(rs.randn(o).astype('float32')).to(dev)
        nw = torch.tensor([0.2], device=dev)
        wrgb = torch.from_numpy(rs.randn(3, o).astype('float32')).to(dev)
        srgb = torch.from_numpy((1 + 0.3 * rs.randn(b, o)).astype('float32')).to(dev)
        brgb = torch.from_numpy(rs.randn(3).astype('float32')).to(dev)
        skip = torch.from_numpy(rs.randn(b, 3, h, w).astype('float32')).to(dev)
        s = 1 / math.sqrt(i * 9)
        dm = hip.demod(hip.weight_sqsum(wt, s), style)
        up_ok = hip.conv_transpose_blur_wino4_supported(o, i, h, w) and b * o * h * w <= 2 ** 27
        if up_ok:
            noise_up = torch.from_numpy(rs.randn(b, 1, 2 * h, 2 * w).astype('float32')).to(dev)
        for mm in ('f32', 'split'):
            uf = hip.pack_conv_weight_wino4(wt, split=mm == 'split')
            ufu = hip.pack_conv_transpose_blur_weight_wino4(wt, k4, split=mm == 'split') if up_ok else None
            for ps in (('0', '1') if mm == 'split' else ('-',)):
                if ps != '-':
                    os.environ['RW_W4H_PS'] = ps
                for styled in (True, False):
                    tag = '%s %s ps%s %s' % ('x'.join(map(str, case)), mm, ps, 'style' if styled else 'nostyle')
                    st = dict(style=style, demod=dm) if styled else {}
                    ep = dict(noise=noise, noise_w=nw, bias=bias, act=True)
                    put(tag + ' conv plain', hip.conv3x3_wino4(x, uf, o, s, **st))
                    put(tag + ' conv epilogue', hip.conv3x3_wino4(x, uf, o, s, **st, **ep))
                    if up_ok:
                        put(tag + ' up plain', hip.conv_transpose3x3s2_blur_wino4(x, ufu, o, s, **st))
                        put(tag + ' up epilogue', hip.conv_transpose3x3s2_blur_wino4(
                            x, ufu, o, s, noise=noise_up, noise_w=nw, bias=bias, act=True, **st))
                    if o == 32:
                        put(tag + ' rgb', hip.conv3x3_wino4_to_rgb(x, uf, o, s, wrgb, srgb, brgb, skip, 1 / math.sqrt(o),
                                                                   **st, **ep)[1])
                        put(tag + ' rgb bare', hip.conv3x3_wino4_to_rgb(x, uf, o, s, wrgb, srgb, None, None,
                                                                        1 / math.sqrt(o), **st)[1])
    print(json.dumps(out))


def main(out, arms):
    res = {}
    for name, lib in arms:
        env = dict(os.environ)
        if lib != 'default':
            env['RW_HIP_LIB'] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker'], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=280)
        if p.returncode != 0:
            sys.exit('%s failed (%d): %s' % (name, p.returncode, p.stderr.decode()[-1500:]))
        res[name] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    names = [n for n, _ in arms]
    keys = list(res[names[0]])
    differ = [k for k in keys if any(res[n].get(k) != res[names[0]][k] for n in names[1:])]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(dict(outputs=len(keys), identical=len(keys) - len(differ), differ=differ, sha256=res), f, indent=1)
    print('%d outputs, %d identical across %s' % (len(keys), len(keys) - len(differ), ' / '.join(names)))
    for k in differ:
        print('DIFFERS:', k)
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    if sys.argv[1] == '--worker':
        worker()
    else:
        main(sys.argv[1], [a.split('=', 1) for a in sys.argv[2:]])
