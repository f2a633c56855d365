"""Do two builds of the library give the generator's glue ops the same bits?

    python scripts/glue_twins_bits.py OUT.json name=path/to/lib.so name=default

The glue ops that are one kernel body for float and double (csrc/rw_ops.hip: pixel_norm, adjust_latent, style_mul,
noise_add, weight_sqsum, demod, to_rgb) and equal_linear run in both dtypes on the shapes of tests/test_gpu_glue_twins.py
(every branch of the shared bodies and the fp32-only branches beside them), on seeded inputs, once per library: each
library in a fresh child process under a time limit of its own (`default` is the in-tree library, any other is selected
with RW_HIP_LIB; csrc/build.sh with RW_LIB_OUT / RW_OBJ_DIR builds one from another checkout).  The outputs are compared
byte for byte with the first library's.  A child that fails ends the run: nothing is started after it.  Exit status 1
if any output differs."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 180


def cases():
    """[(name, output as a CPU tensor)] for the library this process loaded"""
    import torch
    sys.path.insert(0, ROOT)
    from rewriting_amd import hip
    gen = torch.Generator().manual_seed(2024)
    out = []

    def rand(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    def both(name, f32, f64, *args):
        """args: float64 CPU tensors, None or python scalars; the fp32 entry takes the tensors rounded once"""
        for dtype, fn in ((torch.float32, f32), (torch.float64, f64)):
            a = [t.to(dtype).cuda() if isinstance(t, torch.Tensor) else t for t in args]
            out.append(('%s %s' % (name, str(dtype).split('.')[1]), fn(*a).cpu()))

    for shape in ((3, 70), (5, 512)):
        both('pixel_norm %s' % (shape,), hip.pixel_norm, hip.pixel_norm_f64, rand(*shape), 1e-8)
    w, avg = rand(3, 70), rand(70)
    both('adjust_latent avg', hip.adjust_latent, hip.adjust_latent_f64, w, avg, 6, 0.7)
    both('adjust_latent no avg', hip.adjust_latent, hip.adjust_latent_f64, w, None, 6, 0.7)
    for b, c, h, wd in ((2, 5, 3, 5), (2, 5, 4, 4)):
        x = rand(b, c, h, wd)
        both('style_mul %s' % ((b, c, h, wd),), hip.style_mul, hip.style_mul_f64, x, rand(b, c))
        both('noise_add %s' % ((b, c, h, wd),), hip.noise_add, hip.noise_add_f64, x, rand(b, 1, h, wd), rand(1))
    both('weight_sqsum (40, 24, 3, 3)', hip.weight_sqsum, hip.weight_sqsum_f64, rand(40, 24, 3, 3), 1.0 / (24 * 9) ** 0.5)
    for b, i, o in ((2, 24, 40), (3, 64, 48)):
        both('demod %d x %d -> %d' % (b, i, o), hip.demod, hip.demod_f64, rand(o, i).square(), rand(b, i), 1e-8)
    x, wt, s = rand(2, 24, 5, 7), rand(3, 24), rand(2, 24)
    both('to_rgb bias skip', hip.to_rgb, hip.to_rgb_f64, x, wt, s, rand(3), rand(2, 3, 5, 7), 1.0 / 24 ** 0.5)
    both('to_rgb plain', hip.to_rgb, hip.to_rgb_f64, x, wt, s, None, None, 1.0 / 24 ** 0.5)
    for b, i, o in ((3, 70, 40), (5, 64, 48)):
        both('equal_linear %d x %d -> %d' % (b, i, o), hip.equal_linear, hip.equal_linear_f64, rand(b, i), rand(o, i),
             rand(o), 1.0 / i ** 0.5, 0.01, True)
    return out


def child(path):
    import numpy
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    numpy.savez(path, **{name: numpy.frombuffer(t.contiguous().numpy().tobytes(), dtype=numpy.uint8) for name, t in cases()})


def main(out, arms):
    import numpy
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, lib in arms:
            env = dict(os.environ)
            env.pop('RW_HIP_LIB', None)
            if lib != 'default':
                env['RW_HIP_LIB'] = os.path.abspath(lib)
            path = os.path.join(tmp, name + '.npz')
            p = subprocess.run(['timeout', '-k', '10', str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), '--child', path],
                               env=env)
            if p.returncode != 0:
                sys.exit('the run of %s failed (%d): nothing more is started' % (name, p.returncode))
            with numpy.load(path) as z:
                results[name] = {k: z[k].tobytes() for k in z.files}
    first = arms[0][0]
    rows, differing = [], 0
    for case, ref in results[first].items():
        row = dict(case=case, bytes=len(ref), sha256={first: hashlib.sha256(ref).hexdigest()}, equal=True)
        for name, _ in arms[1:]:
            got = results[name].get(case)
            row['sha256'][name] = hashlib.sha256(got).hexdigest() if got is not None else None
            row['equal'] = row['equal'] and got == ref
        differing += not row['equal']
        rows.append(row)
        print('%-8s %s' % ('equal' if row['equal'] else 'DIFFERS', case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(dict(command='python scripts/glue_twins_bits.py OUT.json ' + ' '.join('%s=%s' % (n, l) for n, l in arms),
                       libraries=[n for n, _ in arms], cases=len(rows), differing=differing, rows=rows), f, indent=1)
    print('%d cases, %d differ' % (len(rows), differing))
    return 1 if differing else 0


if __name__ == '__main__':
    if sys.argv[1] == '--child':
        child(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1], [a.split('=', 1) for a in sys.argv[2:]]))
