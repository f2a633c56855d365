"""Interleaved A/B of builds of the library on the headline forward: one fresh process per run, the arms taking turns,
every run written to OUT.json as it arrives (medians and max - min per arm at the end).

    python scripts/ab_libs.py OUT.json ROUNDS name=path/to/lib.so ... [name=default]

`default` is the in-tree library; any other arm is selected with RW_HIP_LIB (csrc/build.sh with RW_LIB_OUT / RW_OBJ_DIR /
RW_EXTRA_FLAGS builds one).  A run that fails ends the comparison: nothing is started after it."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(out, rounds, arms):
    runs = {n: [] for n, _ in arms}
    ms = {n: [] for n, _ in arms}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for r in range(rounds):
        for name, lib in arms:
            env = dict(os.environ)
            if lib != 'default':
                env['RW_HIP_LIB'] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '3'],
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
            if p.returncode != 0:
                sys.exit('run %d of %s failed (%d): %s' % (r, name, p.returncode, p.stderr.decode()[-800:]))
            d = json.loads(p.stdout.decode().strip().splitlines()[-1])
            runs[name].append(d['value'])
            ms[name].append(d.get('ms_per_step'))
            print(r, name, d['value'], d.get('ms_per_step'), flush=True)
            summary = {n: dict(median=statistics.median(v), max_minus_min=max(v) - min(v)) for n, v in runs.items() if v}
            with open(out, 'w') as f:
                json.dump(dict(command='python bench.py --gpus 1 --steps 20 --warmup 3', unit='images/sec', runs=runs,
                               ms_per_step=ms, summary=summary), f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), [a.split('=', 1) for a in sys.argv[3:]])
