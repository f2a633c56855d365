"""Interleaved A/B of switch settings -- and of whole checkouts -- on the headline forward: one fresh process per run, the
arms taking turns, every run written to OUT.json as it arrives (medians and max - min per arm at the end).

    python scripts/ab_env.py OUT.json ROUNDS name[@TREE[#N]]:[ENV=VAL,ENV=VAL...] ...

An arm runs `bench.py --gpus 1 --steps 20 --warmup 3` of TREE (default: this checkout; a built checkout of another commit,
e.g. the parent's, shows that "switch off" is that commit) with its settings added to the environment; `#N` runs the arm in
the first N rounds only.  A run that fails ends the comparison: nothing is started after it.

    python scripts/ab_env.py profiles/x_ab.json 6 parent@../parent#2: off:RW_RGB_INLINE_UP=0 on:
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMAND = ['bench.py', '--gpus', '1', '--steps', '20', '--warmup', '3']


def parse(arm):
    head, _, envs = arm.partition(':')
    name, _, tree = head.partition('@')
    tree, _, n = tree.partition('#')
    return dict(name=name, tree=os.path.abspath(tree) if tree else ROOT, rounds=int(n) if n else None,
                env=dict(kv.split('=', 1) for kv in envs.split(',') if kv))


def main(out, rounds, arms):
    runs = {a['name']: [] for a in arms}
    ms = {a['name']: [] for a in arms}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for r in range(rounds):
        for a in arms:
            if a['rounds'] is not None and r >= a['rounds']:
                continue
            p = subprocess.run([sys.executable] + COMMAND, env=dict(os.environ, **a['env']), cwd=a['tree'],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
            if p.returncode != 0:
                sys.exit('run %d of %s failed (%d): %s' % (r, a['name'], p.returncode, p.stderr.decode()[-800:]))
            d = json.loads(p.stdout.decode().strip().splitlines()[-1])
            runs[a['name']].append(d['value'])
            ms[a['name']].append(d.get('ms_per_step'))
            print(r, a['name'], d['value'], d.get('ms_per_step'), flush=True)
            summary = {n: dict(median=statistics.median(v), max_minus_min=round(max(v) - min(v), 3))
                       for n, v in runs.items() if v}
            with open(out, 'w') as f:
                json.dump(dict(command='python ' + ' '.join(COMMAND), unit='images/sec',
                               arms={b['name']: dict(env=b['env'], other_checkout=b['tree'] != ROOT) for b in arms},
                               runs=runs, ms_per_step=ms, summary=summary), f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), [parse(a) for a in sys.argv[3:]])
