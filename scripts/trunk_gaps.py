"""Idle time of the trunk in the 1024^2 forward, from a rocprofv3 --kernel-trace CSV (kernel trace only, no counters) of
`bench.py --gpus 1 --steps 5 --warmup 1`:

    python scripts/trunk_gaps.py <kernel_trace.csv> [skip_steps=2] > profiles/..._trunk_gaps.json

A forward ends with `conv_wino36h_rgb_kernel` (layer 18 with ToRGB in its epilogue); the trunk is the queue those launches
run on (the RGB branch and the prefetch have their own).  Per steady step (the first `skip_steps` forwards -- the ones that
load code objects and pack weights -- are left out; the first one kept still carries the timer's synchronisation in its
sum of gaps, so read the medians) it prints

  gap_17_18_us     end of the last `tconv_blur_ws_kernel` launch in front of layer 18 (layer 17) -> start of layer 18: where
                   the trunk waits for the RGB stream (StyledConvSeq._run_final);
  trunk_gaps_us    the sum of all gaps between consecutive trunk launches of the step (a launch that starts before the one
                   in front has ended counts as no gap);
  trunk_busy_ms / step_ms   the sum of the trunk launches' durations / first start to last end;
  largest          the five largest gaps with the kernels on either side.
"""
import csv
import json
import statistics
import sys

LAST = 'conv_wino36h_rgb_kernel'
L17 = 'tconv_blur_ws_kernel'


def short(name):
    return name.split('(')[0].split('<')[0].replace('void ', '').strip()


def main(path, skip_steps=2):
    rows = list(csv.DictReader(open(path)))
    lane = 'Stream_Id' if rows and 'Stream_Id' in rows[0] and len({r['Stream_Id'] for r in rows}) > 1 else 'Queue_Id'
    lanes = {r[lane] for r in rows if short(r['Kernel_Name']) == LAST}
    if len(lanes) != 1:
        sys.exit('%s runs on %d %ss: not the trace of one default forward per step' % (LAST, len(lanes), lane))
    trunk = sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])) for r in rows
                    if r[lane] in lanes))
    steps, cur = [], []
    for k in trunk:
        cur.append(k)
        if k[2] == LAST:
            steps.append(cur)
            cur = []
    out = []
    for step in steps[skip_steps:]:
        gaps = [(max(0, b[0] - a[1]), a[2], b[2]) for a, b in zip(step, step[1:])]
        l17 = [k for k in step if k[2] == L17]
        out.append(dict(
            gap_17_18_us=round((step[-1][0] - l17[-1][1]) / 1e3, 1) if l17 else None,
            trunk_gaps_us=round(sum(g[0] for g in gaps) / 1e3, 1),
            trunk_busy_ms=round(sum(e - s for s, e, _ in step) / 1e6, 3),
            step_ms=round((step[-1][1] - step[0][0]) / 1e6, 3),
            launches=len(step),
            largest=[dict(us=round(g / 1e3, 1), after=a, before=b) for g, a, b in sorted(gaps, reverse=True)[:5]]))
    med = {k: statistics.median(s[k] for s in out) for k in ('gap_17_18_us', 'trunk_gaps_us', 'trunk_busy_ms', 'step_ms')
           if out and all(s[k] is not None for s in out)}
    json.dump(dict(trace=path.split('/')[-1], trunk_lane='%s %s' % (lane, min(lanes)), steady_steps=len(out), median=med,
                   steps=out), sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 2)
