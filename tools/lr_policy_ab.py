"""A/B of RUNLMC_LR_POLICY (csrc/rl_lowrank.h LrPolicy) on the benchmark's headline product, by the
rule of profiles/pair_policy/README.md: the sides take turns, alternation by alternation, in ONE job;
each run is a fresh `bench.py --gpus 1 --steps 20 --warmup 5` process, profiler off.

    python tools/lr_policy_ab.py --kern rbf --side parent=0 --side nt=1 --side nt_deep=9 [--side default=]

A side is NAME=VALUE; an empty VALUE leaves the knob unset (the library's choice).  The first
side is the one the others are held against.  One JSON line per run (side, alternation,
ms_per_step), then a verdict line per other side: its median gain over the first side, the larger
of the two ranges (max - min over the alternations), whether it was faster in EVERY alternation,
and `wins` = that and gain > 2 x range.  Any run that fails ends the job."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(kern, value, extra, seconds):
    env = dict(os.environ)
    env.pop('RUNLMC_LR_POLICY', None)
    if value != '':
        env['RUNLMC_DEBUG'] = '1'
        env['RUNLMC_LR_POLICY'] = value
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5',
           '--kern', kern] + extra
    out = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=seconds, text=True)
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit('bench.py exited with %d: the job ends here' % out.returncode)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kern', default='rbf')
    ap.add_argument('--side', action='append', required=True)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=240.0, help='time limit of one bench.py run')
    ap.add_argument('bench_args', nargs='*', help='further bench.py arguments (after --)')
    a = ap.parse_args()
    sides = [s.split('=', 1) for s in a.side]
    ms = {name: [] for name, _ in sides}
    for alt in range(1, a.alternations + 1):
        for name, value in sides:
            rec = run_bench(a.kern, value, a.bench_args, a.seconds)
            t = rec.get('ms_per_step')
            if t is None:
                t = 1e3 / rec['value']
            ms[name].append(t)
            print(json.dumps(dict(side=name, policy=value if value != '' else None, kern=a.kern,
                                  alternation=alt, ms_per_step=t, value=rec.get('value'),
                                  unit=rec.get('unit'))), flush=True)
    first = sides[0][0]
    base = np.array(ms[first])
    for name, _ in sides[1:]:
        v = np.array(ms[name])
        gain = float(np.median(base) - np.median(v))
        rng = float(max(base.max() - base.min(), v.max() - v.min()))
        every = bool(np.all(v < base))
        print(json.dumps(dict(verdict=name, against=first, kern=a.kern, median_ms=float(np.median(v)),
                              against_median_ms=float(np.median(base)), gain_ms=gain, range_ms=rng,
                              faster_in_every_alternation=every, wins=bool(every and gain > 2 * rng))),
              flush=True)


if __name__ == '__main__':
    main()
