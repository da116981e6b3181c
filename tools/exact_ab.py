"""Two builds of the native library side by side on the exact likelihood's kernel-evaluating
steps: seconds of rl_exact_assemble and of the gradient sums (ExactOp.grad_sums) for a
plain-kernel model, by tools/exact_probe.py's method (wall clock around the synchronous call) at
its smallest size (3054, the FX2007 fixture).

    python tools/exact_ab.py --lib PARENT.so --lib runlmc_amd/csrc/librunlmc_hip.so [--reps 9]

The libraries take turns repetition by repetition, in one process, each on a handle of its own;
one JSON line per library with every repetition, the median and the max - min spread, then a
verdict line: the last library's median may exceed the first's by no more than the first's own
spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from exact_probe import problem, timed        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', action='append', required=True)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--n', type=int, default=3054)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'exact_ab.py measures the GPU: no GPU visible'
    from runlmc_amd import _lib
    from runlmc_amd._native import ExactOp
    fk, Xs, Ys, label = problem(a.n)
    X = np.vstack([np.asarray(x, dtype=float).reshape(len(x), -1) for x in Xs])
    y = np.hstack(Ys)
    lens = [len(v) for v in Ys]
    ops, times = [], []
    for path in a.lib:
        lib = _lib.NativeLib(os.path.abspath(path))
        assert lib.is_hip, path
        op = ExactOp(len(y), X.shape[1], lib=lib)
        op.set(X, lens, fk.kernels, fk.coreg_mats(), fk.noise)
        ops.append(op)
        times.append(dict(assemble_s=[], grad_sums_s=[]))
    ydev = torch.from_numpy(y).to(ops[0].device)
    sums = []
    for rep in range(a.reps + 1):                  # (repetition 0 warms up: code objects, allocator)
        for op, t in zip(ops, times):
            ta, _ = timed(op.assemble)
            op.factor()
            alpha = op.solve(ydev)
            op.invert()
            tg, out = timed(lambda: op.grad_sums(alpha))
            if rep:
                t['assemble_s'].append(ta)
                t['grad_sums_s'].append(tg)
            else:
                sums.append(out)
    same = all(np.array_equal(u, v) for s in sums[1:] for u, v in zip(sums[0], s))
    recs = []
    for path, t in zip(a.lib, times):
        rec = dict(lib=path, n=len(y), problem=label, reps=a.reps)
        for key, v in t.items():
            rec[key] = v
            rec[key[:-2] + '_median_s'] = float(np.median(v))
            rec[key[:-2] + '_spread_s'] = float(np.max(v) - np.min(v))
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    verdict = dict(same_gradient_sums=bool(same))
    for key in ('assemble', 'grad_sums'):
        over = recs[-1][key + '_median_s'] - recs[0][key + '_median_s']
        verdict[key + '_median_excess_s'] = over
        verdict[key + '_within_first_spread'] = bool(over <= recs[0][key + '_spread_s'])
    print(json.dumps(verdict), flush=True)


if __name__ == '__main__':
    main()
