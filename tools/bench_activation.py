"""update() step time per encoder activation: bench.py's own headline measurement (BASELINE.json configs[1]: V = 100, 4 cameras of
128^2, B = 16, depth 6, 2048 latents; its synthetic batches, warmup and timed region) with `method.activation` set to each value.

    python tools/bench_activation.py [--rounds 3] [--steps 8] [--warmup 2] [--activations lrelu,relu,tanh]

Every measurement is a fresh child process that imports bench.py and runs its main() with launch_utils.default_cfg wrapped to add
`method__activation` -- nothing of the measurement is re-implemented here.  The activations are interleaved round by round (the same
box, drifting clocks spread over all of them); one JSON line: per activation every ms_per_step, their median / min / max, and the
median ratio to lrelu."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
sys.path.insert(0, {root!r})
import bench
from voxactb_amd.agents.peract_bc import launch_utils as lu
_default_cfg = lu.default_cfg
lu.default_cfg = lambda **over: _default_cfg(method__activation={act!r}, **over)
sys.argv = ['bench.py', '--gpus', '1', '--steps', {steps!r}, '--warmup', {warmup!r}, '--no-cpu-baseline', '--no-other-modes']
bench.main()
'''


def one_run(act, steps, warmup, timeout):
    code = CHILD.format(root=ROOT, act=act, steps=str(steps), warmup=str(warmup))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench.py with activation=%s exited with %d' % (act, r.returncode))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    return float(json.loads(line)['ms_per_step'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--activations', default='lrelu,relu,tanh')
    ap.add_argument('--timeout', type=int, default=600, help='seconds per child run')
    a = ap.parse_args()
    acts = a.activations.split(',')
    ms = {act: [] for act in acts}
    for _ in range(a.rounds):
        for act in acts:
            ms[act].append(round(one_run(act, a.steps, a.warmup, a.timeout), 2))
    res = dict(metric='update_ms_per_step_per_activation', V=100, B=16, steps=a.steps, rounds=a.rounds, runs=ms)
    for act in acts:
        res[act] = dict(median=statistics.median(ms[act]), min=min(ms[act]), max=max(ms[act]))
    if 'lrelu' in ms:
        base = statistics.median(ms['lrelu'])
        res['median_ratio_to_lrelu'] = {act: round(statistics.median(ms[act]) / base, 4) for act in acts}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
