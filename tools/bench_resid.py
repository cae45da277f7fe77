#!/usr/bin/env python3
"""The residual kernels (k_resid2d / k_resid3d) on one GPU: time, traffic, and what to hold them against.

Shapes: C2 (lat-lon Poisson 3600 x 1800 with a land mask; one and eight members, A and C shared, B NULL) and one C5
volume (omega 50 x 360 x 720, A B C shared).  Device-resident float64 arrays through xinv_residual_<form>_f64_dev.  Per shape:
  * resid_ms: HIP events around `--reps` queued launches without norms (median of the per-launch time over `--rounds`
    rounds, after warm-up), and resid_norms_ms: the wall time of a call that also brings the four norms to the host;
  * must_move: the bytes a residual must move -- S, every distinct array, R, each once -- and the rate that gives;
  * copy_ms: a device-to-device copy that moves the same number of bytes (must_move / 2 read + as many written),
    measured in the same run the same way, and the residual's rate as a fraction of the copy's;
  * sweep_ms: one solver sweep of the same problem (xinv_stats.sweep_ms of a 64-sweep resident solve / 64).
No threshold: nobody has measured this before; the numbers go to profiles/resid_bench.txt.

  python tools/bench_resid.py [--reps N] [--rounds N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xinvert_amd import _lib, forms, synthetic          # noqa: E402
from xinvert_amd.resident import ResidentProblem, scalars   # noqa: E402


def events_ms(fn, reps, rounds, warm=3):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def bench(name, p, reps, rounds):
    import torch
    L = _lib.require_gpu()
    rp = ResidentProblem(p, device=0)
    kind, nb, n = rp.kind, rp.nb, rp.n
    # the arrays in full, as the residual entry takes them (a coefficient kept as one value per row is expanded once)
    cs, strides = rp.full_arrays()
    strides = [n] + strides
    distinct = sum(c.numel() for c in cs if c is not None)
    R = torch.empty_like(rp.S)
    st = torch.cuda.current_stream(rp.dev)
    fn = getattr(L, forms.symbol(kind, 'resid_dev'))
    args = [_lib.dptr(R), _lib.dptr(rp.S)] + [_lib.dptr(c) for c in cs] + [nb, _lib.strides_arg(strides)] + scalars(rp.p)
    norms = np.zeros((nb, 4))

    def launch():
        _lib.check(fn(*args, None, ctypes.c_void_p(st.cuda_stream)))

    rms = events_ms(launch, reps, rounds)
    torch.cuda.synchronize()
    wall = []
    for _ in range(5):
        t0 = time.perf_counter()
        _lib.check(fn(*args, _lib.hptr(norms), ctypes.c_void_p(st.cuda_stream)))
        wall.append((time.perf_counter() - t0) * 1e3)
    must = 8 * (rp.S.numel() + distinct + R.numel())
    src = torch.empty(must // 16, dtype=torch.float64, device=rp.dev).normal_()
    dst = torch.empty_like(src)
    cms = events_ms(lambda: dst.copy_(src), reps, rounds)
    _, stats = rp.solve(63, 0.0, timing=1)
    sweep_ms = stats['sweep_ms'] / max(1, stats['sweeps_max'])
    r, c = float(np.median(rms)), float(np.median(cms))
    row = {'shape': name, 'kind': kind, 'members': nb, 'core': list(rp.core), 'resid_ms': round(r, 4),
           'resid_ms_min': round(min(rms), 4), 'resid_norms_wall_ms': round(float(np.median(wall)), 4),
           'must_move_bytes': must, 'resid_GBps': round(must / r / 1e6, 1), 'copy_ms': round(c, 4),
           'copy_GBps': round(must / c / 1e6, 1), 'resid_over_copy_rate': round(c / r, 3),
           'sweep_ms': round(sweep_ms, 4), 'solver_path': stats['path'], 'resid_over_sweep_time': round(r / sweep_ms, 3),
           'norms_member0': [float(v) for v in norms[0]]}
    rp.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resid_bench.txt'))
    a = ap.parse_args()
    lines = ['== python tools/bench_resid.py --reps %d --rounds %d (float64, device-resident, one GPU)' % (a.reps, a.rounds),
             '# resid_ms: HIP events around queued xinv_residual_*_f64_dev launches without norms, per launch, median of the rounds',
             '# must_move: S + every distinct array + R, once each; copy: a device-to-device copy moving the same bytes (half read, half written)',
             '# sweep_ms: xinv_stats.sweep_ms of a 64-sweep resident solve of the same problem / 64']
    for name, make in (('C2 x1', lambda: synthetic.poisson_latlon(1800, 3600, mask=True, members=1)),
                       ('C2 x8', lambda: synthetic.poisson_latlon(1800, 3600, mask=True, members=8)),
                       ('C5 x1', lambda: synthetic.omega_latlon(50, 360, 720, steps=1))):
        lines.append(json.dumps(bench(name, make(), a.reps, a.rounds)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
