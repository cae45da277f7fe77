#!/usr/bin/env python3
"""invert_MultiGrid against the single-grid solve on C2 (the masked 3600 x 1800 invert_Poisson of
synthetic.poisson_latlon), and the throughput of its grid transfers k_mg_restrict / k_mg_prolong.

Default mode: one warm-up call of each, then single-grid invert_Poisson and invert_MultiGrid (ratio 3, gridNo 3) with
the same tolerance and mxLoop; prints, per run, the finest-level sweeps, the wall time and the rel-L2 error against a
tightly converged single-grid solution (tolerance 1e-14), one JSON line each.

--kernels: restriction (3 x 3 and 9 x 9) and prolongation (3 x 3) on device-resident 8 x 1800 x 3600 float64 arrays,
timed with HIP events after warm-up; bytes = the fine array read once (+ the fine forcing read and S written for the
prolongation) plus the coarse array written / read once.  Kernel times without launch gaps:
  rocprofv3 --kernel-trace --stats -d DIR -o mg -- python tools/bench_mg.py --kernels

  python tools/bench_mg.py [--tolerance T] [--mxLoop N] [--kernels [--reps N]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xinvert_amd import Field, invert_MultiGrid, invert_Poisson, synthetic   # noqa: E402
from xinvert_amd import multigrid as mg                                       # noqa: E402

SHAPE = (8, 1800, 3600)


def rel_l2(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.linalg.norm((a - b)[ok]) / np.linalg.norm(b[ok]))


def c2_field():
    p = synthetic.poisson_latlon(1800, 3600, mask=True)
    return Field(p['zeta'][0], ('lat', 'lon'), {'lat': p['lat'], 'lon': p['lon']})


def solve_runs(args):
    F = c2_field()
    dims = ['lat', 'lon']
    base = {'BCs': ['fixed', 'periodic'], 'printInfo': False}
    invert_Poisson(F, dims, iParams=dict(base, mxLoop=10, tolerance=args.tolerance))          # (warm-up)
    invert_MultiGrid(invert_Poisson, F, dims, iParams=dict(base, mxLoop=10, tolerance=args.tolerance))
    ip = dict(base, tolerance=1e-14, mxLoop=args.tight_mxLoop)
    t0 = time.perf_counter()
    R = invert_Poisson(F, dims, iParams=ip)
    t1 = time.perf_counter()
    ref = R.values
    print(json.dumps({'run': 'tight_single_grid', 'tolerance': 1e-14, 'sweeps': float(ip_flags(R, ip)),
                      'wall_s': round(t1 - t0, 3)}), flush=True)
    ip = dict(base, tolerance=args.tolerance, mxLoop=args.mxLoop)
    t0 = time.perf_counter()
    S = invert_Poisson(F, dims, iParams=ip)
    t1 = time.perf_counter()
    print(json.dumps({'run': 'single_grid', 'tolerance': args.tolerance, 'mxLoop': args.mxLoop,
                      'finest_sweeps': float(ip_flags(S, ip)), 'wall_s': round(t1 - t0, 3),
                      'rel_l2_vs_tight': rel_l2(S.values, ref)}), flush=True)
    ip = dict(base, tolerance=args.tolerance, mxLoop=args.mxLoop)
    t0 = time.perf_counter()
    S, fs, os_ = invert_MultiGrid(invert_Poisson, F, dims, iParams=ip, ratio=3, gridNo=3)
    t1 = time.perf_counter()
    print(json.dumps({'run': 'multigrid', 'ratio': 3, 'gridNo': 3, 'tolerance': args.tolerance, 'mxLoop': args.mxLoop,
                      'levels': [list(f.shape) for f in fs],
                      'level_sweeps': [float(np.max(np.asarray(f)[..., 2])) for f in ip['mg_flags']],
                      'finest_sweeps': float(np.max(np.asarray(ip['flags'])[..., 2])), 'wall_s': round(t1 - t0, 3),
                      'rel_l2_vs_tight': rel_l2(S.values, ref)}), flush=True)


def ip_flags(S, ip):
    fl = getattr(S, 'iParams', ip).get('flags')
    return np.max(np.asarray(fl)[..., 2])


def kernel_runs(args):
    import torch
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    fine = torch.randn(SHAPE, dtype=torch.float64, device=dev, generator=g)
    force = torch.randn(SHAPE, dtype=torch.float64, device=dev, generator=g)
    S = torch.zeros(SHAPE, dtype=torch.float64, device=dev)
    n = int(np.prod(SHAPE))
    lat = np.linspace(-90.0, 90.0, SHAPE[1])
    lon = np.arange(SHAPE[2]) * 0.1
    coarse3 = mg.restrict_dev(fine, (3, 3), np.nan)
    tabs = [mg.prolong_table(lat, mg.coarse_coord(lat, 3), False), mg.prolong_table(lon, mg.coarse_coord(lon, 3), True)]
    cases = [('restrict_3x3', lambda: mg.restrict_dev(fine, (3, 3), np.nan), 8 * n + 8 * n // 9),
             ('restrict_9x9', lambda: mg.restrict_dev(fine, (9, 9), np.nan), 8 * n + 8 * n // 81),
             ('prolong_3x3', lambda: mg.prolong_dev(coarse3, S, tabs, 1, force, -9.99e8), 16 * n + 8 * n // 9)]
    for name, fn, byts in cases:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        best = min(ms)
        print(json.dumps({'op': name, 'shape': SHAPE, 'bytes': byts, 'event_ms_min': round(best, 4),
                          'event_ms_median': round(float(np.median(ms)), 4),
                          'TBps_event_min': round(byts / best / 1e9, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tolerance', type=float, default=1e-10)
    ap.add_argument('--mxLoop', type=int, default=100000)
    ap.add_argument('--tight-mxLoop', dest='tight_mxLoop', type=int, default=200000)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if args.kernels:
        kernel_runs(args)
    else:
        solve_runs(args)


if __name__ == '__main__':
    main()
