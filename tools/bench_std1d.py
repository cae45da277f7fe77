#!/usr/bin/env python3
"""Throughput of the 1-D standard form (k_std1d, xinvert_amd/csrc/xinv_std1d.h) on one GPU.

Fixed sweep counts (tolerance 0 never stops early; mxLoop 5000 -> 5001 sweeps) on
  batch   64 x 360 = 23 040 members x 181 points (GeoAdjustment-like lat sections, member-varying B and F, shared A)
  single  one member of 501 points (the reference's GeoAdjustment case size)
and prints one JSON line per case: point-sweeps/s over the HIP-event time of the launch chain, wall time of the whole
call, sweep_launches (= ceil(sweeps / budget) + at most check_every no-op launches).

  python tools/bench_std1d.py [--case batch|single|all] [--reps N] [--mxloop N]
For the VALU-busy fraction run ONE case under a counter collection of its own, e.g.
  rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d DIR -o pmc -- \
      python tools/bench_std1d.py --case batch --reps 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xinvert_amd import _lib          # noqa: E402

UNDEF = -9.99e8


def problem(nb, xc, seed=0):
    rng = np.random.default_rng(seed)
    lat = np.deg2rad(np.linspace(-80, -10, xc))
    A = np.cos(lat) / np.sin(lat) * -1.0                     # positive, smooth (cos / |f|-like)
    B = -rng.uniform(0.1, 0.5, (nb, xc))
    F = rng.standard_normal((nb, xc))
    return np.zeros((nb, xc)), A, B, F


def run(nb, xc, mxloop, reps):
    L = _lib.require_gpu()
    S0, A, B, F = problem(nb, xc)
    best = None
    for _ in range(reps + 1):                                # (the first call warms up: module load, allocations)
        S = S0.copy()
        fl = np.tile([0.0, 1.0, 0.0], (nb, 1))
        t0 = time.perf_counter()
        rc = L.xinv_standard_1d_f64_batched(_lib.hptr(S), _lib.hptr(A), _lib.hptr(B), _lib.hptr(F), nb,
                                            _lib.strides_arg([xc, 0, xc, xc]), xc, 1.0, 0, 1.0, 1.6, UNDEF,
                                            _lib.hptr(fl), mxloop, 0.0, _lib.options(timing=1))
        wall = time.perf_counter() - t0
        _lib.check(rc)
        st = _lib.last_stats()
        rec = dict(case='%dx%d' % (nb, xc), members=nb, points=xc, sweeps=int(st['sweeps_max']),
                   sweep_launches=int(st['sweep_launches']), budget=int(st['sweeps_per_launch']),
                   sweep_ms=st['sweep_ms'], wall_ms=wall * 1e3,
                   point_sweeps_per_s=nb * xc * st['sweeps_max'] / (st['sweep_ms'] * 1e-3),
                   overflow=int(fl[:, 0].max()), finite=bool(np.isfinite(S).all()))
        if best is None or rec['sweep_ms'] < best['sweep_ms']:
            best = rec
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['batch', 'single', 'all'])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--mxloop', type=int, default=5000)
    a = ap.parse_args()
    cases = {'batch': (64 * 360, 181), 'single': (1, 501)}
    for name in (['batch', 'single'] if a.case == 'all' else [a.case]):
        r = run(*cases[name], a.mxloop, a.reps)
        r['name'] = name
        print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
