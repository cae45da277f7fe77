#!/usr/bin/env python3
"""The direct path of the 1-D standard form (k_tridiag, XINV_PATH_DIRECT1D) against the SOR sweeps (k_std1d) on one GPU.

Two GeoAdjustment problems (the coefficients of apps.invert_GeoAdjustment on a step in h0 between 75S and 25S, as the
reference's own test case) on device-resident float64 arrays through xinv_standard_1d_f64_dev, 'extend', one shared A:
23 040 members x 181 points (the step height differs from member to member) and one member x 501 points.  Direct path: HIP events around the launch (xinv_options.timing),
median of `--reps` runs after warm-up, S reset to the first guess before every run.  SOR path: the same data at the
front end's defaults (tolerance 1e-8, mxLoop 5000), median of `--sor-reps` runs.  Traffic: the bytes the direct path
must move (S0, B, F read once, S written once, A shared) over the event time, beside the bytes its three passes do
move (forward: 3 reads + 2 writes; backward: 2 reads + 1 write).  Writes profiles/tridiag_bench.txt, then asserts the
one condition: the direct path is faster than the sweeps on both shapes.

  python tools/bench_tridiag.py [--reps N] [--sor-reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xinvert_amd import _lib          # noqa: E402

UNDEF = -9.99e8
COPY_TBS = 6.29                        # measured float4 copy rate of the MI355X (TB/s)


def geo_problem(nb, xc):
    """apps._coeffs_GeoAdjustment / _cal_params1D written out: A = cosH / fH, B = -f cosG / (g h0), F = -f cosG / g."""
    R, OMEGA, G = 6371200.0, 7.292e-5, 9.80665
    lat = np.linspace(-75, -25, xc)
    lats = np.deg2rad(lat)
    sh = np.concatenate([[np.nan], lats[:-1]])
    h0 = np.full((nb, xc), 1500.0)
    h0[:, xc // 2:] += 20.0 * (1.0 + np.arange(nb)[:, None] / nb)
    f, cosG = 2 * OMEGA * np.sin(lats), np.cos(lats)
    A = np.cos((lats + sh) / 2.0) / (2 * OMEGA * np.sin((lats + sh) / 2.0))
    B = -f * cosG / G / h0
    F = np.broadcast_to(-f * cosG / G, (nb, xc)).copy()
    return A, B, F, (np.deg2rad(lat[1] - lat[0]) * R) ** 2.0


def run(L, t, S0, nb, xc, dsq, path, reps, warm):
    import torch
    strides = _lib.strides_arg([xc, 0, xc, xc])
    fl = np.tile([0.0, 1.0, 0.0], (nb, 1))
    opt = _lib.options(path=path, timing=1)
    st = torch.cuda.current_stream().cuda_stream
    ms, sweeps = [], 0
    for k in range(warm + reps):
        t[0].copy_(S0)
        _lib.check(L.xinv_standard_1d_f64_dev(*[v.data_ptr() for v in t], nb, strides, xc, 1.0, _lib.bc('extend'), dsq,
                                              1.8, UNDEF, _lib.hptr(fl), 5000, 1e-8, opt, st))
        s = _lib.last_stats()
        if k >= warm:
            ms.append(s['sweep_ms'])
        sweeps = s['sweeps_max']
    return ms, sweeps, int(fl[:, 0].sum()), float(fl[:, 1].max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--sor-reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tridiag_bench.txt'))
    args = ap.parse_args()
    import torch
    L = _lib.require_gpu()
    dev = torch.device('cuda', 0)
    lines = ['== python tools/bench_tridiag.py --reps %d --sor-reps %d (GeoAdjustment, float64, device-resident, \'extend\', shared A)'
             % (args.reps, args.sor_reps),
             '# event_ms: HIP events around the launches of one xinv_standard_1d_f64_dev call (xinv_stats.sweep_ms)',
             '# must_move: S0, B, F read once + S written once; moved: the three passes of k_tridiag (5 reads + 3 writes)']
    rows = []
    for nb, xc in ((23040, 181), (1, 501)):
        A, B, F, dsq = geo_problem(nb, xc)
        S0 = np.zeros((nb, xc))
        t = [torch.tensor(v, dtype=torch.float64, device=dev) for v in (S0, A, B, F)]
        S0d = t[0].clone()
        torch.cuda.synchronize()
        dms, _, dovf, _ = run(L, t, S0d, nb, xc, dsq, _lib.PATH_DIRECT1D, args.reps, 3)
        Sd = t[0].cpu().numpy()
        sms, sweeps, sovf, sfl1 = run(L, t, S0d, nb, xc, dsq, _lib.PATH_AUTO, args.sor_reps, 1)
        Ss = t[0].cpu().numpy()
        dmed, smed = float(np.median(dms)), float(np.median(sms))
        must, moved = 4 * 8 * nb * xc + 8 * xc, 8 * 8 * nb * xc + 8 * xc
        rows.append({
            'members': nb, 'xc': xc, 'direct_event_ms_median': round(dmed, 4), 'direct_event_ms_min': round(min(dms), 4),
            'sor_event_ms_median': round(smed, 4), 'sor_sweeps': int(sweeps), 'speedup': round(smed / dmed, 1),
            'must_move_bytes': must, 'must_move_TBps': round(must / dmed / 1e9, 4),
            'frac_of_copy_rate': round(must / dmed / 1e9 / COPY_TBS, 4), 'moved_bytes': moved,
            'moved_TBps': round(moved / dmed / 1e9, 4), 'overflow_members': [dovf, sovf],
            'sor_flags1_max': sfl1, 'rel_l2_direct_vs_sor': float(np.linalg.norm(Sd - Ss) / np.linalg.norm(Sd))})
        lines.append(json.dumps(rows[-1]))
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    # the one condition: on both shapes the direct solve is faster than the sweeps it replaces
    slow = [(r['members'], r['xc'], r['direct_event_ms_median'], r['sor_event_ms_median']) for r in rows
            if not r['direct_event_ms_median'] < r['sor_event_ms_median']]
    assert not slow, 'the direct path is not faster than the sweeps (members, xc, direct ms, sor ms): %s' % slow


if __name__ == '__main__':
    main()
