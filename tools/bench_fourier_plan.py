#!/usr/bin/env python3
"""A Fourier plan (xinv_fourier_plan_*: k_fourier_factor once, then k_fourier_check, k_rowdft x 3 and k_fourier_subst per
solve) against the one-shot entry xinv_fourier_standard_2d_f64_dev on the same problem, one GPU.

Unmasked lat-lon Poisson problems (synthetic.poisson_latlon) at 360 x 180 x 1, 3600 x 1800 x 1 and 3600 x 1800 x 8, shared
coefficients, float64, device-resident.
  plan_ms            HIP events around `--reps` (>= 20) QUEUED plan solves after warm-up, divided by the count; the median of
                     `--rounds` such windows.  Nothing waits on the host inside a window.
  oneshot_sweep_ms   xinv_stats.sweep_ms of the one-shot entry in the same run (its own events around its four launches: two
                     forward transforms, k_fourier_tri, the inverse transform; the check pass and both host round trips lie
                     outside them), median of `--reps` calls.  That code is the parent commit's.
  oneshot_entry_ms   events around the whole one-shot call, for the caller's view.
  subst_ms           k_fourier_subst: what is left of plan_ms after the three transforms, each timed alone with the same
                     events through xinv_rowdft_f64_dev on the solve's rows.  The check pass, the memset and the 8 nb byte
                     copy are in this figure too (the plan has no entry that runs one kernel), so it is an upper bound;
                     `--solves-only` is the body to put under a kernel trace for the kernel's own time.
  create_ms          host clock around FourierPlan(...): allocations, the copies of A and C, k_fourier_factor, the host wait.
  plan_bytes         what the plan holds in HBM.
Both results are compared bitwise.  Writes profiles/fourier_plan_bench.txt, then asserts the one condition: at
3600 x 1800 x 1 plan_ms is not above oneshot_sweep_ms.

  python tools/bench_fourier_plan.py [--reps N] [--rounds N] [--out FILE] [--solves-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import xinvert_amd as xa                           # noqa: E402
from xinvert_amd import _lib, synthetic            # noqa: E402
from xinvert_amd.resident import ResidentProblem   # noqa: E402

UNDEF = -9.99e8
SIZES = ((360, 180, 1), (3600, 1800, 1), (3600, 1800, 8))


def window_ms(fn, count):
    """HIP events around `count` calls of fn() queued back to back -> ms per call."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / count


def median_window(fn, count, rounds, warm=3):
    for _ in range(warm):
        fn()
    return float(np.median([window_ms(fn, count) for _ in range(rounds)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fourier_plan_bench.txt'))
    ap.add_argument('--solves-only', action='store_true', help='create, warm up and queue --reps solves per size; no file')
    args = ap.parse_args()
    assert args.reps >= 20 or args.solves_only, 'time at least 20 queued solves'
    import torch
    L = _lib.require_gpu()
    # (the one-shot entry times its launches with the workspace's events, which the first timed sweep solve creates)
    warm = ResidentProblem(synthetic.poisson_latlon(18, 36, mask=False), device=0)
    warm.solve(4, 1e-30, timing=1)
    warm.close()
    lines = ['== python tools/bench_fourier_plan.py --reps %d --rounds %d (lat-lon Poisson, unmasked, shared A and C, float64, '
             'device-resident)' % (args.reps, args.rounds),
             '# plan_ms: events around --reps queued plan solves / --reps, median of --rounds windows; oneshot_sweep_ms: '
             "xinv_stats.sweep_ms of xinv_fourier_standard_2d_f64_dev (its four launches), median of --reps calls",
             '# subst_ms: plan_ms minus the three transforms timed alone (check pass, memset and status copy included: an upper bound)']
    rows = []
    for xc, yc, nb in SIZES:
        p = synthetic.poisson_latlon(yc, xc, mask=False, members=nb)
        K, n = xc // 2 + 1, yc * xc
        A, C = (torch.from_numpy(np.ascontiguousarray(np.asarray(p['coefs'][q])[:, 0])).cuda() for q in (0, 2))
        F = torch.from_numpy(np.ascontiguousarray(p['coefs'][3], dtype=np.float64).reshape(nb, yc, xc)).cuda()
        S0 = torch.from_numpy(np.ascontiguousarray(p['S0'], dtype=np.float64).reshape(nb, yc, xc)).cuda()
        S, S1 = S0.clone(), S0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = xa.FourierPlan(A, C, nb, yc, xc, p['delxSqr'], p['ratioSqr'], undef=UNDEF)
        create_ms = (time.perf_counter() - t0) * 1e3
        solve = lambda: plan.solve(S, F)
        if args.solves_only:
            for _ in range(3 + args.reps):
                solve()
            assert not plan.status()[0].any()
            plan.close()
            continue
        plan_ms = median_window(solve, args.reps, args.rounds)
        fl_p, bad = plan.status()
        # the one-shot entry: it waits on the host, so every call is a window of its own
        fl = np.zeros((nb, 3))
        st = torch.cuda.current_stream().cuda_stream
        sweep, entry = [], []
        for k in range(3 + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.xinv_fourier_standard_2d_f64_dev(S1.data_ptr(), A.data_ptr(), C.data_ptr(), F.data_ptr(), nb,
                                                          _lib.strides_arg([n, 0, 0, n]), yc, xc, p['delxSqr'], p['ratioSqr'],
                                                          UNDEF, _lib.hptr(fl), st))
            e1.record()
            e1.synchronize()
            if k >= 3:
                sweep.append(_lib.last_stats()['sweep_ms'])
                entry.append(e0.elapsed_time(e1))
        assert min(sweep) > 0, 'the one-shot entry did not time its launches'
        same = bool(torch.equal(S, S1))
        # the transforms on the solve's rows, alone
        rows_f = nb * (yc - 2)
        x = torch.zeros((rows_f, xc), dtype=torch.float64, device='cuda')
        X = torch.zeros((rows_f, K), dtype=torch.complex128, device='cuda')
        x2 = torch.zeros((2 * nb, xc), dtype=torch.float64, device='cuda')
        X2 = torch.zeros((2 * nb, K), dtype=torch.complex128, device='cuda')
        dft = lambda o, i, r, inv: (lambda: _lib.check(L.xinv_rowdft_f64_dev(o.data_ptr(), i.data_ptr(), r, xc, inv, st)))
        fwd = median_window(dft(X, x, rows_f, 0), args.reps, args.rounds)
        fwd2 = median_window(dft(X2, x2, 2 * nb, 0), args.reps, args.rounds)
        inv = median_window(dft(x, X, rows_f, 1), args.reps, args.rounds)
        del x, X, x2, X2
        b_subst = nb * (yc - 2) * K * (16 * 4 + 8 * 2) + nb * 2 * K * 16      # spectrum in and out, twice; inv and gamma in; the known rows
        rows.append({'xc': xc, 'yc': yc, 'members': nb, 'plan_ms': round(plan_ms, 4),
                     'oneshot_sweep_ms': round(float(np.median(sweep)), 4), 'oneshot_entry_ms': round(float(np.median(entry)), 4),
                     'plan_over_oneshot_sweep': round(plan_ms / float(np.median(sweep)), 3),
                     'rowdft_forward_F_ms': round(fwd, 4), 'rowdft_forward_S_ms': round(fwd2, 4), 'rowdft_inverse_ms': round(inv, 4),
                     'subst_ms': round(plan_ms - fwd - fwd2 - inv, 4), 'subst_bytes': int(b_subst),
                     'create_ms': round(create_ms, 3), 'plan_bytes': int(plan.nbytes), 'bitwise_equal': same,
                     'overflow_members': int(fl_p[:, 0].sum()), 'undef_members': int((bad != 0).sum())})
        lines.append(json.dumps(rows[-1]))
        print(lines[-1], flush=True)
        plan.close()
        del S, S1, F, S0
        torch.cuda.empty_cache()
    if args.solves_only:
        return
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    assert all(r['bitwise_equal'] for r in rows), 'a plan solve differs from the one-shot entry'
    # the one condition
    r = rows[1]
    assert r['plan_ms'] <= r['oneshot_sweep_ms'], \
        'the plan solve is above the one-shot launches at 3600 x 1800 x 1: %s ms against %s ms' % (r['plan_ms'], r['oneshot_sweep_ms'])


if __name__ == '__main__':
    main()
