#!/usr/bin/env python3
"""The direct Fourier solve of the 2-D standard form (k_rowdft, k_fourier_tri, k_fourier_check) against a resident SOR solve
of the same problem on one GPU.

Unmasked lat-lon Poisson problems (synthetic.poisson_latlon, the coefficients of apps.invert_Poisson) at 360 x 180,
3600 x 1800 x 1 and 3600 x 1800 x 8, float64, device-resident.  'fourier': HIP events around xinv_fourier_standard_2d_f64_dev
(the whole entry: check pass and its read-back, transforms, recurrence, the flags' read-back), median of `--reps` calls
after warm-up, S reset before every call.  'sor': ResidentProblem.solve at tolerance 1e-10 (xinv_stats.sweep_ms), median of
`--sor-reps`.  Both fields go through ResidentProblem.residual(): max|R| / max|F|.  Per kernel: the bytes it must move and
its rate against a device copy of the same bytes, timed here with the same events.  k_rowdft is timed through
xinv_rowdft_f64_dev on the solve's rows; the recurrence is what is left of xinv_stats.sweep_ms (events around the four
launches) after the transforms, the check pass what is left of the entry after that -- two host round trips included, so
its rate is a lower bound.  Writes profiles/fourier_bench.txt, then asserts the one condition: 'fourier' is faster than
'sor' at 3600 x 1800 x 1.

  python tools/bench_fourier.py [--reps N] [--sor-reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xinvert_amd import _lib, synthetic          # noqa: E402
from xinvert_amd.resident import ResidentProblem   # noqa: E402

UNDEF = -9.99e8


def timed(fn, reps, warm):
    """Median and minimum (ms) of HIP events around fn() on the current stream."""
    import torch
    ms = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warm:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def copy_ms(nbytes, reps):
    """A device copy that moves `nbytes` in all (half read, half written)."""
    import torch
    n = max(1, int(nbytes) // 16)
    a, b = torch.empty(n, dtype=torch.float64, device='cuda'), torch.empty(n, dtype=torch.float64, device='cuda')
    return timed(lambda: b.copy_(a), reps, 3)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sor-reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fourier_bench.txt'))
    args = ap.parse_args()
    import torch
    L = _lib.require_gpu()
    lines = ['== python tools/bench_fourier.py --reps %d --sor-reps %d (lat-lon Poisson, unmasked, float64, device-resident)'
             % (args.reps, args.sor_reps),
             '# fourier_ms: HIP events around xinv_fourier_standard_2d_f64_dev; sor_ms: xinv_stats.sweep_ms at tolerance 1e-10',
             '# resid: max|R| / max|F| by ResidentProblem.residual(); kernels: must-move bytes, ms, and the time of a device copy of the same bytes over it']
    rows = []
    for xc, yc, nb in ((360, 180, 1), (3600, 1800, 1), (3600, 1800, 8)):
        p = synthetic.poisson_latlon(yc, xc, mask=False, members=nb)
        rp = ResidentProblem(p, device=0)
        K, n = xc // 2 + 1, yc * xc
        A, C = (torch.from_numpy(np.ascontiguousarray(np.asarray(p['coefs'][q])[:, 0])).cuda() for q in (0, 2))
        F, S = rp.coefs[3], rp.S
        fl = np.zeros((nb, 3))
        st = torch.cuda.current_stream().cuda_stream

        def fourier():
            S.copy_(rp.S0)
            _lib.check(L.xinv_fourier_standard_2d_f64_dev(S.data_ptr(), A.data_ptr(), C.data_ptr(), F.data_ptr(), nb,
                                                          _lib.strides_arg([n, 0, 0, n]), yc, xc, p['delxSqr'], p['ratioSqr'],
                                                          UNDEF, _lib.hptr(fl), st))
        reset_ms = timed(lambda: S.copy_(rp.S0), args.reps, 3)[0]
        fmed, fmin = timed(fourier, args.reps, 3)
        fmed, fmin = fmed - reset_ms, fmin - reset_ms
        section = _lib.last_stats()['sweep_ms']
        ovf = int(fl[:, 0].sum())
        Sf = S.clone()
        f_res = rp.residual()[1]
        # the transforms on the solve's rows, alone
        rows_f = nb * (yc - 2)
        x = torch.zeros((rows_f, xc), dtype=torch.float64, device='cuda')
        X = torch.zeros((rows_f, K), dtype=torch.complex128, device='cuda')
        fwd = timed(lambda: _lib.check(L.xinv_rowdft_f64_dev(X.data_ptr(), x.data_ptr(), rows_f, xc, 0, st)), args.reps, 3)[0]
        inv = timed(lambda: _lib.check(L.xinv_rowdft_f64_dev(x.data_ptr(), X.data_ptr(), rows_f, xc, 1, st)), args.reps, 3)[0]
        del x, X
        b_dft = rows_f * (xc * 8 + K * 16)
        b_tri = nb * (yc - 2) * K * (16 * 2 + 8 * 2) + nb * 2 * K * 16      # rhs in, solution out, the factors out and in; the two known rows
        b_chk = nb * yc * xc * 8
        tri = max(section - fwd * (1 + 2.0 / (yc - 2)) - inv, 1e-6)
        chk = max(fmed - section, 1e-6)
        kern = {}
        for name, b, ms in (('k_rowdft_forward', b_dft, fwd), ('k_rowdft_inverse', b_dft, inv), ('k_fourier_tri', b_tri, tri),
                            ('k_fourier_check', b_chk, chk)):
            kern[name] = {'must_move_bytes': int(b), 'ms': round(ms, 4), 'TBps': round(b / ms / 1e9, 3),
                          'copy_ms_over_ms': round(copy_ms(b, args.reps) / ms, 3)}
        # the sweeps
        sms, sweeps = [], 0
        for _ in range(args.sor_reps):
            rp.reset()
            sfl, stt = rp.solve(200000, 1e-10, timing=1)
            torch.cuda.synchronize()
            sms.append(stt['sweep_ms'])
            sweeps = int(stt['sweeps_max'])
        s_res = rp.residual()[1]
        Ss = rp.S
        rows.append({'xc': xc, 'yc': yc, 'members': nb, 'fourier_ms_median': round(fmed, 4), 'fourier_ms_min': round(fmin, 4),
                     'fourier_launch_section_ms': round(section, 4), 'sor_ms_median': round(float(np.median(sms)), 4),
                     'sor_sweeps': sweeps, 'speedup': round(float(np.median(sms)) / fmed, 1),
                     'fourier_resid': float((f_res[:, 2] / f_res[:, 3]).max()), 'sor_resid': float((s_res[:, 2] / s_res[:, 3]).max()),
                     'rel_l2_sor_vs_fourier': float((torch.linalg.norm(Ss - Sf) / torch.linalg.norm(Sf)).item()),
                     'overflow_members': ovf, 'kernels': kern})
        lines.append(json.dumps(rows[-1]))
        print(lines[-1], flush=True)
        rp.close()
        del rp, S, F, Sf, Ss
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    # the one condition
    r = rows[1]
    assert r['fourier_ms_median'] < r['sor_ms_median'], \
        "'fourier' is not faster than 'sor' at 3600 x 1800 x 1: %s ms against %s ms" % (r['fourier_ms_median'], r['sor_ms_median'])


if __name__ == '__main__':
    main()
