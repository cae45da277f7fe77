#!/usr/bin/env python3
"""The direct Fourier solve of the 2-D general form (k_fourier_gcheck, k_fourier_cfactor, k_fourier_csubst around k_rowdft)
against a resident SOR solve of the same problem on one GPU.

Gill-Matsuno problems (synthetic.gill_matsuno: six shared coefficient arrays that depend on latitude alone) at 73 x 144 x 3,
720 x 1440 x 8 and 720 x 1440 x 64, float64, device-resident.  'cfourier': HIP events around
xinv_fourier_general_2d_f64_dev (the whole entry: check pass and its read-back, factors, transforms, substitution, the
flags' read-back), median of `--reps` calls after warm-up, S reset before every call.  'sor': ResidentProblem.solve at
tolerance 1e-10 (xinv_stats.sweep_ms), median of `--sor-reps`.  Both fields go through ResidentProblem.residual(), the
general form's residual kernel: max|R| / max|F|.  Per new kernel: the bytes it must move, its device time (the sum of its
launches in one call, median over calls, from torch.profiler's kernel records) and its rate against a device copy of the
same bytes timed here with events.  Where the profiler gives no kernel records the three are reported together, as what is
left of the entry after the transforms.  Writes profiles/fourier_general_bench.txt, then asserts the one condition:
'cfourier' is faster than 'sor' at 720 x 1440 x 8.

  python tools/bench_fourier_general.py [--reps N] [--sor-reps N] [--out FILE]
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
KERNELS = ('k_fourier_gcheck', 'k_fourier_cfactor', 'k_fourier_csubst')


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


def kernel_ms(fn, reps):
    """{kernel: median over `reps` calls of the summed device time (ms) of its launches in one call}, or {} when the
    profiler records no kernel of ours."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    per = {k: [] for k in KERNELS}
    try:
        for _ in range(reps):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            tot = {k: 0.0 for k in KERNELS}
            for ev in prof.events():
                for k in KERNELS:
                    if k in ev.name:
                        tot[k] += float(getattr(ev, 'device_time', 0.0) or getattr(ev, 'cuda_time', 0.0)) / 1e3
            for k in KERNELS:
                per[k].append(tot[k])
    except Exception as e:                                   # (the figures then come from the events alone, and say so)
        print('# torch.profiler: %s' % e, flush=True)
        return {}
    out = {k: float(np.median(v)) for k, v in per.items()}
    return out if all(v > 0 for v in out.values()) else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sor-reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fourier_general_bench.txt'))
    args = ap.parse_args()
    import torch
    L = _lib.require_gpu()
    lines = ['== python tools/bench_fourier_general.py --reps %d --sor-reps %d (Gill-Matsuno, shared coefficients, float64, device-resident)'
             % (args.reps, args.sor_reps),
             '# cfourier_ms: HIP events around xinv_fourier_general_2d_f64_dev; sor_ms: xinv_stats.sweep_ms at tolerance 1e-10',
             '# resid: max|R| / max|F| by ResidentProblem.residual(); kernels: must-move bytes, ms, and the time of a device copy of the same bytes over it']
    rows = []
    for yc, xc, nb in ((73, 144, 3), (720, 1440, 8), (720, 1440, 64)):
        p = synthetic.gill_matsuno(yc, xc, nb)
        rp = ResidentProblem(p, device=0)
        K, n = xc // 2 + 1, yc * xc
        cs = [torch.from_numpy(np.array(np.broadcast_to(np.asarray(p['coefs'][q], dtype=np.float64), (yc, xc))[:, 0])).cuda()
              for q in (0, 2, 3, 4, 5)]
        G, S = rp.coefs[6], rp.S
        fl = np.zeros((nb, 3))
        st = torch.cuda.current_stream().cuda_stream

        def cfourier():
            S.copy_(rp.S0)
            _lib.check(L.xinv_fourier_general_2d_f64_dev(S.data_ptr(), *[c.data_ptr() for c in cs], G.data_ptr(), nb,
                                                         _lib.strides_arg([n, 0, 0, 0, 0, 0, n]), yc, xc, p['delx'], p['delxSqr'],
                                                         p['ratio'], p['ratioSqr'], UNDEF, _lib.hptr(fl), st))
        reset_ms = timed(lambda: S.copy_(rp.S0), args.reps, 3)[0]
        fmed, fmin = timed(cfourier, args.reps, 3)
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
        nset = 1
        must = {'k_fourier_gcheck': nb * yc * xc * 8 + nset * 5 * (yc - 2) * 8,      # G rows 1 .. yc-2, S rows 0, yc-1; the coefficients
                'k_fourier_cfactor': nset * (yc - 2) * (K * 32 + 7 * 8),              # inv, gamma out; five coefficients in, lo, up out
                'k_fourier_csubst': nb * (yc - 2) * K * (16 * 2 + 16 * 2) + nb * 2 * K * 16 + nset * (yc - 2) * K * 32}
        # (csubst: the right-hand side in and rho out, rho in and the solution out, the two known rows; the factors once per set)
        kms = kernel_ms(cfourier, min(args.reps, 5))
        kern = {}
        if kms:
            for name in KERNELS:
                b, ms = must[name], kms[name]
                kern[name] = {'must_move_bytes': int(b), 'ms': round(ms, 4), 'TBps': round(b / ms / 1e9, 3),
                              'copy_ms_over_ms': round(copy_ms(b, args.reps) / ms, 3)}
        else:
            b = sum(must.values())
            ms = max(fmed - fwd * (1 + 2.0 / (yc - 2)) - inv, 1e-6)      # (two host round trips included: a lower bound of the rate)
            kern['gcheck+cfactor+csubst (events, transforms subtracted)'] = {
                'must_move_bytes': int(b), 'ms': round(ms, 4), 'TBps': round(b / ms / 1e9, 3),
                'copy_ms_over_ms': round(copy_ms(b, args.reps) / ms, 3)}
        kern['k_rowdft_forward'] = {'ms': round(fwd, 4)}
        kern['k_rowdft_inverse'] = {'ms': round(inv, 4)}
        # the sweeps
        sms, sweeps, sovf = [], 0, 0
        for _ in range(args.sor_reps):
            rp.reset()
            sfl, stt = rp.solve(200000, 1e-10, timing=1)
            torch.cuda.synchronize()
            sms.append(stt['sweep_ms'])
            sweeps = int(stt['sweeps_max'])
            sovf = int(np.asarray(sfl)[:, 0].sum())
        s_res = rp.residual()[1]
        Ss = rp.S
        rows.append({'yc': yc, 'xc': xc, 'members': nb, 'cfourier_ms_median': round(fmed, 4), 'cfourier_ms_min': round(fmin, 4),
                     'cfourier_launch_section_ms': round(section, 4), 'sor_ms_median': round(float(np.median(sms)), 4),
                     'sor_sweeps': sweeps, 'sor_overflow_members': sovf, 'speedup': round(float(np.median(sms)) / fmed, 1),
                     'cfourier_resid': float((f_res[:, 2] / f_res[:, 3]).max()), 'sor_resid': float((s_res[:, 2] / s_res[:, 3]).max()),
                     'rel_l2_sor_vs_cfourier': float((torch.linalg.norm(Ss - Sf) / torch.linalg.norm(Sf)).item()),
                     'overflow_members': ovf, 'workspace_bytes': int((16 * nb + 32 * nset) * yc * K + nset * 16 * yc),
                     'kernels': kern})
        lines.append(json.dumps(rows[-1]))
        print(lines[-1], flush=True)
        rp.close()
        del rp, S, G, Sf, Ss
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    # the one condition
    r = rows[1]
    assert r['cfourier_ms_median'] < r['sor_ms_median'], \
        "'cfourier' is not faster than 'sor' at 720 x 1440 x 8: %s ms against %s ms" % (r['cfourier_ms_median'], r['sor_ms_median'])


if __name__ == '__main__':
    main()
