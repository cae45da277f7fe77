#!/usr/bin/env python3
"""Generate tests/golden/tridiag_cases.npz from the REFERENCE ITSELF.  Build container only.

Drives the reference's own numbas.trace / numbas.traceCyclic (numbas.py:1589-1685) and numbas.invert_standard_1D
(numbas.py:633-742), imported as plain Python through oracle/ref_import.py and not changed, and stores inputs + outputs
as numeric fixtures.  About half a minute.  Re-run:  python tests/golden/gen_golden_tridiag.py

`pin_*`    the inputs of the reference's tests/test_trace.py, its trace / traceCyclic outputs on them, and the answers
           that test prints (`pin_expect`, `pin_expect_cyc`).
`t<k>_*`   seeded diagonally dominant systems, n in 2, 3, 4, 63, 64, 65, 181, 501, 1000 (`tn` lists them): a, b, c, d, a0,
           cn, `x` = trace, `xc` = traceCyclic.
`c<k>_*`   converged 1-D cases (`names` lists them): invert_standard_1D run until flags[1] < 1e-12 on the masked matrix of
           gen_golden_1d.py at xc 5, 64, 65, 73 (BC fixed / extend / periodic x masks none / F / A / A[xc-1] / B) with
           B <= -0.1, so that 'periodic' and 'extend' are non-singular; an icbc start holding undef values; and periodic
           members with a masked end point (through F[0], F[xc-1], A[0], and both ends).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from oracle.ref_import import load_reference_numbas   # noqa: E402

UNDEF = -9.99e8
BCS = ['fixed', 'extend', 'periodic']
NS = [2, 3, 4, 63, 64, 65, 181, 501, 1000]
XCS = [5, 64, 65, 73]
MASKS = ['none', 'F', 'A', 'Alast', 'B']
SWEEPS = 4000


def coeffs(rng, xc):
    return rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, -0.1, xc), rng.standard_normal(xc), rng.standard_normal(xc) * 0.1


def converged_cases(rng):
    cases = []
    for BCx in BCS:
        for xc in XCS:
            for mk in MASKS:
                A, B, F, S0 = coeffs(rng, xc)
                pick = lambda: rng.choice(xc, max(1, xc // 5), replace=False)
                if mk == 'F':
                    F[pick()] = UNDEF
                elif mk == 'A':
                    A[pick()] = UNDEF
                elif mk == 'Alast':
                    A[xc - 1] = UNDEF
                elif mk == 'B':
                    B[pick()] = UNDEF
                cases.append(dict(name='%s_%d_%s' % (BCx, xc, mk), S0=S0, A=A, B=B, F=F, BCx=BCx, delxSqr=0.49))
        xc = 73
        A, B, F, S0 = coeffs(rng, xc)
        S0 = rng.standard_normal(xc)
        S0[[0, 5, 6, 40, xc - 1]] = UNDEF                     # icbc holding undef values
        F[[5, 6, 40]] = UNDEF
        cases.append(dict(name='%s_icbc' % BCx, S0=S0, A=A, B=B, F=F, BCx=BCx, delxSqr=1.0))
    for xc in (64, 65):                                       # periodic, an end point masked
        for tag in ('F0', 'Flast', 'A0', 'Fboth'):
            A, B, F, S0 = coeffs(rng, xc)
            if tag in ('F0', 'Fboth'):
                F[0] = UNDEF
            if tag in ('Flast', 'Fboth'):
                F[xc - 1] = UNDEF
            if tag == 'A0':
                A[0] = UNDEF
            cases.append(dict(name='periodic_%d_end_%s' % (xc, tag), S0=S0, A=A, B=B, F=F, BCx='periodic',
                              delxSqr=0.49))
    return cases


def main():
    nb = load_reference_numbas()
    rng = np.random.default_rng(20261017)
    out = {}
    # the reference's own test (tests/test_trace.py): inputs, and the answers it compares with np.isclose
    a, b, c, d = np.array([2., 2., 0.]), np.array([3., 3., 3., 3.]), np.array([0., 1., 1.]), np.array([5., 9., 9., 8.])
    out.update(pin_a=a, pin_b=b, pin_c=c, pin_d=d, pin_a0=np.array(5.2), pin_cn=np.array(3.9),
               pin_x=nb.trace(a, b, c, d), pin_xc=nb.traceCyclic(a, b, c, d, 5.2, 3.9),
               pin_expect=np.array([1.6666666666666667, 1.5238095238095233, 1.0952380952380958, 2.6666666666666665]),
               pin_expect_cyc=np.array([2.35815602836879370, 0.49316109422492393, 2.80420466058763960,
                                        -0.39893617021276560]))
    for k, n in enumerate(NS):
        a, c = rng.uniform(-1, 1, n - 1), rng.uniform(-1, 1, n - 1)
        b = rng.uniform(2.5, 4.0, n) * rng.choice([-1.0, 1.0], n)
        d = rng.standard_normal(n)
        a0, cn = rng.uniform(-1, 1), rng.uniform(-1, 1)
        p = 't%d_' % k
        out.update({p + 'a': a, p + 'b': b, p + 'c': c, p + 'd': d, p + 'a0': np.array(a0), p + 'cn': np.array(cn),
                    p + 'x': nb.trace(a, b, c, d), p + 'xc': nb.traceCyclic(a, b, c, d, a0, cn)})
    out['tn'] = np.array(NS)
    names = []
    t0 = time.time()
    for k, cs in enumerate(converged_cases(rng)):
        S = np.array(cs['S0'])
        fl = np.array([0.0, 1.0, 0.0])
        nb.invert_standard_1D(S, cs['A'], cs['B'], cs['F'], len(S), np.sqrt(cs['delxSqr']), cs['BCx'], cs['delxSqr'],
                              1.5, UNDEF, fl, SWEEPS, -1.0)
        if not (fl[0] == 0 and fl[1] < 1e-12):
            raise SystemExit('%s: not converged (flags %s)' % (cs['name'], fl))
        p = 'c%d_' % k
        for key in ('S0', 'A', 'B', 'F'):
            out[p + key] = cs[key]
        out[p + 'S'] = S
        out[p + 'par'] = np.array([BCS.index(cs['BCx']), cs['delxSqr']])
        names.append(cs['name'])
    print('converged: %d cases, %.1f s' % (len(names), time.time() - t0), flush=True)
    out['names'] = np.array(names)
    out['undef'] = np.array(UNDEF)
    np.savez_compressed(os.path.join(HERE, 'tridiag_cases.npz'), **out)
    print('wrote tridiag_cases.npz')


if __name__ == '__main__':
    main()
