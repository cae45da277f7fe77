#!/usr/bin/env python3
"""Generate tests/golden/std1d_cases.npz from the REFERENCE ITSELF.  Build container only.

Drives the reference's own numbas.invert_standard_1D (numbas.py:633-742, imported as plain Python through
oracle/ref_import.py, not changed) on seeded inputs and stores inputs + outputs as numeric fixtures.  About two minutes,
most of it the converged GeoAdjustment case.  Re-run:  python tests/golden/gen_golden_1d.py

Case matrix (`c<k>_*` arrays; `names` lists them): BC fixed / extend / periodic x xc 3, 4, 5, 64, 65, 73, 181, 501 x
masks none / undef in F / in A / in A[xc-1] only (masks point xc-2 through its A[i+1]) / in B; plus a NaN coefficient
(overflow), an all-zero forcing (norm == 0 stop at loop 0), an icbc start holding undef values, and tolerance stops.
Fixed sweep counts use tolerance <= 0, which never stops early.

Converged lexicographic solutions (`geo_*`, `swm_*`): the reference's GeoAdjustment case (its tests/test_GeoAdjustment.py:
yc 501, step h0 1500 / 1520, 'extend', optArg 1.8, tolerance -1e-11, mxLoop 100000) and a synthetic RefStateSWM case, with
the coefficients transcribed below from the reference's apps.py (citations at each formula).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from oracle.ref_import import load_reference_numbas   # noqa: E402

UNDEF = -9.99e8                  # the reference's _undeftmp (core.py:15)
BCS = ['fixed', 'extend', 'periodic']
XCS = [3, 4, 5, 64, 65, 73, 181, 501]
MASKS = ['none', 'F', 'A', 'Alast', 'B']
R_EARTH, OMEGA, G = 6371200.0, 7.292e-5, 9.80665     # reference apps.py default_mParams


def run_ref(nb, S, A, B, F, BCx, delxSqr, optArg, mxLoop, tol):
    S = np.array(S, dtype=np.float64)
    fl = np.array([0.0, 1.0, 0.0])
    nb.invert_standard_1D(S, A, B, F, len(S), np.sqrt(delxSqr), BCx, delxSqr, optArg, UNDEF, fl, mxLoop, tol)
    return S, fl


def matrix_cases(rng):
    cases = []
    for BCx in BCS:
        for xc in XCS:
            for mk in MASKS:
                A = rng.uniform(0.5, 1.5, xc)
                B = rng.uniform(-0.5, 0.0, xc)
                F = rng.standard_normal(xc)
                S0 = rng.standard_normal(xc) * 0.1
                if mk == 'F':
                    F[rng.choice(xc, max(1, xc // 5), replace=False)] = UNDEF
                elif mk == 'A':
                    A[rng.choice(xc, max(1, xc // 5), replace=False)] = UNDEF
                elif mk == 'Alast':
                    A[xc - 1] = UNDEF
                elif mk == 'B':
                    B[rng.choice(xc, max(1, xc // 5), replace=False)] = UNDEF
                mx = 60 if xc < 200 else 30
                cases.append(dict(name='%s_%d_%s' % (BCx, xc, mk), S0=S0, A=A, B=B, F=F, BCx=BCx,
                                  delxSqr=0.49, optArg=1.5, mxLoop=mx, tol=-1.0))
    for BCx in BCS:
        for xc in (65, 181):                      # tolerance stops inside the sweep budget
            A = rng.uniform(0.5, 1.5, xc); B = rng.uniform(-0.5, -0.1, xc); F = rng.standard_normal(xc)
            cases.append(dict(name='%s_%d_tol' % (BCx, xc), S0=np.zeros(xc), A=A, B=B, F=F, BCx=BCx,
                              delxSqr=1.0, optArg=1.7, mxLoop=5000, tol=1e-6))
        xc = 73
        A = rng.uniform(0.5, 1.5, xc); B = rng.uniform(-0.5, 0.0, xc); F = rng.standard_normal(xc)
        A2 = A.copy(); A2[30] = np.nan                   # a NaN coefficient passes the predicate: overflow
        cases.append(dict(name='%s_nan' % BCx, S0=np.zeros(xc), A=A2, B=B, F=F, BCx=BCx, delxSqr=1.0,
                          optArg=1.5, mxLoop=50, tol=-1.0))
        cases.append(dict(name='%s_zero' % BCx, S0=np.zeros(xc), A=A, B=B, F=np.zeros(xc), BCx=BCx,
                          delxSqr=1.0, optArg=1.5, mxLoop=50, tol=-1.0))
        S0 = rng.standard_normal(xc); S0[[0, 5, 6, 40, xc - 1]] = UNDEF   # icbc holding undef values
        F2 = F.copy(); F2[[5, 6, 40]] = UNDEF
        cases.append(dict(name='%s_icbc' % BCx, S0=S0, A=A, B=B, F=F2, BCx=BCx, delxSqr=1.0,
                          optArg=1.5, mxLoop=50, tol=-1.0))
    return cases


def geo_inputs():
    """The reference's GeoAdjustment case (tests/test_GeoAdjustment.py) through apps.__coeffs_GeoAdjustment
    (apps.py:1527-1553) and __cal_params1D (apps.py:2316-2358)."""
    yc = 501
    lat = np.linspace(-75, -25, yc)
    h0 = lat - lat + 1500
    h0[int(yc / 2):] = 1520
    lats = np.deg2rad(lat)
    sh = np.concatenate([[np.nan], lats[:-1]])               # lats.shift({dim: 1}): NaN first
    cosG = np.cos(lats)
    cosH = np.cos((lats + sh) / 2.0)
    f = 2 * OMEGA * np.sin(lats)
    fH = 2 * OMEGA * np.sin((lats + sh) / 2.0)
    zero = h0 - h0
    A = zero + cosH / fH                                      # apps.py:1544
    B = zero - f * cosG / G / h0                              # apps.py:1545 (divides by the raw h0)
    F = zero - f * cosG / G                                   # apps.py:1546
    del1 = np.deg2rad(np.diff(lat)[0]) * R_EARTH
    return dict(lat=lat, h0=h0, A=A, B=B, F=F, delxSqr=del1 ** 2.0, optArg=1.8, BCx='extend',
                mxLoop=100000, tol=-1e-11)


def swm_inputs():
    """A synthetic RefStateSWM case through apps.__coeffs_RefStateSWM (apps.py:1470-1524)."""
    yc = 161
    lat = np.linspace(5, 85, yc)
    lats = np.deg2rad(lat)
    Q = 1e-8 * (1.0 + np.sin(lats))
    M0 = 1e14 * np.cos(lats)
    C0 = 1e9 * np.cos(lats) ** 2
    sh = np.concatenate([[np.nan], lats[:-1]])
    cosG = np.cos(lats)
    cosH = np.cos((lats + sh) / 2.0)                          # apps.py:1497
    sinG = np.sin(lats)
    asin = R_EARTH * sinG
    acos = R_EARTH * cosG
    acos = np.where(acos < 0, -acos * 0.1, acos)              # apps.py:1502
    delY = np.abs(lats[0] - lats[1]) * R_EARTH
    diff = np.zeros_like(M0)                                  # diff_2nd, apps.py:1483-1493
    for j in range(1, yc - 1):
        diff[j] = (((M0[j + 1] - M0[j]) / cosH[j + 1]) - ((M0[j] - M0[j - 1]) / cosH[j])) / (delY ** 2)
    zero = Q - Q
    A = zero + 1.0 / cosH                                     # apps.py:1512
    B = zero - C0 * Q * asin / (np.pi * G * acos ** 3.0)      # apps.py:1513
    F = zero - (asin * C0 ** 2.0 / (2.0 * np.pi * G * acos ** 3.0)) + \
        (2.0 * np.pi * OMEGA ** 2.0 * asin * acos) / G - diff  # apps.py:1514-1515
    del1 = np.deg2rad(np.diff(lat)[0]) * R_EARTH
    eps = np.sin(np.pi / (2.0 * yc + 2.0)) ** 2
    optArg = 2.0 / (1.0 + np.sqrt((2.0 - eps) * eps))
    return dict(lat=lat, Q=Q, M0=M0, C0=C0, A=A, B=B, F=F, delxSqr=del1 ** 2.0, optArg=optArg, BCx='fixed',
                mxLoop=20000, tol=-1.0)


def main():
    nb = load_reference_numbas()
    rng = np.random.default_rng(20261015)
    out = {}
    names = []
    t0 = time.time()
    for k, c in enumerate(matrix_cases(rng)):
        S, fl = run_ref(nb, c['S0'], c['A'], c['B'], c['F'], c['BCx'], c['delxSqr'], c['optArg'], c['mxLoop'], c['tol'])
        p = 'c%d_' % k
        for key in ('S0', 'A', 'B', 'F'):
            out[p + key] = c[key]
        out[p + 'S'], out[p + 'flags'] = S, fl
        out[p + 'par'] = np.array([BCS.index(c['BCx']), c['delxSqr'], c['optArg'], c['mxLoop'], c['tol']])
        names.append(c['name'])
    print('matrix: %d cases, %.1f s' % (len(names), time.time() - t0), flush=True)
    out['names'] = np.array(names)
    out['undef'] = np.array(UNDEF)
    for tag, inp in (('swm', swm_inputs()), ('geo', geo_inputs())):
        t0 = time.time()
        S, fl = run_ref(nb, np.zeros(len(inp['lat'])), inp['A'], inp['B'], inp['F'], inp['BCx'], inp['delxSqr'],
                        inp['optArg'], inp['mxLoop'], inp['tol'])
        print('%s: flags %s, %.1f s' % (tag, fl, time.time() - t0), flush=True)
        if not (fl[0] == 0 and fl[1] < 1e-12):
            raise SystemExit('%s: not converged (flags %s)' % (tag, fl))
        for key, v in inp.items():
            out['%s_%s' % (tag, key)] = np.asarray(v)
        out[tag + '_S'], out[tag + '_flags'] = S, fl
    np.savez_compressed(os.path.join(HERE, 'std1d_cases.npz'), **out)
    print('wrote std1d_cases.npz')


if __name__ == '__main__':
    main()
