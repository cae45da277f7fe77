#!/usr/bin/env python3
"""Generate tests/golden/resid_cases.npz from the REFERENCE ITSELF.  Build container only.

Pins tests/resid_model.py (the residual R = L(S) - F) to the reference's own kernels, imported as plain
Python through oracle/ref_import.py and not changed.  The reference has no residual; it has `S += temp * optArg / den`.
So, per case:
  * the points are split into classes such that no two points of a class lie in each other's stencil (rows / planes by
    parity; columns by parity, and with periodic x and odd xc the last column a class of its own: the wrap would put
    columns xc-1 and 0 into one parity class);
  * the forcing is set to undef outside one class, and the reference's kernel runs ONE sweep (mxLoop = 0) with optArg = 1
    from a random O(1) S: only the class's points move, and none of them reads another;
  * the reference's residual at those points is (S_out - S_in) * den / delxSqr, with den recomputed here from the inputs.
With 'extend' boundaries S first goes through the reference's own pre-pass (a run with an all-undef forcing), so that the
pre-pass of the class runs changes nothing.

The npz holds inputs and recorded results only: per case `c<k>_S`, `c<k>_<array letter>`, `c<k>_sc` (scalars, in the
order of `scalar_names`), `c<k>_ref` (the recovered residual, NaN where the reference changed nothing), `c<k>_changed`,
`c<k>_den`, `c<k>_Sout` (the value after the sweep, where changed); `names`, `kinds`, `bcs`.
Re-run:  python tests/golden/gen_golden_resid.py        (a few seconds)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from oracle.ref_import import load_reference_numbas   # noqa: E402

UNDEF = -9.99e8
ARRAYS = {'std2d': 'ABCF', 'gen2d': 'ABCDEFG', 'std2dt': 'ABCDEF', 'std3d': 'ABCF', 'gen3d': 'ABCDEFGH'}
SCALARS = ['delx', 'delxSqr', 'ratio', 'ratioQtr', 'ratioSqr', 'ratio2', 'ratio1', 'ratio2Sqr', 'ratio1Sqr']


def scalars(kind, rng):
    delx = float(rng.uniform(0.6, 1.4))
    sc = dict(delx=delx, delxSqr=delx * delx)
    if kind in ('std3d', 'gen3d'):
        r2, r1 = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))
        sc.update(ratio2=r2, ratio1=r1, ratio2Sqr=r2 * r2, ratio1Sqr=r1 * r1)
    else:
        r = float(rng.uniform(0.5, 2.0))
        sc.update(ratio=r, ratioQtr=r / 4.0, ratioSqr=r * r)
    return sc


def run_ref(nb, kind, S, arrs, sc, bcs):
    """One sweep of the reference's kernel (mxLoop = 0, optArg = 1) on a copy of S."""
    S = np.array(S, dtype=np.float64)
    fl = np.array([0.0, 1.0, 0.0])
    shp = S.shape
    if kind == 'std2d':
        nb.invert_standard_2D(S, *arrs, shp[0], shp[1], 1.0, sc['delx'], bcs[0], bcs[1], sc['delxSqr'], sc['ratioQtr'],
                              sc['ratioSqr'], 1.0, UNDEF, fl, 0, 1e-30)
    elif kind == 'std2dt':
        nb.invert_standard_2D_test(S, *arrs, shp[0], shp[1], 1.0, sc['delx'], bcs[0], bcs[1], sc['delxSqr'],
                                   sc['ratioQtr'], sc['ratioSqr'], 1.0, UNDEF, fl, 0, 1e-30)
    elif kind == 'gen2d':
        nb.invert_general_2D(S, *arrs, shp[0], shp[1], 1.0, sc['delx'], bcs[0], bcs[1], sc['delxSqr'], sc['ratio'],
                             sc['ratioQtr'], sc['ratioSqr'], 1.0, UNDEF, fl, 0, 1e-30)
    elif kind == 'std3d':
        nb.invert_standard_3D(S, *arrs, shp[0], shp[1], shp[2], 1.0, 1.0, sc['delx'], bcs[0], bcs[1], bcs[2],
                              sc['delxSqr'], sc['ratio2Sqr'], sc['ratio1Sqr'], 1.0, UNDEF, fl, 0, 1e-30)
    else:
        nb.invert_general_3D(S, *arrs, shp[0], shp[1], shp[2], 1.0, 1.0, sc['delx'], bcs[0], bcs[1], bcs[2],
                             sc['delxSqr'], sc['ratio2'], sc['ratio1'], sc['ratio2Sqr'], sc['ratio1Sqr'], 1.0, UNDEF, fl,
                             0, 1e-30)
    return S


def denominator(kind, arrs, sc):
    """The reference's `optArg / (...)` denominator at every point (x wrapped; garbage where it is not used)."""
    E1 = lambda a: np.roll(a, -1, axis=-1)
    with np.errstate(all='ignore'):
        if kind == 'std2d':
            A, B, C, F = arrs
            return (np.roll(A, -1, axis=0) + A) * sc['ratioSqr'] + (E1(C) + C)
        if kind == 'std2dt':
            A, B, C, D, E, F = arrs
            return (np.roll(A, -1, axis=0) + A) * sc['ratioSqr'] + (E1(D) + D) - E * sc['delxSqr']
        if kind == 'gen2d':
            A, B, C, D, E, F, G = arrs
            return (A * sc['ratioSqr'] + C) * 2.0 - F * sc['delxSqr']
        if kind == 'std3d':
            A, B, C, F = arrs
            return ((np.roll(A, -1, axis=0) + A) * sc['ratio2Sqr'] + (np.roll(B, -1, axis=1) + B) * sc['ratio1Sqr'] +
                    (E1(C) + C))
        A, B, C, D, E, F, G, H = arrs
        return (A * sc['ratio2Sqr'] + B * sc['ratio1Sqr'] + C) * 2.0 - G * sc['delxSqr']


def classes(shape, per):
    """Integer class of every point: no two points of a class within one step of each other in every direction."""
    xc = shape[-1]
    cx = np.arange(xc) % 2
    if per and xc % 2:
        cx[-1] = 2
    cls = np.broadcast_to(cx, shape).copy()
    mult = 3
    for ax in range(len(shape) - 2, -1, -1):
        cls = cls + mult * (np.arange(shape[ax]) % 2).reshape((-1,) + (1,) * (len(shape) - 1 - ax))
        mult *= 2
    return cls


def make_case(rng, name, kind, shape, bcs, zeroB, masks):
    sc = scalars(kind, rng)
    letters = ARRAYS[kind]
    arrs = []
    for q, a in enumerate(letters):
        forcing = q == len(letters) - 1
        if forcing:
            v = rng.standard_normal(shape)
        elif a in 'ABC' and not (kind in ('std2d', 'std2dt', 'gen2d') and a == 'B') and not (kind == 'std2dt' and a == 'C'):
            v = rng.uniform(0.6, 1.6, shape)                 # the second-derivative coefficients: positive
        else:
            v = rng.uniform(-0.4, 0.4, shape)
        arrs.append(v)
    if kind in ('std2dt',):
        arrs[4] = -np.abs(arrs[4])                           # E <= 0 keeps the denominator away from 0
    if kind == 'gen2d':
        arrs[5] = -np.abs(arrs[5])
    if kind == 'gen3d':
        arrs[6] = -np.abs(arrs[6])
    if zeroB and kind in ('std2d', 'gen2d', 'std2dt'):
        arrs[1] = np.zeros(shape)
        if kind == 'std2dt':
            arrs[2] = np.zeros(shape)
    for which in masks:                                      # a few undef values in that array
        a = arrs[letters.index(which)]
        idx = rng.choice(a.size, max(1, a.size // 9), replace=False)
        a.reshape(-1)[idx] = UNDEF
    per = bcs[-1] == 'periodic'
    S0 = rng.standard_normal(shape)
    cls = classes(shape, per)

    def only(cval):
        """The arrays with the forcing defined on class `cval` alone (None: nowhere).  The general 3-D form's west-periodic
        branch never tests H (numbas.py:849-852), so there column 0 is switched off through G, which it does test."""
        a = list(arrs[:-1]) + [np.where(cls == cval, arrs[-1], UNDEF) if cval is not None else np.full(shape, UNDEF)]
        if kind == 'gen3d' and per:
            G = a[6].copy()
            G[..., 0] = np.where(cls[..., 0] == cval, G[..., 0], UNDEF) if cval is not None else UNDEF
            a[6] = G
        return a

    S_in = run_ref(NB, kind, S0, only(None), sc, bcs)         # (only the 'extend' pre-pass can have changed it)
    den = denominator(kind, arrs, sc)
    ref = np.full(shape, np.nan)
    changed = np.zeros(shape, dtype=bool)
    Sout = np.full(shape, np.nan)
    for cval in np.unique(cls):
        S_out = run_ref(NB, kind, S_in, only(cval), sc, bcs)
        ch = S_out != S_in
        assert not (ch & (cls != cval)).any(), name
        with np.errstate(all='ignore'):
            rec = (S_out - S_in) * den / sc['delxSqr']
        ref[ch] = rec[ch]
        Sout[ch] = S_out[ch]
        changed |= ch
    return dict(name=name, kind=kind, bcs=bcs, S=S_in, arrs=arrs, sc=sc, ref=ref, changed=changed, den=den, Sout=Sout)


def main():
    global NB
    NB = load_reference_numbas()
    rng = np.random.default_rng(20251)
    cases = []
    for kind in ('std2d', 'gen2d', 'std2dt'):
        for bcs, shape in ((('fixed', 'fixed'), (5, 8)), (('extend', 'fixed'), (6, 9)), (('fixed', 'periodic'), (7, 9)),
                           (('extend', 'periodic'), (6, 8)), (('fixed', 'periodic'), (3, 5))):
            for zeroB in (False, True):
                for masks in ((), ('F',), ('A', 'F') if kind != 'gen2d' else ('C', 'G')):
                    if zeroB and masks:
                        continue
                    if kind == 'gen2d' and masks == ('F',):
                        masks = ('G',)
                    nm = '%s_%s_%s_%dx%d_%s_%s' % (kind, bcs[0], bcs[1], shape[0], shape[1], 'B0' if zeroB else 'B',
                                                   ''.join(masks) or 'nomask')
                    cases.append(make_case(rng, nm, kind, shape, list(bcs), zeroB, masks))
    for kind in ('std3d', 'gen3d'):
        last = 'F' if kind == 'std3d' else 'H'
        for bcs, shape in ((('fixed', 'fixed', 'fixed'), (4, 5, 7)), (('fixed', 'extend', 'periodic'), (4, 5, 7)),
                           (('fixed', 'fixed', 'periodic'), (3, 4, 6)), (('extend', 'extend', 'fixed'), (4, 5, 6))):
            for masks in ((), (last,), ('B', last)):
                nm = '%s_%s_%dx%dx%d_%s' % (kind, '_'.join(bcs), shape[0], shape[1], shape[2], ''.join(masks) or 'nomask')
                cases.append(make_case(rng, nm, kind, shape, list(bcs), False, masks))
    out = dict(names=np.array([c['name'] for c in cases]), kinds=np.array([c['kind'] for c in cases]),
               bcs=np.array(['/'.join(c['bcs']) for c in cases]), scalar_names=np.array(SCALARS))
    nlive = 0
    for k, c in enumerate(cases):
        out['c%d_S' % k] = c['S']
        for a, v in zip(ARRAYS[c['kind']], c['arrs']):
            out['c%d_%s' % (k, a)] = v
        out['c%d_sc' % k] = np.array([c['sc'].get(s, 0.0) for s in SCALARS])
        for f in ('ref', 'changed', 'den', 'Sout'):
            out['c%d_%s' % (k, f)] = c[f]
        nlive += int(c['changed'].sum())
    path = os.path.join(HERE, 'resid_cases.npz')
    np.savez_compressed(path, **out)
    print('%d cases, %d recovered residuals -> %s (%d bytes)' % (len(cases), nlive, path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
