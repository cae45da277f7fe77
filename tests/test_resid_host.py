"""The residual R = L(S) - F, host side: the numpy model (tests/resid_model.py) against residuals
recovered from the reference's own kernels (tests/golden/resid_cases.npz, written by tests/golden/gen_golden_resid.py), the
header / table / export bookkeeping, and the front end's state rebuild.  No GPU."""
import os
import re

import numpy as np
import pytest

import resid_model
from xinvert_amd import _lib, apps, forms
from xinvert_amd.field import Field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDEF = -9.99e8
ARRAYS = {k: forms.FORMS[k].arrays for k in forms.RESIDUAL}
U = 2.0 ** -53                                             # unit roundoff of float64


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'resid_cases.npz'))


def _case(g, k):
    kind = str(g['kinds'][k])
    arrs = [g['c%d_%s' % (k, a)] for a in ARRAYS[kind]]
    sc = dict(zip([str(s) for s in g['scalar_names']], g['c%d_sc' % k]))
    per = str(g['bcs'][k]).split('/')[-1] == 'periodic'
    return kind, g['c%d_S' % k], arrs, sc, per


def test_model_agrees_with_the_reference_kernels(golden):
    """Every point the reference moved: the model's residual equals the recovered one within the rounding of the recovery.
    The reference computes q = fl(1 / den), t = fl(temp * q), S_out = fl(S_in + t); the fixture holds
    rec = fl(fl(fl(S_out - S_in) * den) / delxSqr).  With u = 2^-53:
      * S_out = (S_in + t)(1 + e1) and the difference fl(S_out - S_in) (1 + e2): two roundings at the magnitude of S, each at
        most u * max(|S_in|, |S_out|) in t, i.e. times |den| / delxSqr in the residual;
      * q, t, the product with den and the division by delxSqr: four roundings relative to the residual itself, and the
        model's own final division a fifth: 5 u |R| (second-order terms are below one more u |R|: 6 u |R| in all).
    The bound is derived, not tuned; the figures are printed before the assertion."""
    g = golden
    worst = 0.0
    kinds = set()
    for k in range(len(g['names'])):
        kind, S, arrs, sc, per = _case(g, k)
        kinds.add((kind, str(g['bcs'][k])))
        R, live = resid_model.residual(kind, S, arrs, sc, per, UNDEF)
        ch = g['c%d_changed' % k]
        assert np.array_equal(live, ch), g['names'][k]                   # undef placement == what the reference changed
        assert np.array_equal(R == UNDEF, ~ch), g['names'][k]
        ref, den, Sout = g['c%d_ref' % k][ch], g['c%d_den' % k][ch], g['c%d_Sout' % k][ch]
        smag = np.maximum(np.abs(S[ch]), np.abs(Sout))
        bound = 2 * U * smag * np.abs(den) / sc['delxSqr'] + 6 * U * np.abs(R[ch])
        err = np.abs(R[ch] - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (g['names'][k], float((err / bound).max()))
    print('largest error / bound over %d cases: %.3f' % (len(g['names']), worst))
    # the fixture covers every form under fixed / extend / periodic
    for kind in forms.RESIDUAL:
        bcs = '/'.join(b for kk, b in kinds if kk == kind)
        assert 'fixed' in bcs and 'extend' in bcs and 'periodic' in bcs, kind


def test_fixture_covers_zero_and_nonzero_B_and_masks(golden):
    g = golden
    names = [str(n) for n in g['names']]
    for kind in ('std2d', 'gen2d', 'std2dt'):
        assert any(n.startswith(kind + '_') and '_B0_' in n for n in names)
        assert any(n.startswith(kind + '_') and '_B_' in n for n in names)
    for k, n in enumerate(names):
        kind = str(g['kinds'][k])
        assert g['c%d_S' % k].size <= 4 * 5 * 7
        if '_B0_' in n:
            assert not g['c%d_B' % k].any()
            # B identically zero: the 5-point expression (B = None) gives the same residual up to the sign of a zero
            _, S, arrs, sc, per = _case(g, k)
            R9, l9 = resid_model.residual(kind, S, arrs, sc, per, UNDEF)
            if kind != 'std2dt':
                R5, l5 = resid_model.residual(kind, S, [arrs[0], None] + arrs[2:], sc, per, UNDEF)
                assert np.array_equal(l5, l9) and np.array_equal(R5, R9)
    assert any(n.endswith('nomask') for n in names) and any(not n.endswith('nomask') for n in names)


def test_norms_of_the_model():
    R = np.array([[UNDEF, 1.0, -3.0], [2.0, UNDEF, 0.5]])
    live = R != UNDEF
    F = np.array([[9.0, -7.0, 1.0], [2.0, 100.0, 0.0]])
    assert np.array_equal(resid_model.norms(R, F, live), [4.0, 6.5 / 4, 3.0, 7.0])
    n0 = resid_model.norms(R, F, np.zeros_like(live))
    assert n0[0] == 0 and np.isnan(n0[1]) and n0[2] == 0 and n0[3] == 0
    R[0, 1] = np.nan
    nn = resid_model.norms(R, F, live)
    assert nn[0] == 4 and np.isnan(nn[1]) and np.isnan(nn[2]) and nn[3] == 7.0


def _prototypes(path):
    """[(name, [(C type, parameter name)])] of every `int xinv_...(...);`, in file order (as tests/test_host.py parses xinv.h)."""
    hdr = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    out = []
    for name, plist in re.findall(r'\bint\s+(xinv_\w+)\s*\(([^)]*)\)\s*;', hdr):
        ps = []
        for par in plist.split(','):
            m = re.fullmatch(r'\s*(.*?)(\w+)\s*', par, flags=re.S)
            ps.append((' '.join(m.group(1).replace('*', ' * ').split()).replace('* *', '**'), m.group(2)))
        out.append((name, ps))
    return out


def test_residual_header_matches_the_forms_table():
    import ctypes
    protos = _prototypes(os.path.join(ROOT, 'include', 'xinv_resid.h'))
    want = [forms.symbol(k, e) for k in forms.RESIDUAL for e in ('resid_dev', 'resid_batched')]
    assert [n for n, _ in protos] == want                             # one prototype per entry, same names, same order
    dp = ctypes.POINTER(ctypes.c_double)
    ctype_of = {'double *': (dp, ctypes.c_void_p), 'const double *': (dp, ctypes.c_void_p),
                'int64_t': (ctypes.c_int64,), 'double': (ctypes.c_double,), 'int': (ctypes.c_int,),
                'const int64_t *': (ctypes.POINTER(ctypes.c_int64),),
                'const xinv_options *': (ctypes.POINTER(_lib.XinvOptions),), 'void *': (ctypes.c_void_p,)}
    by_name = dict(protos)
    for k in forms.RESIDUAL:
        for e in ('resid_dev', 'resid_batched'):
            name = forms.symbol(k, e)
            ps = forms.params(k, e)
            assert [n for _, n in by_name[name]] == [n for n, _ in ps], name
            for (ctype, pname), (_, t) in zip(by_name[name], ps):
                assert t in ctype_of[ctype], (name, pname)
            # the solve entry's arguments, behind R and S, up to undef
            solve = [n for n, _ in forms.params(k, 'dev' if e == 'resid_dev' else 'batched')]
            mine = [n for n, _ in ps]
            assert mine[0] == 'R' and mine[1:mine.index('undef') + 1] == solve[:solve.index('undef') + 1]
            assert mine[mine.index('undef') + 1:] == ['norms', 'stream' if e == 'resid_dev' else 'opt']
    for k in ('bih2d', 'std1d'):
        with pytest.raises(KeyError):
            forms.symbol(k, 'resid_dev')
    # xinv.h itself declares none of them (its prototype count is pinned), names all of them, and includes the header
    main = open(os.path.join(ROOT, 'include', 'xinv.h')).read()
    assert '#include "xinv_resid.h"' in main
    stripped = re.sub(r'/\*.*?\*/', ' ', main, flags=re.S)
    for name in want:
        assert re.search(r'\b%s\s*\(' % name, main) and name not in stripped


def test_library_exports_the_residual_symbols():
    L = _lib.load()
    for k in forms.RESIDUAL:
        for e in ('resid_dev', 'resid_batched'):
            name = forms.symbol(k, e)
            assert name in _lib.EXPORTS
            fn = getattr(L, name)
            assert fn.argtypes == forms.argtypes(k, e)


def test_solver_state_rebuild():
    """apps.residual works on the state the solver left: where the forcing is undefined, the value _mask_FS put there (zero,
    or icbc) instead of the de-mask fill the user's S holds."""
    lat, lon = np.linspace(-30, 30, 5), np.linspace(0, 70, 8)
    F = np.arange(40, dtype=np.float64).reshape(5, 8) + 1.0
    F[1, 2] = np.nan; F[3, 5] = np.nan
    Ff = Field(F, ('lat', 'lon'), {'lat': lat, 'lon': lon})
    ip = {'undef': np.nan, 'BCs': ['fixed', 'fixed']}
    maskF, initS, _ = apps._mask_FS(Ff, ['lat', 'lon'], ip, None)
    S_user = np.where(np.isnan(F), np.nan, 7.0)                       # de-masked with iParams['undef']
    st = apps._solver_state(S_user, maskF.values, initS.values)
    assert st[1, 2] == 0.0 and st[3, 5] == 0.0 and (st[~np.isnan(F)] == 7.0).all() and not np.isnan(st).any()
    ic = Field(np.full((5, 8), 3.5), ('lat', 'lon'), {'lat': lat, 'lon': lon})
    maskF, initS, _ = apps._mask_FS(Ff, ['lat', 'lon'], ip, ic)
    S_user = np.where(np.isnan(F), 3.5, 7.0)                          # (with icbc nothing is de-masked)
    st = apps._solver_state(S_user, maskF.values, initS.values)
    assert st[1, 2] == 3.5 and st[3, 5] == 3.5 and st[2, 2] == 7.0
    # the residual's own de-mask
    R = Field(np.array([[UNDEF, 1.0], [2.0, UNDEF]]), ('y', 'x'))
    out = apps._demask_residual(R, {'undef': np.nan}).values
    assert np.isnan(out[0, 0]) and np.isnan(out[1, 1]) and out[0, 1] == 1.0 and out[1, 0] == 2.0


def test_residual_raises_for_the_forms_it_does_not_cover():
    lat, lon = np.linspace(-30, 30, 9), np.linspace(0, 70, 12)
    F = Field(np.ones((9, 12)), ('lat', 'lon'), {'lat': lat, 'lon': lon})
    for name in ('StommelMunk', 'GeoAdjustment', 'RefStateSWM', 'nonsense'):
        with pytest.raises(Exception, match='unsupported problem'):
            apps.residual(name, F, F, ['lat', 'lon'], iParams={'printInfo': False})
    assert set(apps._RESIDUAL) >= {'poisson', 'omega', '3docean', 'fofonoff', 'stommel', 'gillmatsuno_test'}
    assert all(apps._res_func(getattr(apps.core, v[1])) is not None for v in apps._RESIDUAL.values())
    with pytest.raises(Exception, match="iParams\\['residual'\\]"):
        apps.invert_StommelMunk(F, ['lat', 'lon'], iParams={'printInfo': False, 'residual': True},
                                mParams={'A4': 1e3, 'D': 100.0})
