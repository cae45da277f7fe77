"""Manufactured solutions on the GPU (the table and the bounds: tests/mms_cases.py, tests/test_mms_host.py).

Residuals: apps.residual on the manufactured S for every table row at the table's three grids -- k_resid2d / k_resid3d, the
front end's masking / scaling and the row-constant upload on real builder output -- must shrink by 4 per refinement.
Solves: one per kernel family, on two grids, the error against the manufactured S shrinking by 4 while the returned max|R|
stays below 1 % of the truncation residual of S itself, so that iteration error cannot pose as discretisation error."""
import functools

import numpy as np
import pytest

import mms_cases as M
import util
from xinvert_amd import _lib, apps, multigrid

pytestmark = pytest.mark.gpu

ids = lambda k: '/'.join(k)
INVERT = {n[len('invert_'):].lower(): getattr(apps, n) for n in dir(apps) if n.startswith('invert_')}
SWEEPS = dict(mxLoop=60000, tolerance=1e-14)


def _ratios(es):
    return [es[i] / es[i + 1] for i in range(len(es) - 1)]


def _assert_order(es, what):
    r = _ratios(es)
    print(what, 'e =', ' '.join('%.3e' % e for e in es), 'ratios =', ' '.join('%.2f' % v for v in r))
    assert r[-1] >= M.LAST, (what, r)
    assert r[0] >= (M.FIRST if len(r) > 1 else M.LAST), (what, r)


def _truncation(case, p):
    """[n_live, mean|R|, max|R|, max|F|] of the manufactured S on the GPU."""
    ip = dict(p['iParams'])
    apps.residual(case.app, p['icbc'], p['F'], list(case.dims), case.coords, p['icbc'], p['mParams'], ip)
    return np.asarray(ip['resid'])[0]


# ------------------------------------------------------------------------------------------------ residuals
@pytest.mark.parametrize('key', sorted(M.RESIDUAL_CASES), ids=ids)
def test_residual_of_the_manufactured_solution(key):
    case = M.CASES[key]
    es = []
    for n in M.GRIDS:
        p = M.problem(case, n)
        nm = _truncation(case, p)
        assert nm[0] == p['live_expected'], (key, n)
        es.append(nm[2] / nm[3])
    _assert_order(es, ids(key))


@pytest.mark.parametrize('kind', sorted(M.MASKED))
def test_residual_with_a_masked_block(kind):
    key, how = M.MASKED[kind]
    case = M.CASES[key]
    es = []
    for n in M.GRIDS:
        p = M.problem(case, n, mask=how)
        nm = _truncation(case, p)
        assert nm[0] == p['live_expected'], (key, n)
        es.append(nm[2] / nm[3])
    _assert_order(es, ids(key) + ' masked:' + how)


# ------------------------------------------------------------------------------------------------ solves
def _solve(case, n, extra=None, mask=None):
    """-> (E, stats, returned max|R| or None, truncation max|R| or None, S, p)."""
    p = M.problem(case, n, mask=mask)
    resid = case.app in apps._RESIDUAL
    ip = dict(p['iParams'], **SWEEPS)
    ip.update(extra or {})
    if resid:
        ip['residual'] = True
    S = INVERT[case.app](p['F'], list(case.dims), case.coords, p['icbc'], p['mParams'], ip)
    live = p['live']
    E = np.abs(S.values - p['S'])[live].max() / np.abs(p['S'][live]).max()
    ret = trunc = None
    if resid:
        ret = float(np.asarray(S.iParams['resid'])[0][2])
        trunc = float(_truncation(case, p)[2])
    return E, S.iParams['stats'], ret, trunc, S.values, p


def _solve_family(key, grids, check, extra=None):
    case = M.CASES[key]
    Es = []
    for n in grids:
        E, st, ret, trunc, _, _ = _solve(case, n, extra)
        check(st)
        print(ids(key), n, 'E %.3e' % E, 'returned max|R| %r' % ret, 'truncation max|R| %r' % trunc)
        if ret is not None:
            assert ret <= 0.01 * trunc, (key, n, ret, trunc)
        Es.append(E)
    _assert_order(Es, ids(key))


G2, G3 = (32, 64), (16, 32)                                   # 33 x 64 -> 65 x 128; 9 x 17 x 32 -> 17 x 33 x 64


def test_solve_pipe2d_standard_form_latlon_poisson():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['pipelined'] == 1, st
    _solve_family(('poisson', 'lat-lon'), G2, check)


def test_solve_fourier_latlon_poisson():
    def check(st):
        assert st['path'] == _lib.PATH_FOURIER2D, st
    _solve_family(('poisson', 'lat-lon'), G2, check, extra={'method': 'fourier'})


def test_solve_pipe2d_general_form_latlon_gill_matsuno():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['pipelined'] == 1 and st['xuniform_mask'] == 0x1f, st
    _solve_family(('gillmatsuno', 'lat-lon'), G2, check)


def test_solve_general_form_full_coefficient_arrays_stommel_with_a_friction_field():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['pipelined'] == 0 and st['xuniform_mask'] != 0x1f, st
    _solve_family(('stommel', 'cartesian', 'Rfield'), G2, check)


def test_solve_nine_point_standard_form_eliassen():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['colours'] == 4, st
    _solve_family(('eliassen', 'z-lat'), G2, check)


def test_solve_standard_test_form_cartesian_fofonoff():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['xuniform_mask'] == 7 and st['pipelined'] == 0, st
    _solve_family(('fofonoff', 'cartesian'), G2, check)


def test_solve_pipe3d_standard_form_latlon_omega():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['sweeps_per_launch'] == 2 and st['xuniform_mask'] == 7, st
    _solve_family(('omega', 'lat-lon'), G3, check)


def test_solve_general_3d_form_ocean():
    def check(st):
        assert st['path'] == _lib.PATH_FUSED and st['xuniform_mask'] == 0x7f, st
    _solve_family(('3docean', 'lat-lon'), G3, check)


@functools.lru_cache(maxsize=None)
def _oracle_solution(key, n, mask):
    case = M.CASES[key]
    p = M.problem(case, n, mask=mask)
    q, _ = M.oracle_problem(case, p)
    S, fl = util.run_oracle(q, 400000, 1e-13, 0)
    assert fl[2] < 400000
    S.setflags(write=False)
    return S


@pytest.mark.parametrize('coords,mask', [('lat-lon', None), ('cartesian', None), M.MASKED_SOLVE['bih2d'][0][1:] + M.MASKED_SOLVE['bih2d'][1:]])
def test_solve_biharmonic_one_pass_kernel_stommel_munk(coords, mask):
    """17 x 48 -> 33 x 96 (periodic x: the one-pass kernel takes xc % 3 == 0) and 17 x 33 -> 33 x 65: the sweep count of the
    biharmonic form grows with the fourth power of the size, so its grids stay one step below the second-order forms'.
    It has no residual: iteration error is held against the converged oracle (reference ordering) instead -- at most 1 %
    of the discretisation error.  The masked variant puts an undefined block inside the domain."""
    key = ('stommelmunk', coords)
    case = M.CASES[key]
    Es = []
    for n in (16, 32):
        E, st, _, _, S, p = _solve(case, n, extra=dict(mxLoop=400000, tolerance=1e-13), mask=mask)
        assert st['path'] == _lib.PATH_FUSED and st['colours'] == 9, st
        live = p['live']
        assert np.abs(S - _oracle_solution(key, n, mask))[live].max() <= 0.01 * np.abs(S - p['S'])[live].max(), (key, n)
        Es.append(E)
    _assert_order(Es, ids(key) + (' masked:' + mask if mask else ''))


@pytest.mark.parametrize('app', ['geoadjustment', 'refstateswm'])
def test_solve_one_dimensional_apps_by_sweeps_and_directly(app):
    """65 -> 129 -> 257 points.  The direct solve has no iteration error; the sweeps must agree with it to 1 % of the
    discretisation error."""
    key = (app, 'lat')
    case = M.CASES[key]
    Es, Ed = [], []
    for n in M.GRIDS:
        E1, st1, _, _, S1, p = _solve(case, n, extra=dict(mxLoop=100000, tolerance=1e-14))
        assert st1['path'] == _lib.PATH_WAVE1D, st1
        E2, st2, _, _, S2, _ = _solve(case, n, extra={'method': 'direct'})
        assert st2['path'] == _lib.PATH_DIRECT1D, st2
        live = p['live']
        assert np.abs(S1 - S2)[live].max() <= 0.01 * np.abs(S2 - p['S'])[live].max(), (key, n)
        Es.append(E1)
        Ed.append(E2)
    _assert_order(Es, ids(key) + ' sweeps')
    _assert_order(Ed, ids(key) + ' direct')


def test_solve_multigrid_latlon_poisson():
    key = ('poisson', 'lat-lon')
    case = M.CASES[key]
    Es = []
    for n in G2:
        p = M.problem(case, n)
        ip = dict(p['iParams'], **SWEEPS)
        S, fs, os_ = multigrid.invert_MultiGrid(apps.invert_Poisson, p['F'], list(case.dims), case.coords, p['icbc'], p['mParams'],
                                                ip, ratio=2, gridNo=3)
        assert len(os_) == 3 and os_[0].shape == (p['shape'][0] // 4, p['shape'][1] // 4)     # three levels ran
        ipr = dict(p['iParams'])
        apps.residual(case.app, S, p['F'], list(case.dims), case.coords, p['icbc'], p['mParams'], ipr)
        ret, trunc = float(np.asarray(ipr['resid'])[0][2]), float(_truncation(case, p)[2])
        assert ret <= 0.01 * trunc, (n, ret, trunc)
        live = p['live']
        Es.append(np.abs(np.asarray(S.values) - p['S'])[live].max() / np.abs(p['S'][live]).max())
    _assert_order(Es, 'multigrid ' + ids(key))
