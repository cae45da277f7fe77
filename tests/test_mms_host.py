"""Manufactured solutions, host side: every app's coefficient builder and the grid metrics, through the numpy
residual model (tests/resid_model.py) or -- for the apps without a residual -- a converged oracle / direct solve, must
converge at second order to the continuous operator tests/mms_cases.py states.  No GPU.

e(n) = max|R| / max|F| of the manufactured S on grid n (E(n) = max|S - S_exact| / max|S_exact| for the solves); theory gives
e(n) / e(2n) = 4.  Asserted: >= 3.0 at the first refinement, >= 3.5 at the last.  The table's S and grids are chosen so that
the model alone gives >= 3.7 at the last (the measured ratios are in DESIGN.md 6.1); the bound is a condition on the
code, not a tolerance to tune."""
import numpy as np
import pytest

import mms_cases as M
import tridiag_model
import util
from xinvert_amd import apps, forms
from xinvert_amd.field import Field

ids = lambda k: '/'.join(k)
RES_KEYS = sorted(M.RESIDUAL_CASES)
SOLVE_KEYS = sorted(M.SOLVE_CASES)


def _ratios(es):
    return [es[i] / es[i + 1] for i in range(len(es) - 1)]


def _assert_order(es, what):
    r = _ratios(es)
    print(what, 'e =', ' '.join('%.3e' % e for e in es), 'ratios =', ' '.join('%.2f' % v for v in r))
    assert r[-1] >= M.LAST, (what, r)
    assert r[0] >= (M.FIRST if len(r) > 1 else M.LAST), (what, r)


@pytest.mark.parametrize('key', RES_KEYS, ids=ids)
def test_builder_and_metrics_give_a_second_order_residual(key):
    case = M.CASES[key]
    es = []
    for n in M.GRIDS:
        p = M.problem(case, n)
        nm = M.model_norms(case, p)
        assert nm[0] == p['live_expected'], (key, n)
        es.append(nm[2] / nm[3])
    M.check_weights(case, p)                                   # on the finest grid
    _assert_order(es, ids(key))


@pytest.mark.parametrize('kind', sorted(M.MASKED))
def test_masked_forcing_keeps_the_order_on_the_live_points(kind):
    """An undefined block in the forcing (_mask_FS, _remask, _scale_remask): NaN in one form, a value in another.  The
    block's S comes from icbc; the live count is the interior minus the block."""
    key, how = M.MASKED[kind]
    case = M.CASES[key]
    assert case.kind == kind
    es = []
    for n in M.GRIDS:
        p = M.problem(case, n, mask=how)
        blk = M.block(p['shape'])
        assert (np.isnan(p['F'].values[blk]).all() if how == 'nan' else (p['F'].values[blk] == p['iParams']['undef']).all())
        clear = M.problem(case, n)
        assert p['live_expected'] == clear['live_expected'] - int(np.prod([s.stop - s.start for s in blk]))
        nm = M.model_norms(case, p)
        assert nm[0] == p['live_expected'], (key, n)
        es.append(nm[2] / nm[3])
    _assert_order(es, ids(key) + ' masked:' + how)


SOLVES = [(k, None) for k in SOLVE_KEYS] + [M.MASKED_SOLVE[k] for k in sorted(M.MASKED_SOLVE)]


@pytest.mark.parametrize('key,mask', SOLVES, ids=[ids(k) + ('' if m is None else '/masked:' + m) for k, m in SOLVES])
def test_apps_without_a_residual_converge_in_the_solution(key, mask):
    """StommelMunk (oracle, reference ordering, converged until further sweeps move S by less than 1 % of the
    discretisation error) and the two 1-D apps (the tridiagonal direct solve: no iteration error at all).  The masked
    variants put an undefined block inside the domain: its S comes from icbc, and the order holds on the live points."""
    case = M.CASES[key]
    Es = []
    for n in (M.GRIDS[:2] if case.rank == 2 else M.GRIDS):
        p = M.problem(case, n, mask=mask)
        if mask is not None:
            assert p['live_expected'] < M.problem(case, n)['live_expected']
        q, iP = M.oracle_problem(case, p)
        assert int((q['coefs'][-1] != M.UNDEF)[p['live']].sum()) == p['live_expected'] == int(p['live'].sum())
        assert (q['coefs'][-1][M.block(p['shape'])] == M.UNDEF).all() or mask is None
        if case.rank == 1:
            S, _ = tridiag_model.direct_solve(q['S0'], q['coefs'][0], q['coefs'][1], q['coefs'][2], case.BCs[0], q['delxSqr'], M.UNDEF)
        else:
            S, fl = util.run_oracle(q, 400000, 1e-13, 0)
            assert fl[2] < 400000
            more, _ = util.run_oracle(dict(q, S0=S), 500, 0.0, 0)
            assert np.abs(more - S).max() <= 0.01 * np.abs(S - p['S'])[p['live']].max()
        live = p['live']
        Es.append(np.abs(S - p['S'])[live].max() / np.abs(p['S'][live]).max())
    M.check_weights(case, p)
    _assert_order(Es, ids(key))


@pytest.mark.parametrize('key', sorted(M.CASES), ids=ids)
def test_cal_params_state_the_metric(key):
    """_cal_params1D/2D/3D against the metric the table states: degrees * pi / 180 * Rearth on the dims that are angles."""
    case = M.CASES[key]
    p = M.problem(case, 16)
    _, _, _, iP = M.front_state(case, p)
    hs = [float(m[1] - m[0]) for m in p['metric']]             # first core dim first
    names = [('del1',), ('del2', 'del1'), ('del3', 'del2', 'del1')][case.rank - 1]
    for nm, h, N in zip(names, hs, p['shape']):
        assert iP[nm] == pytest.approx(h, rel=1e-13), (key, nm)
        assert iP['gc' + nm[-1]] == N
    assert iP['del1Sqr'] == pytest.approx(hs[-1] ** 2, rel=1e-13)
    if case.rank == 2:
        r = hs[1] / hs[0]
        for nm, v in (('ratio', r), ('ratioSqr', r ** 2), ('ratioQtr', r / 4), ('ratioSSr', r ** 4), ('del1Tr', hs[1] ** 3),
                      ('del1SSr', hs[1] ** 4)):
            assert iP[nm] == pytest.approx(v, rel=1e-13), (key, nm)
    if case.rank == 3:
        for nm, v in (('ratio1', hs[2] / hs[1]), ('ratio2', hs[2] / hs[0]), ('ratio1Sqr', (hs[2] / hs[1]) ** 2),
                      ('ratio2Sqr', (hs[2] / hs[0]) ** 2)):
            assert iP[nm] == pytest.approx(v, rel=1e-13), (key, nm)


ALL_COORDS = ('lat-lon', 'z-lat', 'z-lon', 'cartesian', 'lat')


def _accepts(case, coords):
    """Does the app's builder take this coordinate branch?  (Its `else` raises 'unsupported coords'; the 1-D apps name
    'cartesian' and raise 'not supported'.)"""
    p = M.problem(case, 16)
    iP = apps._update(apps.default_iParams, p['iParams'])
    mP = apps._update(apps.default_mParams, p['mParams'], case.valid)
    try:
        getattr(apps, case.builder)(p['F'], list(case.dims), coords, mP, iP, p['icbc'])
    except Exception as e:
        if 'unsupported coords' in str(e) or 'not supported for' in str(e):
            return False
        raise
    return True


def test_table_holds_every_app_in_every_branch_it_accepts():
    """An app added to apps.py without a table entry fails here."""
    table_apps = {k[0] for k in M.CASES}
    assert table_apps == set(apps._RESIDUAL) | set(M.NO_RESIDUAL)
    entry_points = {n[len('invert_'):].lower() for n in dir(apps) if n.startswith('invert_')}
    assert entry_points == table_apps                          # every invert_* has its rows
    for app in sorted(table_apps):
        have = {k[1] for k in M.CASES if k[0] == app}
        case = next(c for k, c in M.CASES.items() if k[0] == app)
        accepted = {c for c in ALL_COORDS if _accepts(case, c)}
        assert have == accepted, (app, have, accepted)
        assert have == set(M.BRANCHES.get(app, ('lat-lon', 'cartesian')))
    assert set(M.MASKED) == set(forms.RESIDUAL) and set(M.MASKED) | set(M.MASKED_SOLVE) == set(forms.FORMS) - {'std1d'}
    # every form has a row, and every row states a coefficient for letters of its own form only
    assert {c.kind for c in M.CASES.values()} == set(forms.FORMS)
    for k, c in M.CASES.items():
        assert set(c.coef) <= set(forms.FORMS[c.kind].arrays[:-1]), k
        assert all(flag in ('half', 'grid') for _, flag in c.coef.values()), k
        assert all(b in ('fixed', 'periodic') for b in c.BCs), k


def test_grid_flag_is_what_keeps_a_grid_sampled_coefficient_second_order():
    """The helper's own teeth: PV2D samples f0^2 / N2(z) on the grid point and the kernel uses it half a cell lower.  Against
    the unshifted function the residual is first order (ratio 2); against the shifted one it is second order."""
    case = M.CASES[('pv2d', 'cartesian')]
    assert case.grid_flagged() == ['A']
    plain = M.Case(case.app, case.coords, case.dims, case.axes, case.BCs, case.mParams,
                   dict(case.coef, A=(case.coef['A'][0], 'half')), case.S, case.user, case.shape, fields=case.fields)
    es = []
    for n in M.GRIDS:
        nm = M.model_norms(plain, M.problem(plain, n))
        es.append(nm[2] / nm[3])
    r = _ratios(es)
    assert 1.7 <= r[-1] <= 2.3, r


def test_front_end_arguments_of_the_table_rows():
    """Each row's mParams are ones its entry point accepts, and its S is non-zero on every fixed boundary."""
    for k, c in M.CASES.items():
        p = M.problem(c, 16)
        apps._update(apps.default_mParams, p['mParams'], c.valid)              # raises on a key the app refuses
        for ax, BC in enumerate(c.BCs):
            if BC == 'fixed':
                for e in (0, -1):
                    assert np.abs(np.take(p['S'], e, axis=ax)).max() > 0, k
        assert isinstance(p['F'], Field) and p['F'].dims == c.dims
