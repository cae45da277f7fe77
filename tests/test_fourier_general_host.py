"""The direct Fourier solve of the 2-D general form ('cfourier') without a GPU: the numpy restatement
(tests/fourier_general_model.py) against a long-double truth (tests/fourier_general_ld.py) and against the oracle's converged
lexicographic sweeps, the front end's eligibility errors, the sigma table and the C-ABI names.

Measured here (python -m pytest tests/test_fourier_general_host.py -s prints them; DESIGN.md 4.16 records them):
    family                          rel-L2(model, truth)     max|R| / (max|G| delxSqr) of the model's field, in long double
    random dominant, 22 shapes      3.1e-17 .. 3.2e-16       4.9e-16 .. 5.0e-15
    Gill-Matsuno 9 x 12 .. 73 x 144 7.3e-16 .. 1.7e-14       1.1e-15 .. 3.8e-14
The bars are 4x the largest value of each family (floor 2^-53), for rounding differences between numpy builds.
    Gill-Matsuno 37 x 72: rel-L2(model, oracle) 2e-13 (892 sweeps);  73 x 144: 9e-13 (3251 sweeps)
"""
import os
import re

import numpy as np
import pytest

import fourier_general_ld as T
import fourier_general_model as GM
import fourier_model as M
import util
from xinvert_amd import _lib, apps, core, fourier
from xinvert_amd.field import Field

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = -9.99e8
HALF_ULP = 2.0 ** -53

# 4x the largest value measured over each family's shapes (the module's header)
RANDOM_BARS = (4 * 3.17e-16, 4 * 4.95e-15)
GM_BARS = (4 * 1.71e-14, 4 * 3.79e-14)

RANDOM_SHAPES = [(yc, xc, 2) for yc in (3, 4, 5, 6) for xc in (3, 4, 6, 8, 125)] + [(300, 12, 1), (130, 45, 1)]
GM_SHAPES = [(9, 12), (19, 30), (37, 72), (73, 144)]


def rel_ld(S, truth):
    d = np.asarray(S).astype(T.LD) - truth
    return float(np.sqrt((d * d).sum() / (truth * truth).sum()))


def model_against_truth(p, bars, what):
    St = T.ld_solve(p['S0'], p['c'], p['G'], p['sc'])
    Sm, fl = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    assert St.dtype == np.longdouble and not fl.any()
    assert np.array_equal(Sm[:, [0, -1]], p['S0'][:, [0, -1]]) and np.array_equal(St[:, [0, -1]], p['S0'][:, [0, -1]])
    fe = rel_ld(Sm, St)
    be = float(T.ld_backward(Sm, p['c'], p['G'], p['sc']).max())
    bt = float(T.ld_backward(St, p['c'], p['G'], p['sc']).max())
    print('%s %3d x %3d x %d: rel-L2(model, truth) %.2e; backward error in long double model %.2e truth %.2e'
          % (what, p['yc'], p['xc'], p['nb'], fe, be, bt))
    assert fe <= max(bars[0], HALF_ULP), (fe, bars)
    assert be <= max(bars[1], HALF_ULP), (be, bars)
    assert bt * 64 <= be                                     # (the truth is one: 64 significant bits leave 2^-11 of the rounding)
    return Sm


@pytest.mark.parametrize('yc,xc,nb', RANDOM_SHAPES, ids=['%dx%d' % s[:2] for s in RANDOM_SHAPES])
def test_model_against_the_long_double_truth(yc, xc, nb):
    model_against_truth(GM.problem(yc, xc, nb, False, 7000 + 10 * xc + yc), RANDOM_BARS, 'random')


@pytest.mark.parametrize('ny,nx', GM_SHAPES, ids=['%dx%d' % s for s in GM_SHAPES])
def test_model_against_the_truth_on_gill_matsuno(ny, nx):
    p = GM.gill_matsuno(ny, nx)
    Sm = model_against_truth(p, GM_BARS, 'gill-matsuno')
    assert np.isfinite(Sm).all()


@pytest.mark.parametrize('ny,nx', [(37, 72), (73, 144)])
def test_model_is_the_fixed_point_of_the_reference_sweeps(oracle, ny, nx):
    """rel-L2(model, converged lexicographic oracle) within the project's bound for converged fields.  (At 9 x 12
    and 19 x 30 the oracle's sweeps overflow: those shapes are not used here.)"""
    p = GM.gill_matsuno(ny, nx)
    Sm, fl = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    So, flo = util.run_oracle(p['full'], 2000000, 1e-14, oracle.LEX)
    assert flo[0] == 0 and flo[2] < 2000000, flo
    err = util.rel_l2(Sm[0], So)
    print('gill-matsuno %d x %d: rel-L2(model, oracle) %.1e (oracle loops %d)' % (ny, nx, err, flo[2]))
    assert not fl.any() and err <= 1e-6


def test_shared_coefficients_and_single_members_give_the_same_bits():
    p = GM.problem(6, 12, 3, True, 5)
    S, _ = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    per = [np.broadcast_to(x, (3, 6)).copy() for x in p['c']]
    S2, _ = GM.solve(p['S0'], per, p['G'], p['sc'], U)
    assert np.array_equal(S, S2)
    S1, fl1 = GM.solve(p['S0'][1], p['c'], p['G'][1], p['sc'], U)
    assert S1.shape == (6, 12) and np.array_equal(S1, S[1]) and list(fl1) == [0, 0, 0]


def test_model_refuses_undef_and_flags_nan_for_the_member_alone():
    p = GM.problem(6, 12, 3, False, 6)
    S, fl = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    assert not fl.any()
    arrays = dict(zip('ACDEF', p['c']), G=p['G'], S=p['S0'])

    def solve(**over):
        a = dict(arrays, **over)
        return GM.solve(a['S'], [a[k] for k in 'ACDEF'], a['G'], p['sc'], U)

    for name, idx in [('G', (1, 2, 3)), ('S', (2, 0, 5)), ('S', (0, 5, 0))] + [(k, (1, 4)) for k in 'ACDEF']:
        bad = arrays[name].copy()
        bad[idx] = U
        with pytest.raises(ValueError, match='member %d holds undef at 1' % idx[0]):
            solve(**{name: bad})
    for name, idx in [('G', (1, 0, 3)), ('G', (1, 5, 3)), ('S', (1, 2, 2))] + [(k, (1, j)) for k in 'ACDEF' for j in (0, 5)]:
        ok = arrays[name].copy()                               # points the solve never reads
        ok[idx] = U
        S2, _ = solve(**{name: ok})
        assert np.array_equal(S2[:, 1:-1], S[:, 1:-1]), (name, idx)
    Gn = p['G'].copy()
    Gn[1, 3, 3] = np.nan
    Sn, fl = solve(G=Gn)
    assert list(fl[:, 0]) == [0, 1, 0] and np.array_equal(Sn[[0, 2]], S[[0, 2]])


def test_sigma_is_exactly_zero_where_the_half_spectrum_is_real():
    for n in (3, 4, 5, 6, 8, 12, 125, 144, 360, 4096):
        s = GM.sigma(n)
        assert s.shape == (n // 2 + 1,) and s[0] == 0.0
        if n % 2 == 0:
            assert s[n // 2] == 0.0
        assert (s[1:(n + 1) // 2] > 0).all()
        k = np.arange(n // 2 + 1)
        # (float64's argument 2 pi k / n carries up to two roundings of a value near pi: 2 * 4.4e-16, plus sin's own)
        assert np.abs(s - np.sin(2 * np.pi * k / n)).max() <= 1e-15
    host = open(os.path.join(ROOT, 'xinvert_amd', 'csrc', 'xinv_fourier_host.h')).read()
    assert re.search(r'\(k == 0 \|\| 2 \* k == n\) \? 0\.0 : \(double\)sinl\(', host)      # (the library's table: the same rule)


# ------------------------------------------------------------------ the front end's eligibility
def front(ny=9, nx=12, nb=2):
    lat = np.linspace(-60, 60, ny)
    lon = np.arange(nx) * (360.0 / nx)
    rng = np.random.default_rng(7)
    dims3 = ('t', 'lat', 'lon')
    co = {'t': np.arange(nb), 'lat': lat, 'lon': lon}
    G = Field(rng.standard_normal((nb, ny, nx)), dims3, co)
    S = Field(np.zeros((nb, ny, nx)), dims3, co)
    row = lambda v: np.broadcast_to(v[:, None], (ny, nx))
    cs = dict(A=row(np.cos(np.deg2rad(lat))), B=np.broadcast_to(np.zeros(()), (ny, nx)), C=row(1.0 / np.cos(np.deg2rad(lat))),
              D=row(np.sin(np.deg2rad(lat))), E=row(0.3 + 0 * lat), F=row(-0.1 * np.cos(np.deg2rad(lat))))
    ip = apps._update(apps.default_iParams, apps._cal_params2D(lat, lon, 'lat-lon'))
    ip = dict(ip, BCs=['fixed', 'periodic'], method='cfourier', printInfo=False, mxLoop=3)
    return dict(cs, G=G, S=S, ip=ip)


def call(c, **over):
    c = dict(c, **over)
    return core.inv_general2D(c['A'], c['B'], c['C'], c['D'], c['E'], c['F'], c['G'], c['S'], ['lat', 'lon'], c['ip'])


def past_the_refusals(fn):
    """The call is not refused: it solves (a GPU is there) or gets as far as asking for one."""
    try:
        fn()
    except _lib.XinvError as e:
        assert 'no CPU fallback' in str(e), e


def masked(f, at):
    return Field(np.where(np.arange(f.values.size).reshape(f.shape) == at, U, f.values), f.dims, f.coords)


REFUSED = {
    'non-zero B': (lambda c: dict(B=np.full((9, 12), 0.01)), r'B must be identically zero'),
    'extend, periodic': (lambda c: dict(ip=dict(c['ip'], BCs=['extend', 'periodic'])), r"along y is 'extend'"),
    'fixed, fixed': (lambda c: dict(ip=dict(c['ip'], BCs=['fixed', 'fixed'])), r"along x is 'fixed'"),
    'masked forcing': (lambda c: dict(G=masked(c['G'], 40)), r'array G holds one on rows 1 \.\. yc-2'),
    'masked boundary row': (lambda c: dict(S=masked(c['S'], 3)), r'array S holds one on rows 0 and yc-1'),
}
for _k in 'ACDEF':
    REFUSED['%s varies along x' % _k] = (lambda c, k=_k: {k: c[k] * (1 + 0.01 * (np.arange(12) == 5))},
                                         r'%s must be constant along x' % _k)
    REFUSED['undef in %s' % _k] = (lambda c, k=_k: {k: np.where(np.arange(9)[:, None] == 4, U, c[k])}, r'array %s holds one' % _k)


@pytest.mark.parametrize('name', list(REFUSED))
def test_each_condition_is_refused_by_name_and_sor_is_not(name):
    change, pattern = REFUSED[name]
    c = front()
    c = dict(c, **change(c))
    with pytest.raises(Exception, match=pattern) as ei:
        call(c)
    assert "'cfourier'" in str(ei.value) and "'sor' solves this case" in str(ei.value)
    past_the_refusals(lambda: call(c, ip=dict(c['ip'], method='sor')))


def test_the_conditions_are_checked_in_the_stated_order():
    """B, the y code, the x code, A, C, D, E, F constant along x, undef, yc, xc: with every condition broken the first is
    named; mended one by one, the next."""
    c = front(nx=14)
    vary = lambda a: a * (1 + 0.01 * (np.arange(14) == 5))
    broken = dict(B=np.full((9, 14), 0.01), ip=dict(c['ip'], BCs=['extend', 'fixed']), G=masked(c['G'], 40),
                  **{k: vary(c[k]) for k in 'ACDEF'})
    steps = [('B', r'B must be identically zero'), ('ip', r"along y is 'extend'"), ('ip2', r"along x is 'fixed'")] + \
            [(k, r'%s must be constant along x' % k) for k in 'ACDEF'] + [('G', r'array G holds one'), (None, r'prime factor 7')]
    cur = dict(c, **broken)
    for key, pattern in steps:
        with pytest.raises(Exception, match=pattern):
            call(cur)
        if key == 'ip':
            cur = dict(cur, ip=dict(c['ip'], BCs=['fixed', 'fixed']))
        elif key == 'ip2':
            cur = dict(cur, ip=c['ip'])
        elif key is not None:
            cur = dict(cur, **{key: c[key]})
    with pytest.raises(Exception, match='yc must be at least 3'):
        two = (np.ones(2), True)
        fourier.eligible_general(two, (None, False), two, two, two, two, np.ones((1, 2, 12)), np.ones((1, 2, 12)),
                                 ['fixed', 'periodic'], U)


@pytest.mark.parametrize('nx,factor', [(14, 7), (77, 7)])
def test_row_lengths_with_another_prime_factor_are_refused(nx, factor):
    c = front(nx=nx)
    with pytest.raises(Exception, match='the row length %d has the prime factor %d' % (nx, factor)) as ei:
        call(c)
    assert "'cfourier'" in str(ei.value) and "'sor' solves this case" in str(ei.value)
    past_the_refusals(lambda: call(c, ip=dict(c['ip'], method='sor')))


def test_cfourier_is_the_2d_general_forms_alone():
    c = front()
    G, ip = c['G'], c['ip']
    with pytest.raises(Exception, match="'cfourier' is available for the 2-D general form only.*inv_standard2D.*'sor' solves this case"):
        core.inv_standard2D(G, G, G, G, c['S'], ['lat', 'lon'], ip)
    with pytest.raises(Exception, match="'cfourier' is available for the 2-D general form only.*inv_standard1D.*'sor' solves this case"):
        core.inv_standard1D(G, G, G, c['S'], ['lon'], ip)
    with pytest.raises(Exception, match="'cfourier' is available for the 2-D general form only.*inv_standard3D.*'sor' solves this case"):
        core.inv_standard3D(G, G, G, G, c['S'], ['t', 'lat', 'lon'], ip)
    with pytest.raises(Exception, match="^iParams\\['method'\\] must be 'sor' or 'direct'"):
        call(c, ip=dict(ip, method='fft'))
    with pytest.raises(Exception, match="'fourier' is available for the 2-D standard form only"):
        call(c, ip=dict(ip, method='fourier'))
    with pytest.raises(NotImplementedError, match="'cfourier' runs on one device"):
        call(c, ip=dict(ip, devices=[0, 1]))
    with pytest.raises(NotImplementedError, match='one device'):
        call(c, ip=dict(ip, devices='all'))
    # an eligible call passes every check and asks for the GPU
    past_the_refusals(lambda: call(c))
    past_the_refusals(lambda: call(c, **{k: np.ascontiguousarray(c[k]) for k in 'ABCDEF'}))     # (dense arrays, constant along x)


def test_eligible_general_hands_over_one_value_per_row():
    c = front()
    Gv, Sv = c['G'].values, c['S'].values
    co = [(c['A'][:, 0].copy(), True), (None, False)] + [(np.ascontiguousarray(c[k]), False) for k in 'CDEF']
    rows = fourier.eligible_general(*co, Gv, Sv, ['fixed', 'periodic'], U)
    assert len(rows) == 5 and all(r.shape == (9,) for r in rows)
    for r, k in zip(rows, 'ACDEF'):
        assert np.array_equal(r, c[k][:, 0])
    Sb = Sv.copy()
    Sb[1, 4, 3] = U                                            # an interior first guess is not read
    fourier.eligible_general(*co, Gv, Sb, ['fixed', 'periodic'], U)
    pole = [(np.where(np.arange(9) % 8 == 0, U, r), True) for r in rows]      # rows 0 and yc-1 of a coefficient are not read
    fourier.eligible_general(pole[0], (None, False), *pole[1:], Gv, Sv, ['fixed', 'periodic'], U)
    nan = rows[0].copy()
    nan[0] = np.nan                                            # (NaN beyond the pole is constant along x too)
    full = np.broadcast_to(nan[:, None], (9, 12)).copy()
    fourier.eligible_general((full, False), (None, False), *co[2:], Gv, Sv, ['fixed', 'periodic'], U)


def test_template_builds_the_forcing_on_the_host_for_cfourier():
    src = open(os.path.join(ROOT, 'xinvert_amd', 'apps.py')).read()
    assert "not in ('fourier', 'cfourier')" in src


# ------------------------------------------------------------------ C-ABI
def test_abi_names_declared_typed_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xinv.h')).read()
    sub = open(os.path.join(ROOT, 'include', 'xinv_fourier.h')).read()
    L = _lib.load()
    for name in ('xinv_fourier_general_2d_f64_dev', 'xinv_fourier_general_2d_f64_batched'):
        assert re.search(r'\bint\s+%s\s*\(' % name, sub) and len(re.findall(r'\b%s\s*\(' % name, hdr)) == 1, name
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == 18
        proto = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, sub).group(1)
        assert len(proto.split(',')) == 18, name


def test_build_lists_the_new_unit():
    from xinvert_amd import build
    assert ('xinv_tu_cfourier', 'xinv_tu_cfourier.hip', []) in build.UNITS
    assert os.path.exists(os.path.join(build.CSRC, 'xinv_cfourier.h')) and '-ffp-contract=off' in build.BASE_FLAGS
    assert M.MAX_N == fourier.MAX_N
