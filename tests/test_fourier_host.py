"""The direct Fourier solve of the 2-D standard form without a GPU: the numpy restatement (tests/fourier_model.py) against
the oracle's converged lexicographic sweeps, its residual through tests/resid_model.py, the front end's eligibility
errors, and the C-ABI names.

Measured here (python -m pytest tests/test_fourier_host.py -s prints them; DESIGN.md 4.16 records them):
    case              rel-L2(model, oracle)   max|R| / max|F| of the model's field
    latlon 7 x 12     3.5e-14                 2.9e-16
    latlon 37 x 45    5.9e-12                 1.7e-15
    latlon 19 x 30    4.4e-11                 9.2e-16
    cartesian 16 x 20 1.7e-13                 1.9e-15
(the oracle's own fields, swept to tolerance 1e-14, hold 1.5e-14 .. 2.9e-12 by the same measure)
"""
import os
import re

import numpy as np
import pytest

import fourier_ld as T
import fourier_model as M
import resid_model as RM
import util
import xinvert_amd as xa
from xinvert_amd import _lib, apps, core, fourier, synthetic
from xinvert_amd.field import Field

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = -9.99e8


def latlon_case(ny, nx, seed):
    """Unmasked lat-lon Poisson problem with random (non-zero) boundary rows -> the problem dict of tests/util.py."""
    p = synthetic.member(synthetic.poisson_latlon(ny, nx, mask=False, seed=seed), 0)
    rng = np.random.default_rng(seed)
    scale = np.abs(p['coefs'][3]).max() * p['delxSqr']
    S0 = np.zeros((ny, nx))
    S0[0], S0[-1] = rng.standard_normal(nx) * scale, rng.standard_normal(nx) * scale
    return dict(p, S0=S0)


def cartesian_case(ny, nx, seed):
    rng = np.random.default_rng(seed)
    A = np.broadcast_to(rng.uniform(0.5, 1.5, ny)[:, None], (ny, nx))
    C = np.broadcast_to(rng.uniform(0.5, 1.5, ny)[:, None], (ny, nx))
    S0 = np.zeros((ny, nx))
    S0[0], S0[-1] = rng.standard_normal(nx), rng.standard_normal(nx)
    dely, delx = 1.3, 1.1
    r = delx / dely
    return dict(kind='std2d', yc=ny, xc=nx, BCy='fixed', BCx='periodic', dely=dely, delx=delx, delxSqr=delx ** 2, ratio=r,
                ratioQtr=r / 4, ratioSqr=r ** 2, optArg=1.5, undef=U, S0=S0,
                coefs=[A, np.zeros((ny, nx)), C, rng.standard_normal((ny, nx))])


CASES = [('latlon 7 x 12', lambda: latlon_case(7, 12, 1)), ('latlon 37 x 45', lambda: latlon_case(37, 45, 2)),
         ('latlon 19 x 30', lambda: latlon_case(19, 30, 3)), ('cartesian 16 x 20', lambda: cartesian_case(16, 20, 4))]


def crel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def model_solve(p):
    A, _, C, F = p['coefs']
    return M.solve(p['S0'], np.asarray(A)[:, 0], np.asarray(C)[:, 0], F, p['delxSqr'], p['ratioSqr'], U)


def backward_error(p, S):
    """max|R| / max|F| of a field by the numpy restatement of the residual (tests/resid_model.py)."""
    A, _, C, F = [None if c is None else np.ascontiguousarray(c, dtype=np.float64) for c in p['coefs']]
    R, live = RM.residual('std2d', S, [A, None, C, F], p, True, U)
    nrm = RM.norms(R, F, live)
    return nrm[2] / nrm[3]


@pytest.mark.parametrize('name,make', CASES, ids=[c[0] for c in CASES])
def test_model_is_the_fixed_point_of_the_reference_sweeps(oracle, name, make):
    """rel-L2(model, converged lexicographic oracle) within the project's bound for converged fields, and
    the model's backward error.  A backward-stable solve leaves a residual of a few eps times what the stencil sums in
    magnitude, |R| <= c eps (|L| |S|): here (|L| |S|) <= (4 max(A) ratioSqr + 4 max(C)) max|S| / delxSqr, and c = 64 covers
    the log2(xc) <= 6 butterfly levels of the two transforms and the three operations per row of the recurrence."""
    p = make()
    S, fl = model_solve(p)
    assert list(fl) == [0, 0, 0]
    So, flo = util.run_oracle(p, 2000000, 1e-14, oracle.LEX)
    assert flo[0] == 0 and flo[2] < 2000000, flo
    err, be = util.rel_l2(S, So), backward_error(p, S)
    print('%-18s rel-L2(model, oracle) %.1e   max|R|/max|F| model %.1e  oracle %.1e  (oracle loops %d)'
          % (name, err, be, backward_error(p, So), flo[2]))
    assert err <= 1e-6
    A, _, C, F = p['coefs']
    stencil = (4 * np.asarray(A)[1:].max() * p['ratioSqr'] + 4 * np.asarray(C)[1:-1].max()) * np.abs(S).max() / p['delxSqr']
    assert be <= 64 * np.finfo(np.float64).eps * stencil / np.abs(F[1:-1]).max()
    assert np.array_equal(S[0], p['S0'][0]) and np.array_equal(S[-1], p['S0'][-1])


def test_model_transform_is_numpys():
    rng = np.random.default_rng(5)
    for n in (3, 4, 5, 12, 30, 45, 64, 360):
        for rows in (1, 2, 3):
            x = rng.standard_normal((rows, n))
            ref = np.fft.rfft(x)
            X = M.rfft_rows(x)
            assert crel(X, ref) < 2e-15, (n, rows)
            assert crel(M.irfft_rows(X, n), x) < 2e-15, (n, rows)
            junk = ref.copy()
            junk[:, 0] += 3j                                   # numpy ignores Im X[0] (and Im X[n/2]); so does the model
            if n % 2 == 0:
                junk[:, -1] -= 2j
            assert crel(M.irfft_rows(junk, n), x) < 2e-15, (n, rows)
    assert M.factor(3600) == [4, 4, 3, 3, 5, 5] and M.factor(45) == [3, 3, 5] and M.factor(64) == [4, 4, 4]
    _, lam = M.tables(3600)
    assert lam[0] == 0.0 and abs(lam[1] / (2 * np.pi / 3600) ** 2 - 1) < 1e-6        # (2 - 2 cos would hold 9 digits here)


LD_SHAPES = [(3, 3), (5, 6), (37, 128), (130, 45), (300, 12)]


@pytest.mark.parametrize('yc,xc', LD_SHAPES, ids=['%dx%d' % s for s in LD_SHAPES])
def test_long_double_truth_leaves_a_64th_of_the_models_residual(yc, xc):
    """tests/fourier_ld.py pinned against the model, two members with their own A, C in [0.5, 1.5]: the truth's residual of
    the five-point equation, evaluated in long double, is at most 1/64 of the model's (a solve carried out in 64
    significant bits instead of 53 leaves 2^-11 of the rounding; measured 1/1600 .. 1/380, the truth's residual 4e-19 ..
    2e-16, the model's 6e-16 .. 2e-13), and the model lies within 1e-9 of the truth (measured 5e-17 .. 1e-13)."""
    rng = np.random.default_rng(1000 * yc + xc)
    nb = 2
    A, C = rng.uniform(0.5, 1.5, (nb, yc)), rng.uniform(0.5, 1.5, (nb, yc))
    F = rng.standard_normal((nb, yc, xc))
    S0 = rng.standard_normal((nb, yc, xc)) * np.abs(F).max() * 1.21
    sc = (1.21, (1.1 / 1.3) ** 2)
    St = T.ld_solve(S0, A, C, F, *sc)
    Sm, fl = M.solve(S0, A, C, F, *sc, U)
    assert St.dtype == np.longdouble and not fl.any()
    assert np.array_equal(St[:, [0, -1]], S0[:, [0, -1]])
    be_t, be_m = T.ld_backward(St, A, C, F, *sc), T.ld_backward(Sm, A, C, F, *sc)
    d = Sm.astype(np.longdouble) - St
    fe = float(np.sqrt((d * d).sum() / (St * St).sum()))
    print('ld truth %3d x %3d: max|R|/max|F| truth %.1e model %.1e (1/%.0f); rel-L2(model, truth) %.1e'
          % (yc, xc, be_t.max(), be_m.max(), (be_m / be_t).min(), fe))
    assert (be_t * 64 <= be_m).all(), (be_t, be_m)
    assert fe < 1e-9
    one = T.ld_solve(S0[1], A[1], C[1], F[1], *sc)             # a single member, a shared row of coefficients
    assert one.shape == (yc, xc) and np.array_equal(one, St[1])


def test_model_refuses_undef_and_flags_nan_for_the_member_alone():
    rng = np.random.default_rng(6)
    yc, xc, nb = 6, 12, 3
    A, C = rng.uniform(0.5, 1.5, (nb, yc)), rng.uniform(0.5, 1.5, (nb, yc))
    F, S0 = rng.standard_normal((nb, yc, xc)), rng.standard_normal((nb, yc, xc))
    S, fl = M.solve(S0, A, C, F, 1.0, 0.8, U)
    assert not fl.any()
    for arr, idx in ((F, (1, 2, 3)), (S0, (2, 0, 5)), (S0, (0, yc - 1, 0)), (A, (1, yc - 1)), (C, (0, 1))):
        bad = arr.copy()
        bad[idx] = U
        args = [bad if a is arr else a for a in (S0, A, C, F)]
        with pytest.raises(ValueError, match='holds undef'):
            M.solve(*args, 1.0, 0.8, U)
    for arr, idx in ((F, (1, 0, 3)), (S0, (1, 2, 2)), (A, (1, 0)), (C, (1, 0)), (C, (1, yc - 1))):     # points the solve never reads
        ok = arr.copy()
        ok[idx] = U
        args = [ok if a is arr else a for a in (S0, A, C, F)]
        S2, _ = M.solve(*args, 1.0, 0.8, U)
        assert np.array_equal(S2[:, 1:-1], S[:, 1:-1])
    An = A.copy()
    An[1, 3] = np.nan
    Sn, fl = M.solve(S0, An, C, F, 1.0, 0.8, U)
    assert list(fl[:, 0]) == [0, 1, 0] and np.array_equal(Sn[[0, 2]], S[[0, 2]])


# ------------------------------------------------------------------ the front end's eligibility
def front(ny=9, nx=12, nb=2):
    lat = np.linspace(-60, 60, ny)
    lon = np.arange(nx) * (360.0 / nx)
    rng = np.random.default_rng(7)
    dims3 = ('t', 'lat', 'lon')
    co = {'t': np.arange(nb), 'lat': lat, 'lon': lon}
    F = Field(rng.standard_normal((nb, ny, nx)), dims3, co)
    S = Field(np.zeros((nb, ny, nx)), dims3, co)
    row = lambda v: np.broadcast_to(v[:, None], (ny, nx))
    A, C = row(np.cos(np.deg2rad(lat))), row(1.0 / np.cos(np.deg2rad(lat)))
    B = np.broadcast_to(np.zeros(()), (ny, nx))
    ip = apps._update(apps.default_iParams, apps._cal_params2D(lat, lon, 'lat-lon'))
    ip = dict(ip, BCs=['fixed', 'periodic'], method='fourier', printInfo=False, mxLoop=3)
    return dict(A=A, B=B, C=C, F=F, S=S, ip=ip)


def call(c, **over):
    c = dict(c, **over)
    return core.inv_standard2D(c['A'], c['B'], c['C'], c['F'], c['S'], ['lat', 'lon'], c['ip'])


def past_the_refusals(fn):
    """The call is not refused: it solves (a GPU is there) or gets as far as asking for one."""
    try:
        fn()
    except _lib.XinvError as e:
        assert 'no CPU fallback' in str(e), e


REFUSED = {
    'masked forcing': (lambda c: dict(F=Field(np.where(np.arange(c['F'].values.size).reshape(c['F'].shape) == 40, U, c['F'].values),
                                              c['F'].dims, c['F'].coords)), r'array F holds one'),
    'undef in A': (lambda c: dict(A=np.where(np.arange(9)[:, None] == 4, U, c['A'])), r'array A holds one'),
    'A varies along x': (lambda c: dict(A=c['A'] * (1 + 0.01 * (np.arange(12) == 5))), r'A must be constant along x'),
    'non-zero B': (lambda c: dict(B=np.full((9, 12), 0.01)), r'B must be identically zero'),
    'extend, periodic': (lambda c: dict(ip=dict(c['ip'], BCs=['extend', 'periodic'])), r"along y is 'extend'"),
    'fixed, fixed': (lambda c: dict(ip=dict(c['ip'], BCs=['fixed', 'fixed'])), r"along x is 'fixed'"),
}


@pytest.mark.parametrize('name', list(REFUSED))
def test_each_condition_is_refused_by_name_and_sor_is_not(name):
    change, pattern = REFUSED[name]
    c = front()
    c = dict(c, **change(c))
    with pytest.raises(Exception, match=pattern) as ei:
        call(c)
    assert "'fourier'" in str(ei.value) and "'sor' solves this case" in str(ei.value)
    past_the_refusals(lambda: call(c, ip=dict(c['ip'], method='sor')))


@pytest.mark.parametrize('nx,factor', [(14, 7), (77, 7)])
def test_row_lengths_with_another_prime_factor_are_refused(nx, factor):
    c = front(nx=nx)
    with pytest.raises(Exception, match='the row length %d has the prime factor %d' % (nx, factor)) as ei:
        call(c)
    assert "'sor' solves this case" in str(ei.value)
    past_the_refusals(lambda: call(c, ip=dict(c['ip'], method='sor')))
    assert fourier.length_error(4500) and '4096' in fourier.length_error(4500)
    for ok in (3, 12, 45, 225, 360, 3600, 4096):
        assert fourier.length_error(ok) is None, ok


def test_fourier_is_the_2d_standard_forms_alone():
    c = front()
    F, ip = c['F'], c['ip']
    with pytest.raises(Exception, match="'fourier' is available for the 2-D standard form only.*inv_general2D"):
        core.inv_general2D(F, F, F, F, F, F, F, c['S'], ['lat', 'lon'], ip)
    with pytest.raises(Exception, match="'fourier' is available for the 2-D standard form only.*inv_standard1D"):
        core.inv_standard1D(F, F, F, c['S'], ['lon'], ip)
    past_the_refusals(lambda: core.inv_general2D(c['A'], c['B'], c['C'], c['B'], c['B'], c['B'], F, c['S'], ['lat', 'lon'],
                                                 dict(ip, method='sor', ratio=1.0)))
    with pytest.raises(Exception, match="must be 'sor' or 'direct'"):
        call(c, ip=dict(ip, method='fft'))
    with pytest.raises(NotImplementedError, match='one device'):
        call(c, ip=dict(ip, devices=[0, 1]))
    # an eligible call passes every check and asks for the GPU
    past_the_refusals(lambda: call(c))
    past_the_refusals(lambda: call(c, A=np.ascontiguousarray(c['A']), B=np.zeros((9, 12))))     # (dense arrays, constant along x)


def test_eligible_hands_over_one_value_per_row():
    c = front()
    Fv, Sv = c['F'].values, c['S'].values
    Ar, Cr = fourier.eligible((c['A'][:, 0].copy(), True), (None, False), (np.ascontiguousarray(c['C']), False), Fv, Sv,
                              ['fixed', 'periodic'], U)
    assert Ar.shape == Cr.shape == (9,) and np.array_equal(Cr, c['C'][:, 0])
    with pytest.raises(Exception, match='array S holds one on rows 0 and yc-1'):
        Sb = Sv.copy()
        Sb[1, -1, 3] = U
        fourier.eligible((Ar, True), (None, False), (Cr, True), Fv, Sb, ['fixed', 'periodic'], U)
    Sb = Sv.copy()
    Sb[1, 4, 3] = U                                            # an interior first guess is not read
    fourier.eligible((Ar, True), (None, False), (Cr, True), Fv, Sb, ['fixed', 'periodic'], U)


# ------------------------------------------------------------------ C-ABI
def test_abi_names_declared_typed_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xinv.h')).read()
    sub = open(os.path.join(ROOT, 'include', 'xinv_fourier.h')).read()
    assert re.search(r'^#include "xinv_fourier.h"', hdr, flags=re.M)
    L = _lib.load()
    for name, nargs in (('xinv_fourier_standard_2d_f64_dev', 13), ('xinv_fourier_standard_2d_f64_batched', 13),
                        ('xinv_rowdft_f64_dev', 6)):
        assert re.search(r'\bint\s+%s\s*\(' % name, sub) and len(re.findall(r'\b%s\s*\(' % name, hdr)) == 1, name
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == nargs
        proto = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, sub).group(1)
        assert len(proto.split(',')) == nargs, name
    assert _lib.PATH_FOURIER2D == 6 and re.search(r'#define\s+XINV_PATH_FOURIER2D\s+6\b', hdr)
    assert xa.rfft_rows is fourier.rfft_rows and xa.irfft_rows is fourier.irfft_rows


def test_build_lists_the_new_unit():
    from xinvert_amd import build
    assert ('xinv_tu_fourier', 'xinv_tu_fourier.hip', []) in build.UNITS
    assert os.path.exists(os.path.join(build.CSRC, 'xinv_fourier.h')) and '-ffp-contract=off' in build.BASE_FLAGS
    assert any(h.endswith('xinv_fourier.h') for h in build._abi_headers())
