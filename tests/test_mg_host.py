"""invert_MultiGrid on the host (no GPU): the level plan, coarse coordinates, prolongation tables and argument errors
(xinvert_amd/multigrid.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as M  # noqa: E402
from xinvert_amd import apps, multigrid as mg  # noqa: E402
from xinvert_amd import invert_MultiGrid, invert_Poisson, invert_GeoAdjustment, invert_RefStateSWM  # noqa: E402
from xinvert_amd.field import Field  # noqa: E402


def test_exported():
    import xinvert_amd
    assert xinvert_amd.invert_MultiGrid is mg.invert_MultiGrid


@pytest.mark.parametrize('lengths, BCs, ratio, gridNo, want', [
    ((1800, 3600), ('fixed', 'periodic'), 3, 3, [(9, 9), (3, 3), (1, 1)]),
    ((721, 1440), ('fixed', 'periodic'), 3, 3, [(9, 9), (3, 3), (1, 1)]),
    ((100, 100), ('fixed', 'fixed'), 2, 4, [(8, 8), (4, 4), (2, 2), (1, 1)]),
    # below 3 coarse points a dim is not coarsened at that level
    ((20, 100), ('fixed', 'fixed'), 3, 3, [(1, 9), (3, 3), (1, 1)]),
    ((26, 27), ('fixed', 'fixed'), 3, 3, [(1, 9), (3, 3), (1, 1)]),
    ((27, 27), ('fixed', 'fixed'), 3, 3, [(9, 9), (3, 3), (1, 1)]),
    # periodic: only where the ratio divides the length
    ((90, 100), ('fixed', 'periodic'), 3, 3, [(9, 1), (3, 1), (1, 1)]),
    ((90, 99), ('fixed', 'periodic'), 3, 3, [(9, 9), (3, 3), (1, 1)]),
    ((90, 102), ('extend', 'periodic'), 3, 3, [(9, 1), (3, 3), (1, 1)]),
    # a level that coarsens nothing is left out; one level is the plain solve
    ((8, 8), ('fixed', 'fixed'), 3, 3, [(1, 1)]),
    ((10, 10), ('fixed', 'fixed'), 3, 3, [(3, 3), (1, 1)]),
    ((100, 100), ('fixed', 'fixed'), 3, 1, [(1, 1)]),
    ((100, 100), ('fixed', 'fixed'), 1, 3, [(1, 1)]),
    ((9, 30, 60), ('fixed', 'fixed', 'periodic'), 3, 3, [(1, 9, 1), (3, 3, 3), (1, 1, 1)]),
])
def test_level_plan(lengths, BCs, ratio, gridNo, want):
    assert mg.level_ratios(lengths, BCs, ratio, gridNo) == want


def test_coarse_blocks_and_trimmed_tails():
    x = np.arange(11) * 0.5 + 1.0
    c = mg.coarse_coord(x, 3)                     # blocks [0..2], [3..5], [6..8]; 9, 10 belong to none
    assert np.array_equal(c, [1.5, 3.0, 4.5])
    v = np.arange(11.0)[None]
    assert np.array_equal(M.restrict(v, (3,), np.nan), [[1.0, 4.0, 7.0]])
    assert np.array_equal(mg.restrict_array(v, [(1, 3)]), [[1.0, 4.0, 7.0]])


@pytest.mark.parametrize('n, r', [(721, 9), (721, 3), (1440, 9), (3600, 9), (1800, 3), (100, 7), (64, 2)])
@pytest.mark.parametrize('kind', ['lat', 'lon', 'uniform', 'descending'])
def test_coarse_coordinates_are_uniform(n, r, kind):
    x = {'lat': np.linspace(-90.0, 90.0, n), 'lon': np.arange(n) * (360.0 / n),
         'uniform': np.arange(n) * 0.1 + 7.0, 'descending': 1000.0 - 12.5 * np.arange(n)}[kind]
    c = mg.coarse_coord(x, r)
    assert len(c) == n // r
    apps._uniform_interval(c, np.diff(c)[0], 'coarse')
    assert np.isclose(np.diff(c)[0], r * (x[1] - x[0]))


def _fine_coords(kind, n, periodic):
    if periodic:
        return {0: np.arange(n) * (360.0 / n), 1: np.arange(n) * (360.0 / n) - 180.0, 2: np.arange(n) * 0.7 + 3.0}[kind]
    return {0: np.arange(n) * 0.25 - 3.0, 1: np.linspace(-90.0, 90.0, n), 2: 1000.0 - 25.0 * np.arange(n)}[kind]


# (the pairs the level plan coarsens: n // r >= 3, and r | n on a periodic dim)
TABLE_CASES = [(n, r, p) for n in (9, 10, 11, 100, 721, 1440, 3600) for r in (2, 3, 9) for p in (False, True)
               if n // r >= 3 and not (p and n % r)]


@pytest.mark.parametrize('n, r, periodic', TABLE_CASES)
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_prolongation_tables_match_numpy_interp(n, r, periodic, kind):
    xf = _fine_coords(kind, n, periodic)
    xc = mg.coarse_coord(xf, r)
    lo, hi, w = mg.prolong_table(xf, xc, periodic)
    assert lo.dtype == hi.dtype == np.int64 and lo.shape == hi.shape == w.shape == (n,)
    assert lo.min() >= 0 and hi.min() >= 0 and lo.max() < len(xc) and hi.max() < len(xc)
    assert ((w >= 0) & (w <= 1)).all()
    rng = np.random.default_rng(n * 31 + r)
    for f in (1.0 + rng.random(len(xc)), np.sin(xc * 0.05) + 2.0):
        got = (1.0 - w) * f[lo] + w * f[hi]
        if periodic:
            ref = np.interp(xf, xc, f, period=n * (xf[1] - xf[0]))
        elif xc[0] > xc[-1]:                                  # (numpy.interp needs increasing coordinates)
            ref = np.interp(xf, xc[::-1], f[::-1])
        else:
            ref = np.interp(xf, xc, f)
        assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-15


def test_prolongation_clamps_and_wraps():
    xf = np.arange(12) * 1.0
    xc = mg.coarse_coord(xf, 3)                               # 1, 4, 7, 10
    lo, hi, w = mg.prolong_table(xf, xc, False)
    assert (lo[0], hi[0], w[0]) == (0, 0, 0.0) and (lo[11], hi[11], w[11]) == (3, 3, 0.0)
    lo, hi, w = mg.prolong_table(xf, xc, True)                # period 12: 11 and 0 lie between 10 and 1 (= 13)
    assert (lo[11], hi[11]) == (3, 0) and w[11] == 1.0 / 3.0
    assert (lo[0], hi[0]) == (3, 0) and w[0] == 2.0 / 3.0
    lo, hi, w = mg.prolong_table(xf, xf, False)               # a dim neither level coarsens
    assert np.array_equal(lo, np.arange(12)) and np.array_equal(hi, lo) and not w.any()


def test_model_prolongation_keeps_masked_and_edge_points():
    c = np.arange(12.0).reshape(1, 3, 4)
    f0 = np.full((1, 9, 12), -5.0)
    tabs = [mg.prolong_table(np.arange(9.0), mg.coarse_coord(np.arange(9.0), 3), False),
            mg.prolong_table(np.arange(12.0), mg.coarse_coord(np.arange(12.0), 3), True)]
    force = np.zeros((1, 9, 12))
    force[0, 4, 5] = -9.99e8
    out = M.prolong(c, f0, tabs, keep_edges=1, force=force)
    assert (out[0, 0] == -5.0).all() and (out[0, -1] == -5.0).all() and out[0, 4, 5] == -5.0
    assert out[0, 1, 1] == c[0, 0, 0] and out[0, 4, 4] == c[0, 1, 1]


def test_model_restriction_skips_undefined_points():
    v = np.array([[1.0, np.nan, 3.0, np.nan, np.nan, np.nan, 2.0]])
    assert np.array_equal(M.restrict(v, (3,), np.nan), [[2.0, np.nan]], equal_nan=True)
    w = np.where(np.isnan(v), -1.0, v)
    assert np.array_equal(M.restrict(w, (3,), -1.0), [[2.0, -1.0]])
    assert np.array_equal(mg.restrict_array(v, [(1, 3)]), M.restrict(v, (3,), np.nan), equal_nan=True)


def _poisson_field(ny=30, nx=60):
    lat = np.linspace(-60.0, 60.0, ny)
    lon = np.arange(nx) * (360.0 / nx)
    return Field(np.ones((ny, nx)), ('lat', 'lon'), {'lat': lat, 'lon': lon})


@pytest.mark.parametrize('app', [invert_GeoAdjustment, invert_RefStateSWM])
def test_one_dimensional_app_raises(app):
    F = Field(np.ones(30), ('lat',), {'lat': np.linspace(-60.0, 60.0, 30)})
    with pytest.raises(Exception, match='1-D app'):
        invert_MultiGrid(app, F, ['lat'])


@pytest.mark.parametrize('kw', [dict(gridNo=0), dict(gridNo=-1), dict(ratio=0), dict(gridNo=1.5)])
def test_bad_hierarchy_raises(kw):
    with pytest.raises(Exception, match='gridNo|ratio'):
        invert_MultiGrid(invert_Poisson, _poisson_field(), ['lat', 'lon'], iParams={'BCs': ['fixed', 'periodic']}, **kw)


@pytest.mark.parametrize('devices', [[0, 1], 'all'])
def test_several_devices_raise(devices):
    with pytest.raises(NotImplementedError):
        invert_MultiGrid(invert_Poisson, _poisson_field(), ['lat', 'lon'],
                         iParams={'BCs': ['fixed', 'periodic'], 'devices': devices})


def test_unknown_function_raises():
    with pytest.raises(Exception, match='not one of'):
        invert_MultiGrid(len, _poisson_field(), ['lat', 'lon'])
