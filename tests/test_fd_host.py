"""Host side of the finite differences (xinvert_amd/finitediffs.py, utils.py): exports, padBCs, the numpy model against
apps._deriv_center, BC / fill handling, argument errors and loop_noncore.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_model as M  # noqa: E402
from xinvert_amd.field import Field  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _atmos():
    d = np.load(os.path.join(HERE, 'golden', 'poisson_atmos.npz'))
    return Field(np.asarray(d['S60_ep'][0]), ('lat', 'lon'), {'lat': d['lat'], 'lon': d['lon']})


def test_the_five_names_import_from_the_package():
    from xinvert_amd import FiniteDiff, deriv, deriv2, padBCs, loop_noncore   # noqa: F401
    import xinvert_amd
    for name in ('FiniteDiff', 'deriv', 'deriv2', 'padBCs', 'loop_noncore'):
        assert callable(getattr(xinvert_amd, name))


def test_padBCs_as_the_reference_test_asserts():
    # reference tests/test_FDs.py:24-37, on the lat-lon grid of the Poisson fixture
    from xinvert_amd import padBCs
    T = _atmos()
    T_Px = padBCs(T, dim='lon', BCs=('fixed', 'fixed'), fill=(1, 1))
    T_Py = padBCs(T, dim='lat', BCs=('extend', 'fixed'), fill=(2, 2))
    T_Py2 = padBCs(T, dim='lat', BCs=('periodic', 'periodic'))
    T_Py3 = padBCs(T, dim='lat', BCs=('reflect', 'extend'), fill=(3, 3))
    assert T_Px.shape == (73, 146) and T_Py.shape == (75, 144)
    assert (T_Px.values[:, 0] == 1).all() and (T_Px.values[:, -1] == 1).all()
    assert (T_Py.values[0] == T_Py.values[1]).all()
    assert (T_Py.values[-1] == 2).all()
    assert (T_Py2.values[1] == T_Py2.values[-1]).all()
    assert (T_Py2.values[-2] == T_Py2.values[0]).all()
    assert (T_Py3.values[0] == T_Py3.values[2]).all()
    assert (T_Py3.values[-1] == T_Py3.values[-2]).all()
    # the padded coordinate is extrapolated linearly at both ends
    lat = np.asarray(T['lat'], np.float64)
    assert T_Py['lat'][0] == lat[0] * 2 - lat[1] and T_Py['lat'][-1] == lat[-1] * 2 - lat[-2]
    assert np.array_equal(T_Py['lat'][1:-1], lat)
    # and the numpy model pads the same way
    assert np.array_equal(M.pad(T.values, 0, ('reflect', 'extend')), T_Py3.values)


def test_padBCs_takes_ndarray_with_dims_and_str_BCs():
    from xinvert_amd import padBCs
    a = np.arange(12.0).reshape(3, 4)
    p = padBCs(a, 'x', 'periodic', dims=('y', 'x'))
    assert isinstance(p, np.ndarray) and np.array_equal(p, np.pad(a, [(0, 0), (1, 1)], mode='wrap'))
    p = padBCs(a, 'y', ['fixed', 'reflect'], fill=(7, 8), dims=('y', 'x'))
    assert (p[0] == 7).all() and np.array_equal(p[-1], a[1])


@pytest.mark.parametrize('BC', ['fixed', 'extend', 'reflect', 'periodic'])
@pytest.mark.parametrize('axis', [0, 1])
def test_model_equals_cal_flow_deriv_center(BC, axis):
    from xinvert_amd.apps import _deriv_center
    rng = np.random.default_rng(3)
    lat = np.linspace(-80, 80, 33)
    lev = np.array([1000., 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30, 20, 10])
    for coord in (lat, lev):
        n = coord.size
        shape = (n, 7) if axis == 0 else (7, n)
        dims = ('a', 'b')
        coords = {dims[axis]: coord}
        f = Field(rng.standard_normal(shape), dims, coords)
        scale = 1.7
        mine = M.deriv(f, dims[axis], (BC, BC), (0.5, 0.5), scale)
        theirs = _deriv_center(f.values, axis, coord, BC, scale, fill=0.5)
        assert np.array_equal(mine, theirs, equal_nan=True)


def test_FiniteDiff_normalises_BCs_and_fill():
    from xinvert_amd import FiniteDiff
    dm = {'T': 'time', 'Z': 'lev', 'Y': 'lat', 'X': 'lon'}
    fd = FiniteDiff(dm)
    assert fd.BCs == {d: ('extend', 'extend') for d in dm} and fd.fill == {d: (0, 0) for d in dm}
    fd = FiniteDiff(dm, BCs='periodic', fill=2.5)
    assert fd.BCs == {d: ('periodic', 'periodic') for d in dm} and fd.fill == {d: (2.5, 2.5) for d in dm}
    user_bcs = {'Y': 'reflect', 'X': ('fixed', 'extend')}
    user_fill = {'X': (1, 2)}
    fd = FiniteDiff(dm, BCs=user_bcs, fill=user_fill, coords='cartesian')
    assert fd.BCs == {'T': ('extend', 'extend'), 'Z': ('extend', 'extend'), 'Y': ('reflect', 'reflect'),
                      'X': ('fixed', 'extend')}
    assert fd.fill == {'T': (0, 0), 'Z': (0, 0), 'Y': (0, 0), 'X': (1, 2)}
    assert user_bcs == {'Y': 'reflect', 'X': ('fixed', 'extend')}        # (the caller's dict is left alone)
    fd = FiniteDiff(dm, BCs=None, fill=None)
    assert fd.BCs['Z'] == ('extend', 'extend') and fd.fill['Z'] == (0, 0)
    assert "'cartesian' coords" in repr(FiniteDiff(dm, coords='cartesian'))


def test_per_call_BCs_and_fill_override():
    from xinvert_amd.finitediffs import _overwriteBCs, _overwriteFills
    old = {'Y': ('extend', 'extend'), 'X': ('periodic', 'periodic')}
    assert _overwriteBCs(None, old) is old
    assert _overwriteBCs('fixed', old) == {'Y': ('fixed', 'fixed'), 'X': ('fixed', 'fixed')}
    assert _overwriteBCs({'Y': 'reflect', 'Q': 'fixed'}, old) == {'Y': ('reflect', 'reflect'),
                                                                   'X': ('periodic', 'periodic')}
    assert _overwriteBCs({'Y': ['fixed', 'extend']}, old)['Y'] == ['fixed', 'extend']
    assert old == {'Y': ('extend', 'extend'), 'X': ('periodic', 'periodic')}
    fo = {'Y': (0, 0), 'X': (1, 1)}
    assert _overwriteFills(None, fo) is fo
    assert _overwriteFills(3, fo) == {'Y': (3, 3), 'X': (3, 3)}
    assert _overwriteFills({'X': (4, 5), 'Q': 1}, fo) == {'Y': (0, 0), 'X': (4, 5)}


def test_argument_errors():
    from xinvert_amd import FiniteDiff, deriv, deriv2, padBCs
    T = _atmos()
    with pytest.raises(Exception, match="'periodic' cannot be mixed with other BCs"):
        padBCs(T, 'lat', ('periodic', 'fixed'))
    with pytest.raises(Exception, match="'periodic' cannot be mixed with other BCs"):
        deriv(T, 'lat', ('extend', 'periodic'))
    with pytest.raises(Exception, match='unsupported BC'):
        deriv2(T, 'lat', ('extend', 'extrapolate'))
    with pytest.raises(Exception, match='unsupported scheme: upwind'):
        deriv(T, 'lat', scheme='upwind')
    with pytest.raises(Exception, match='unsupported coords: sphere'):
        FiniteDiff({'Y': 'lat', 'X': 'lon'}, coords='sphere')
    fd = FiniteDiff({'Y': 'lat', 'X': 'lon'})
    with pytest.raises(Exception, match='lengths of vector and dims are not equal'):
        fd.divg([T, T], ['X'])
    with pytest.raises(Exception, match='invalid component'):
        FiniteDiff({'Z': 'lat', 'Y': 'lat', 'X': 'lon'}, coords='cartesian').vort(u=T, v=T, components='q')
    # datetime coordinate
    t = np.arange('2000-01-01', '2000-01-05', dtype='datetime64[D]')
    F = Field(np.zeros((4, 3)), ('time', 'x'), {'time': t})
    with pytest.raises(TypeError, match='datetime'):
        deriv(F, 'time')
    with pytest.raises(TypeError, match='datetime'):
        padBCs(F, 'time', 'extend')
    for meth, line in (('shear_strain', ':488'), ('deformation_rate', ':516'), ('Okubo_Weiss', ':542')):
        with pytest.raises(NotImplementedError, match=line):
            getattr(fd, meth)(T, T)


def test_loop_noncore():
    from xinvert_amd import loop_noncore
    F = Field(np.zeros((2, 3, 4)), ('time', 'lat', 'lon'),
              {'time': np.array([10., 20.]), 'lat': np.array([-1., 0., 1.])})
    assert list(loop_noncore(F, ['time', 'lat', 'lon'])) == [{}]
    assert list(loop_noncore(F, ['lat', 'lon'])) == [{'time': 10.}, {'time': 20.}]
    got = list(loop_noncore(F, ['lon']))
    assert got == [{'time': a, 'lat': b} for a in (10., 20.) for b in (-1., 0., 1.)]
    assert list(loop_noncore(F, 'lon')) == got
