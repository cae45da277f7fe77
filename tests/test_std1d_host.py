"""The 1-D standard form without a GPU: the lexicographic model against the reference's own outputs (bit for bit), the
red-black model against the same fixed point, the front end's parameters and errors, and the C-ABI names."""
import os
import re

import numpy as np
import pytest

import std1d_model as M
from xinvert_amd import _lib, apps, core
from xinvert_amd.field import Field

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BCS = ['fixed', 'extend', 'periodic']


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'std1d_cases.npz'))


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def test_lexicographic_model_reproduces_every_golden_case(gold):
    undef = float(gold['undef'])
    names = list(gold['names'])
    assert len(names) >= 135
    for k, name in enumerate(names):
        p = 'c%d_' % k
        par = gold[p + 'par']
        S, fl = M.lex_solve(gold[p + 'S0'], gold[p + 'A'], gold[p + 'B'], gold[p + 'F'], BCS[int(par[0])], par[1],
                            par[2], undef, int(par[3]), par[4])
        assert bits_equal(S, gold[p + 'S']), name
        assert bits_equal(fl, gold[p + 'flags']), name


def test_golden_matrix_covers_the_issue_cases(gold):
    names = [str(n) for n in gold['names']]
    for bc in BCS:
        for tag in ('nan', 'zero', 'icbc'):
            assert '%s_%s' % (bc, tag) in names
    k = names.index('fixed_nan')
    assert gold['c%d_flags' % k][0] == 1.0                   # overflow
    k = names.index('extend_zero')
    assert gold['c%d_flags' % k][2] == 0.0                   # norm == 0 stop at loop 0


def test_red_black_model_reaches_the_reference_fixed_point(gold):
    g = lambda k: gold['swm_' + k]
    S, fl = M.rb_solve(np.zeros(len(g('lat'))), g('A'), g('B'), g('F'), 'fixed', float(g('delxSqr')),
                       float(g('optArg')), -9.99e8, 20000, 1e-14)
    assert fl[0] == 0
    assert np.linalg.norm(S - g('S')) / np.linalg.norm(g('S')) < 1e-6


def test_kernel_norm_order_is_a_function_of_xc():
    rng = np.random.default_rng(0)
    for xc in (3, 128, 129, 513, 8192):
        S = rng.standard_normal(xc)
        n = M.kernel_norm(S, -9.99e8)
        assert abs(n - np.abs(S).mean()) <= 1e-14 * abs(n)
    assert M.shape(512) == (8, 1) and M.shape(513) == (8, 2) and M.shape(M.MAX_XC) == (8, 16)


def test_golden_geoadjustment_residual(gold):
    g = lambda k: gold['geo_' + k]
    A, B, F, s, d = g('A'), g('B'), g('F'), g('S'), float(g('delxSqr'))
    r = (A[2:] * (s[2:] - s[1:-1]) - A[1:-1] * (s[1:-1] - s[:-2])) / d + (B[1:-1] * s[1:-1] - F[1:-1])
    assert np.linalg.norm(r) / np.linalg.norm(F[1:-1]) <= 1e-9


def test_geoadjustment_coefficients_restate_the_generator(gold):
    lat = gold['geo_lat']
    h0 = Field(gold['geo_h0'], ('lat',), {'lat': lat})
    ip = apps._update(apps.default_iParams, {'undef': -9999})
    F, S0, (A, B) = apps._coeffs_GeoAdjustment(h0, ['lat'], 'lat', apps.default_mParams, ip, None)
    assert bits_equal(A, gold['geo_A']) and bits_equal(B, gold['geo_B']) and bits_equal(F.values, gold['geo_F'])
    assert np.isnan(A[0])                                     # the half-grid shift


def test_refstateswm_coefficients_restate_the_generator(gold):
    lat = gold['swm_lat']
    Q = Field(gold['swm_Q'], ('lat',), {'lat': lat})
    mp = dict(apps.default_mParams, M0=Field(gold['swm_M0'], ('lat',), {'lat': lat}),
              C0=Field(gold['swm_C0'], ('lat',), {'lat': lat}))
    F, S0, (A, B) = apps._coeffs_RefStateSWM(Q, ['lat'], 'lat', mp, apps._update(apps.default_iParams, {}), None)
    assert bits_equal(A, gold['swm_A']) and bits_equal(B, gold['swm_B']) and bits_equal(F.values, gold['swm_F'])


def test_cal_params1D_values_and_errors():
    lat = np.linspace(-75, -25, 501)
    p = apps._cal_params1D(lat, 'lat')
    del1 = np.deg2rad(0.1) * 6371200.0
    eps = np.sin(np.pi / (2.0 * 501 + 2.0)) ** 2
    assert p['gc1'] == 501 and np.isclose(p['del1'], del1) and p['del1Sqr'] == p['del1'] ** 2.0
    assert p['optArg'] == 2.0 / (1.0 + np.sqrt((2.0 - eps) * eps))
    assert list(p['flags']) == [0.0, 1.0, 0.0]
    with pytest.raises(Exception, match='unsupported coords for 2D case: cartesian'):
        apps._cal_params1D(lat, 'cartesian')
    with pytest.raises(Exception, match='non-uniform'):
        apps._cal_params1D(np.r_[lat[:-1], lat[-1] + 1.0], 'lat')


def test_front_end_errors_before_any_device_work():
    lat = np.linspace(-60, -20, 41)
    h0 = Field(np.full(41, 1500.0), ('lat',), {'lat': lat})
    with pytest.raises(Exception, match='1 dimensional forcing are needed'):
        apps.invert_GeoAdjustment(h0, dims=['lat', 'lon'])
    with pytest.raises(Exception, match='not supported for cartesian coordinates'):
        apps.invert_GeoAdjustment(h0, dims=['lat'], coords='cartesian')
    with pytest.raises(Exception, match='not supported for cartesian coordinates'):
        apps.invert_RefStateSWM(h0, dims=['lat'], coords='cartesian', mParams={'M0': h0, 'C0': 1.0})
    bad = Field(np.full(41, 1500.0), ('lat',), {'lat': np.r_[lat[:-1], 30.0]})
    with pytest.raises(Exception, match='non-uniform'):
        apps.invert_GeoAdjustment(bad, dims=['lat'])
    with pytest.raises(Exception, match='1 dimensions are needed for inversion'):
        core.inv_standard1D(h0, h0, h0, h0, ['lat', 'lon'], {})
    with pytest.raises(Exception, match='is not used'):
        apps.invert_GeoAdjustment(h0, dims=['lat'], mParams={'beta': 1.0})


def test_abi_names_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xinv.h')).read()
    for name in ('xinv_standard_1d_f64', 'xinv_standard_1d_f64_batched', 'xinv_standard_1d_f64_dev'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTS
    assert _lib.PATH_WAVE1D == 4 and '#define XINV_PATH_WAVE1D 4' in hdr
