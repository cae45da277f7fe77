"""The tridiagonal direct solver without a GPU: the numpy restatement (tests/tridiag_model.py) against the reference's own
trace / traceCyclic outputs bit for bit, its direct solution of the 1-D standard form against the reference's converged
SOR solutions (tests/golden/tridiag_cases.npz, std1d_cases.npz), the front end's errors, and the C-ABI names."""
import os
import re

import numpy as np
import pytest

import tridiag_model as M
import xinvert_amd as xa
from xinvert_amd import _lib, core, tridiag
from xinvert_amd.field import Field

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'tridiag_cases.npz'))


@pytest.fixture(scope='module')
def gold1d():
    return np.load(os.path.join(HERE, 'golden', 'std1d_cases.npz'))


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def rel_l2(a, b, undef):
    ok = b != undef                                           # over defined points
    return np.linalg.norm(a[ok] - b[ok]) / np.linalg.norm(b[ok])


def test_model_is_the_reference_bit_for_bit(gold):
    assert list(gold['tn']) == [2, 3, 4, 63, 64, 65, 181, 501, 1000]
    for p in ['pin_'] + ['t%d_' % k for k in range(len(gold['tn']))]:
        g = lambda k: gold[p + k]
        assert bits_equal(M.trace(g('a'), g('b'), g('c'), g('d')), g('x')), p
        assert bits_equal(M.traceCyclic(g('a'), g('b'), g('c'), g('d'), g('a0'), g('cn')), g('xc')), p


def test_model_batched_is_the_model_one_by_one(gold):
    g = lambda k: gold['t4_' + k]                             # n = 64
    rng = np.random.default_rng(0)
    d = rng.standard_normal((5, 64))
    b = g('b') + rng.uniform(0, 1, (5, 64)) * np.sign(g('b'))
    a0 = rng.uniform(-1, 1, 5)
    x, xc = M.trace(g('a'), b, g('c'), d), M.traceCyclic(g('a'), b, g('c'), d, a0, g('cn'))
    for m in range(5):
        assert bits_equal(x[m], M.trace(g('a'), b[m], g('c'), d[m]))
        assert bits_equal(xc[m], M.traceCyclic(g('a'), b[m], g('c'), d[m], a0[m], g('cn')))


def test_model_gives_the_answers_the_reference_test_prints(gold):
    g = lambda k: gold['pin_' + k]
    assert np.isclose(M.trace(g('a'), g('b'), g('c'), g('d')), g('expect')).all()
    assert np.isclose(M.traceCyclic(g('a'), g('b'), g('c'), g('d'), 5.2, 3.9), g('expect_cyc')).all()


def test_direct_solution_within_the_converged_field_contract(gold, gold1d):
    undef = float(gold['undef'])
    names = [str(n) for n in gold['names']]
    assert len(names) == 3 * 4 * 5 + 3 + 8
    for bc in M.BCS:
        assert '%s_icbc' % bc in names
        for xc in (5, 64, 65, 73):
            for mk in ('none', 'F', 'A', 'Alast', 'B'):
                assert '%s_%d_%s' % (bc, xc, mk) in names
    assert sum('_end_' in n for n in names) == 8
    for k, name in enumerate(names):
        p = 'c%d_' % k
        par = gold[p + 'par']
        S, fl = M.direct_solve(gold[p + 'S0'], gold[p + 'A'], gold[p + 'B'], gold[p + 'F'], int(par[0]), par[1], undef)
        assert fl[0] == 0 and np.isfinite(S).all(), name
        assert rel_l2(S, gold[p + 'S'], undef) < 1e-6, name
    for tag in ('geo', 'swm'):
        g = lambda k: gold1d['%s_%s' % (tag, k)]
        S, fl = M.direct_solve(np.zeros(len(g('lat'))), g('A'), g('B'), g('F'), str(g('BCx')), float(g('delxSqr')), undef)
        assert fl[0] == 0 and np.isfinite(S).all(), tag
        assert rel_l2(S, g('S'), undef) < 1e-6, tag


def test_periodic_masked_end_points_take_plain_trace(gold):
    undef = float(gold['undef'])
    names = [str(n) for n in gold['names']]
    for tag in ('F0', 'Flast', 'A0', 'Fboth'):
        k = names.index('periodic_64_end_' + tag)
        p = 'c%d_' % k
        s = M.assemble(gold[p + 'S0'], gold[p + 'A'], gold[p + 'B'], gold[p + 'F'], 'periodic', 0.49, undef)
        assert not s['cyc'][0], tag
    k = names.index('periodic_64_none')
    p = 'c%d_' % k
    assert M.assemble(gold[p + 'S0'], gold[p + 'A'], gold[p + 'B'], gold[p + 'F'], 'periodic', 0.49, undef)['cyc'][0]


def test_singular_and_nan_systems_report_overflow(gold1d):
    undef = float(gold1d['undef'])
    names = [str(n) for n in gold1d['names']]
    for bc in M.BCS:                                          # a NaN coefficient passes the predicate
        p = 'c%d_' % names.index('%s_nan' % bc)
        S, fl = M.direct_solve(gold1d[p + 'S0'], gold1d[p + 'A'], gold1d[p + 'B'], gold1d[p + 'F'], bc, 1.0, undef)
        assert fl[0] == 1 and list(fl[1:]) == [0, 0], bc
    xc = 16                                                   # all-Neumann with B = 0: singular
    S, fl = M.direct_solve(np.zeros(xc), np.ones(xc), np.zeros(xc), np.ones(xc), 'extend', 1.0, undef)
    assert fl[0] == 1 and not np.isfinite(S).all()


def test_length_and_argument_errors():
    one = np.ones(4)
    for f in (M.trace, tridiag.trace):
        with pytest.raises(Exception, match='lengths of given arrays are not satisfied'):
            f(np.ones(4), one, np.ones(3), one)
        with pytest.raises(Exception, match='lengths of given arrays are not satisfied'):
            f(np.ones(3), one, np.ones(3), np.ones(5))
    with pytest.raises(Exception, match='lengths of given arrays are not satisfied'):
        tridiag.traceCyclic(np.ones(3), one, np.ones(2), one, 1.0, 1.0)
    with pytest.raises(Exception, match='batch axes of the given arrays differ'):
        tridiag.trace(np.ones((2, 3)), np.ones((3, 4)), np.ones(3), one)
    assert xa.trace is tridiag.trace and xa.traceCyclic is tridiag.traceCyclic
    assert tridiag.trace(np.ones((0, 3)), np.ones((0, 4)), np.ones(3), one).shape == (0, 4)
    import torch                                              # numpy arrays with a tensor corner: refused by name
    with pytest.raises(_lib.XinvError, match='numpy arrays, or CUDA float64 tensors'):
        tridiag.traceCyclic(np.ones(3), one, np.ones(3), one, torch.tensor(0.5, dtype=torch.float64), 0.25)


def test_method_direct_is_the_1d_forms_alone():
    y, x = np.arange(8.0), np.arange(9.0)
    F = Field(np.zeros((8, 9)), ('lat', 'lon'), {'lat': y, 'lon': x})
    ip = dict(xa.default_iParams, method='direct')
    with pytest.raises(Exception, match="'direct' is available for the 1-D standard form only"):
        core.inv_standard2D(F, F, F, F, F, ['lat', 'lon'], ip)
    with pytest.raises(Exception, match="'direct' is available for the 1-D standard form only"):
        core.inv_general2D(F, F, F, F, F, F, F, F, ['lat', 'lon'], ip)
    with pytest.raises(Exception, match="must be 'sor' or 'direct'"):
        core.inv_standard1D(F, F, F, F, ['lat'], dict(ip, method='cg'))


def test_abi_names_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xinv.h')).read()
    sub = open(os.path.join(ROOT, 'include', 'xinv_trace.h')).read()      # (the prototypes: xinv.h includes it)
    assert re.search(r'^#include "xinv_trace.h"', hdr, flags=re.M)
    L = _lib.load()
    for name in ('xinv_tridiag_f64', 'xinv_tridiag_f64_dev'):
        assert re.search(r'\bint\s+%s\s*\(' % name, sub) and re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    assert _lib.PATH_DIRECT1D == 5 and re.search(r'#define\s+XINV_PATH_DIRECT1D\s+5\b', hdr)


def test_build_lists_the_new_unit():
    from xinvert_amd import build
    assert ('xinv_tu_tridiag', 'xinv_tu_tridiag.hip', []) in build.UNITS
    assert os.path.exists(os.path.join(build.CSRC, 'xinv_tridiag.h'))
