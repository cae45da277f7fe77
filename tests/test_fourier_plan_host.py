"""Fourier plans without a GPU ("Plans"): the numpy restatement of k_fourier_factor / k_fourier_subst
(tests/fourier_plan_model.py) gives the BITS of the one-shot restatement (tests/fourier_model.py) -- the stored-factor march
with the real and imaginary parts separated is the same sequence of float64 operations --, the C-ABI names, and the words
with which ResidentProblem.solve_fourier refuses a batch outside the path's scope.
"""
import inspect
import os
import re

import numpy as np
import pytest

import fourier_model as M
import fourier_plan_model as PM
import xinvert_amd as xa
from xinvert_amd import _lib, fourier, resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = -9.99e8
SHAPES = [(7, 12), (16, 20), (37, 45)]


def case(yc, xc, grid, shared, nb=3):
    """-> (S0, F [nb, yc, xc], A, C [yc] or [nb, yc], delxSqr, ratioSqr)"""
    rng = np.random.default_rng(1000 * yc + xc + (7 if shared else 0))
    if grid == 'latlon':
        lat = np.deg2rad(np.linspace(-80.0, 80.0, yc))
        A, C = np.cos(lat), 1.0 / np.cos(lat)
        dlat, dlon = np.deg2rad(160.0 / (yc - 1)), 2 * np.pi / xc
        delxSqr, ratioSqr = (6371200.0 * dlon) ** 2, (dlon / dlat) ** 2
        if not shared:
            w = 1.0 + 0.125 * np.arange(nb)[:, None]
            A, C = A * w, C / w
    else:
        shape = (yc,) if shared else (nb, yc)
        A, C = rng.uniform(0.5, 1.5, shape), rng.uniform(0.5, 1.5, shape)
        delxSqr, ratioSqr = 1.21, (1.1 / 1.3) ** 2
    F = rng.standard_normal((nb, yc, xc))
    S0 = rng.standard_normal((nb, yc, xc)) * np.abs(F).max() * delxSqr
    return S0, F, A, C, delxSqr, ratioSqr


@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-member'])
@pytest.mark.parametrize('grid', ['latlon', 'cartesian'])
@pytest.mark.parametrize('yc,xc', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_stored_factor_march_has_the_one_shots_bits(yc, xc, grid, shared):
    S0, F, A, C, delxSqr, ratioSqr = case(yc, xc, grid, shared)
    ref, flr = M.solve(S0, A, C, F, delxSqr, ratioSqr, U)
    _, lam = M.tables(xc)
    fac = PM.factor(A, C, ratioSqr, lam)
    assert fac[0].shape == (1 if shared else 3, yc, xc // 2 + 1)
    S, fl, bad = PM.solve(S0, F, delxSqr, ratioSqr, fac, A, C, U)
    assert not bad.any() and np.array_equal(fl, flr) and not fl.any()
    assert np.array_equal(S, ref)
    # the factors once, another forcing: again the one-shot's bits; one forcing for all members too
    F2 = F[::-1] * 3.0
    assert np.array_equal(PM.solve(S0, F2, delxSqr, ratioSqr, fac, A, C, U)[0], M.solve(S0, A, C, F2, delxSqr, ratioSqr, U)[0])
    one = np.broadcast_to(F[1], F.shape)
    assert np.array_equal(PM.solve(S0, F[1], delxSqr, ratioSqr, fac, A, C, U)[0], M.solve(S0, A, C, one, delxSqr, ratioSqr, U)[0])


def test_model_factors_are_the_one_shots_forward_factors():
    S0, F, A, C, delxSqr, ratioSqr = case(16, 20, 'cartesian', False)
    _, lam = M.tables(20)
    inv, gam = PM.factor(A, C, ratioSqr, lam)
    lo, up, di = M.system(A, C, ratioSqr, lam)
    gp = np.zeros((3, lam.size))
    for j in range(1, 15):
        i = 1.0 / (di[:, j] if j == 1 else di[:, j] - lo[:, j, None] * gp)
        gp = up[:, j, None] * i
        assert np.array_equal(inv[:, j], i) and np.array_equal(gam[:, j], gp)
    assert not inv[:, [0, -1]].any() and not gam[:, [0, -1]].any()


def test_model_skips_the_member_with_undef_and_flags_nan_alone():
    S0, F, A, C, delxSqr, ratioSqr = case(7, 12, 'cartesian', False)
    _, lam = M.tables(12)
    fac = PM.factor(A, C, ratioSqr, lam)
    good = PM.solve(S0, F, delxSqr, ratioSqr, fac, A, C, U)[0]
    Fb = F.copy()
    Fb[1, 3, 5] = U
    S, fl, bad = PM.solve(S0, Fb, delxSqr, ratioSqr, fac, A, C, U)
    assert bad.tolist() == [0, 1, 0]
    assert np.array_equal(S[1], S0[1]) and np.array_equal(S[[0, 2]], good[[0, 2]])
    Fn = F.copy()
    Fn[2, 2, 2] = np.nan
    S, fl, bad = PM.solve(S0, Fn, delxSqr, ratioSqr, fac, A, C, U)
    assert fl[:, 0].tolist() == [0, 0, 1] and not bad.any() and np.array_equal(S[[0, 1]], good[[0, 1]])
    An = A.copy()
    An[0, 3] = np.nan
    S, fl, bad = PM.solve(S0, F, delxSqr, ratioSqr, PM.factor(An[0], C[0], ratioSqr, lam), An[0], C[0], U)
    assert fl[:, 0].tolist() == [1, 1, 1]                      # shared coefficients: every member's flag


# ------------------------------------------------------------------ C-ABI
PLAN_ABI = (('xinv_fourier_plan_create_standard_2d_f64_dev', 11), ('xinv_fourier_plan_solve_f64_dev', 6),
            ('xinv_fourier_plan_status', 3), ('xinv_fourier_plan_destroy', 1))


def test_plan_abi_names_declared_typed_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xinv.h')).read()
    sub = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'xinv_fourier.h')).read(), flags=re.S)
    assert re.search(r'typedef\s+struct\s+xinv_fourier_plan\s+xinv_fourier_plan\s*;', sub)
    L = _lib.load()
    for name, nargs in PLAN_ABI:
        proto = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, sub)
        assert proto and len(proto.group(1).split(',')) == nargs, name
        assert len(re.findall(r'\b%s\s*\(' % name, hdr)) == 1, name
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == nargs, name
        assert getattr(L, name).restype is not None
    src = open(os.path.join(ROOT, 'xinvert_amd', 'csrc', 'xinv_fourier.h')).read()
    for kernel in ('k_fourier_factor', 'k_fourier_subst'):
        assert re.search(r'__global__ void __launch_bounds__\(\w+\) %s\(' % kernel, src), kernel
    assert re.search(r'const int \*skip;', src)
    assert xa.FourierPlan is fourier.FourierPlan
    for method in ('solve', 'status', 'close'):
        assert callable(getattr(fourier.FourierPlan, method))


def test_the_entries_refuse_a_dead_plan_and_bad_arguments_before_any_device_call():
    """The argument checks come first, so they answer without a GPU."""
    import ctypes
    L = _lib.load()
    err = lambda: L.xinv_last_error().decode()
    flags = np.zeros((1, 3))
    assert L.xinv_fourier_plan_solve_f64_dev(None, None, None, 0, 0, None) == -1 and 'not a live plan' in err()
    assert L.xinv_fourier_plan_status(None, _lib.hptr(flags), None) == -1 and 'not a live plan' in err()
    assert L.xinv_fourier_plan_destroy(None) == 0
    h = ctypes.c_void_p()
    one = ctypes.c_void_p(8)                                  # (never dereferenced: the checks below come first)
    create = lambda nb, st, yc, xc: L.xinv_fourier_plan_create_standard_2d_f64_dev(
        ctypes.byref(h), one, one, nb, _lib.strides_arg(st), yc, xc, 1.0, 1.0, U, None)
    assert create(0, [0, 0], 5, 12) == -1 and 'nbatch < 1' in err()
    assert create(1, [0, 0], 2, 12) == -1 and 'every core dimension needs at least 3 points' in err()
    assert create(2, [0, -1], 5, 12) == -1 and 'negative batch stride' in err()
    assert create(2, [4, 0], 5, 12) == -1 and 'batch stride must be 0 (shared; not S) or at least one member' in err()
    assert create(2, [5, 0], 5, 14) == -1 and 'the row length 14 has the prime factor 7' in err()
    assert create(2, [5, 5], 5, 4500) == -1 and "beyond the transform's LDS budget" in err()
    assert L.xinv_fourier_plan_create_standard_2d_f64_dev(ctypes.byref(h), None, one, 1, _lib.strides_arg([0, 0]), 5, 12, 1.0,
                                                          1.0, U, None) == -1 and 'null array' in err()
    assert h.value is None


# ------------------------------------------------------------------ ResidentProblem.solve_fourier: the refusals
REFUSED = {
    'non-zero B': (dict(B_nonzero=True), r'B must be identically zero \(the array B is not\)'),
    'extend y': (dict(BCy='extend'), r"BCs must be \['fixed', 'periodic'\] \(the boundary code along y is 'extend'\)"),
    'fixed x': (dict(BCx='fixed'), r"BCs must be \['fixed', 'periodic'\] \(the boundary code along x is 'fixed'\)"),
    'A varies along x': (dict(varies=('A',)), r'A must be constant along x \(the array A varies along it\)'),
    'C varies along x': (dict(varies=('C',)), r'C must be constant along x \(the array C varies along it\)'),
    'xc = 14': (dict(xc=14), r'the row length 14 has the prime factor 7 \(the transform takes products of 2, 3 and 5\)'),
}


@pytest.mark.parametrize('name', list(REFUSED))
def test_resident_eligibility_refuses_by_the_front_ends_words(name):
    over, pattern = REFUSED[name]
    ok = dict(kind='std2d', B_nonzero=False, BCy='fixed', BCx='periodic', varies=(), yc=9, xc=12)
    fourier.resident_eligible(**ok)
    with pytest.raises(Exception, match=pattern) as ei:
        fourier.resident_eligible(**dict(ok, **over))
    assert "'sor' solves this case" in str(ei.value)


def test_resident_eligibility_order_and_other_kinds():
    ok = dict(kind='std2d', B_nonzero=False, BCy='fixed', BCx='periodic', varies=(), yc=9, xc=12)
    with pytest.raises(_lib.XinvError, match="not for kind 'gen2d'"):
        fourier.resident_eligible(**dict(ok, kind='gen2d'))
    # the order of fourier.eligible: B, the boundary codes, A, C, the row length
    with pytest.raises(Exception, match='B must be identically zero'):
        fourier.resident_eligible(**dict(ok, B_nonzero=True, BCy='extend', varies=('A', 'C'), xc=14))
    with pytest.raises(Exception, match="along y is 'extend'"):
        fourier.resident_eligible(**dict(ok, BCy='extend', BCx='fixed', varies=('A',), xc=14))
    with pytest.raises(Exception, match='A must be constant'):
        fourier.resident_eligible(**dict(ok, varies=('C', 'A'), xc=14))
    src = inspect.getsource(resident.ResidentProblem.solve_fourier) + inspect.getsource(resident.ResidentProblem._fourier_plan)
    assert 'resident_eligible' in src and 'FourierPlan' in src
    assert callable(resident.ResidentProblem.fourier_status)


def test_a_plan_asks_for_the_gpu():
    """No CPU fallback: without a device the constructor says so; with one it builds the plan."""
    try:
        plan = xa.FourierPlan(np.ones(5), np.ones(5), 1, 5, 12, 1.0, 1.0)
    except _lib.XinvError as e:
        assert 'no CPU fallback' in str(e), e
    else:
        plan.close()
