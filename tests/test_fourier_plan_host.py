"""Fourier plans without a GPU ("Plans"): the numpy restatement of k_fourier_factor / k_fourier_subst
(tests/fourier_plan_model.py) gives the BITS of the one-shot restatement (tests/fourier_model.py) -- the stored-factor march
with the real and imaginary parts separated is the same sequence of float64 operations --, the C-ABI names, the argument checks
of the plan entries, of the four one-shot entries and of xinv_rowdft_f64_dev (all answered before any device call), and the
words with which ResidentProblem.solve_fourier refuses a batch outside the path's scope.
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


# ------------------------------------------------------------------ the one-shot entries and the row transform
# Every refusal below is answered before the first device call: the device addresses are dummies that are never
# dereferenced, the host arrays of the _batched entries are small.  (nper: the per-row coefficient arrays between S and the
# forcing; letters: how the stride rule names them.)
FORMS = {'standard': (2, 'A, C', 'A and C', 2), 'general': (5, 'A, C, D, E, F', 'A, C, D, E and F', 4)}
STRIDE_RULE = 'batch stride must be 0 (shared; not S) or at least one member (%s: one value per row)'
LDS = "the row length 4500 is beyond the transform's LDS budget (at most 4096 points)"
PRIME = 'the row length 14 has the prime factor 7 (the transform takes products of 2, 3 and 5)'


def _strides(nper, yc, xc, **over):
    st = [yc * xc] + [yc] * nper + [yc * xc]
    for k, v in over.items():
        st[{'S': 0, 'coef': 1, 'last_coef': nper, 'forcing': nper + 1}[k]] = v
    return st


# name -> (keyword arguments of `dev_entry`, the message); the later cases are wrong in two ways and report the earlier one
DEV_REFUSED = {
    'null coefficient': (dict(null=1), 'null array'),
    'null forcing': (dict(null=-1), 'null array'),
    'null S': (dict(null=0), 'null array'),
    'null strides': (dict(no_strides=True), 'null strides'),
    'nbatch = 0': (dict(nb=0), 'nbatch < 1'),
    'yc = 2': (dict(yc=2), 'every core dimension needs at least 3 points'),
    'negative stride': (dict(nb=2, over=dict(coef=-1)), 'negative batch stride'),
    'S shared': (dict(nb=2, over=dict(S=0)), STRIDE_RULE),
    'S too close': (dict(nb=2, over=dict(S=5 * 12 - 1)), STRIDE_RULE),
    'coefficient too close': (dict(nb=2, over=dict(last_coef=5 - 1)), STRIDE_RULE),
    'forcing too close': (dict(nb=2, over=dict(forcing=5 * 12 - 1)), STRIDE_RULE),
    'xc = 14': (dict(xc=14), PRIME),
    'xc = 4500': (dict(xc=4500), LDS),
    'null array before null strides': (dict(null=1, no_strides=True), 'null array'),
    'null strides before nbatch': (dict(no_strides=True, nb=0), 'null strides'),
    'core dimension before the strides': (dict(nb=2, yc=2, over=dict(coef=-1)), 'every core dimension needs at least 3 points'),
    'stride rule before the row length': (dict(nb=2, xc=14, over=dict(S=0)), STRIDE_RULE),
}


def dev_entry(L, form, nb=1, yc=5, xc=12, null=None, no_strides=False, over={}):
    import ctypes
    nper = FORMS[form][0]
    arrays = [ctypes.c_void_p(8)] * (nper + 2)
    if null is not None:
        arrays[null] = None
    flags = np.zeros((max(nb, 1), 3))
    st = None if no_strides else _lib.strides_arg(_strides(nper, yc, xc, **over))
    fn = getattr(L, 'xinv_fourier_%s_2d_f64_dev' % form)
    return fn(*arrays, nb, st, yc, xc, *([1.0] * FORMS[form][3]), U, _lib.hptr(flags), None)


@pytest.mark.parametrize('name', list(DEV_REFUSED))
@pytest.mark.parametrize('form', list(FORMS))
def test_the_device_entries_refuse_bad_arguments_before_any_device_call(form, name):
    kw, msg = DEV_REFUSED[name]
    L = _lib.load()
    assert dev_entry(L, form, **kw) == -1
    err = L.xinv_last_error().decode()
    assert err == 'xinv_fourier: ' + (msg % FORMS[form][1] if '%s' in msg else msg)


@pytest.mark.parametrize('form', list(FORMS))
def test_a_valid_device_call_gets_as_far_as_the_device(form):
    """Past the checks the entry asks HIP for the current device: without one that is XINV_ERR_HIP (-2), not an argument
    error.  (With a device the dummy addresses would be read: the call is made only where there is none.)"""
    L = _lib.load()
    if L.xinv_device_count() >= 1:
        pytest.skip('a device is present: the call would read the dummy addresses')
    assert dev_entry(L, form) == -2
    assert dev_entry(L, form, nb=2) == -2


def host_entry(L, form, nb=1, yc=5, xc=12, over={}, **opt):
    nper = FORMS[form][0]
    arrays = [np.ones((nb, yc, xc))] + [np.ones((nb, yc))] * nper + [np.ones((nb, yc, xc))]
    flags = np.zeros((nb, 3))
    fn = getattr(L, 'xinv_fourier_%s_2d_f64_batched' % form)
    return fn(*[_lib.hptr(a) for a in arrays], nb, _lib.strides_arg(_strides(nper, yc, xc, **over)), yc, xc,
              *([1.0] * FORMS[form][3]), U, _lib.hptr(flags), _lib.options(**opt))


MASKS = 'float64 arrays only, %s one value per row (f32_mask, prep_flags and rowconst_mask must be 0)'
HOST_REFUSED = {
    'ndev = 2': (dict(devices=[0, 1]), 'one device only (xinv_options.ndev must be 0 or 1)'),
    'f32_mask': (dict(f32_mask=1), MASKS),
    'rowconst_mask': (dict(rowconst_mask=2), MASKS),
    'xc = 14': (dict(xc=14), PRIME),
    'the arguments before the options': (dict(nb=2, over=dict(S=0), devices=[0, 1]), STRIDE_RULE),
    'ndev before the masks': (dict(devices=[0, 1], f32_mask=1), 'one device only (xinv_options.ndev must be 0 or 1)'),
    'the masks before the row length': (dict(f32_mask=1, xc=14), MASKS),
}


@pytest.mark.parametrize('name', list(HOST_REFUSED))
@pytest.mark.parametrize('form', list(FORMS))
def test_the_host_entries_refuse_options_and_the_row_length_before_asking_for_a_device(form, name):
    kw, msg = HOST_REFUSED[name]
    L = _lib.load()
    assert host_entry(L, form, **kw) == -1                    # (XINV_ERR_ARG, also where there is no device)
    err = L.xinv_last_error().decode()
    assert err == 'xinv_fourier: ' + (msg % FORMS[form][2 if msg is MASKS else 1] if '%s' in msg else msg)


@pytest.mark.parametrize('form', list(FORMS))
def test_a_valid_host_call_without_a_device_is_nodev(form):
    L = _lib.load()
    if L.xinv_device_count() >= 1:
        pytest.skip('a device is present: the call would be a solve, not XINV_ERR_NODEV')
    assert host_entry(L, form, nb=2) == -3
    assert L.xinv_last_error().decode() == 'no HIP device available'


ROWDFT_REFUSED = {
    'null out': (dict(out=None), 'null array'),
    'null in': (dict(inp=None), 'null array'),
    'in place': (dict(inp=8), 'the transform is not in place'),
    'nrows = 0': (dict(nrows=0), 'nrows < 1'),
    'n = 1': (dict(n=1), 'a row needs at least 2 points, got 1'),
    'n = 14': (dict(n=14), PRIME),
    'n = 8192': (dict(n=8192), "the row length 8192 is beyond the transform's LDS budget (at most 4096 points)"),
    'null before in place': (dict(out=None, inp=None), 'null array'),
    'in place before nrows': (dict(inp=8, nrows=0), 'the transform is not in place'),
    'nrows before the row length': (dict(nrows=0, n=14), 'nrows < 1'),
}


@pytest.mark.parametrize('inverse', [0, 1])
@pytest.mark.parametrize('name', list(ROWDFT_REFUSED))
def test_the_row_transform_refuses_bad_arguments_before_any_device_call(name, inverse):
    import ctypes
    kw, msg = ROWDFT_REFUSED[name]
    a = dict(dict(out=8, inp=4096, nrows=3, n=12), **kw)
    ptr = lambda v: None if v is None else ctypes.c_void_p(v)
    L = _lib.load()
    assert L.xinv_rowdft_f64_dev(ptr(a['out']), ptr(a['inp']), a['nrows'], a['n'], inverse, None) == -1
    assert L.xinv_last_error().decode() == 'xinv_fourier: ' + msg


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
