"""The tridiagonal direct solver on the GPU (k_tridiag, xinvert_amd/csrc/xinv_tridiag.h): trace / traceCyclic and the
direct path of the 1-D standard form (XINV_PATH_DIRECT1D) bit for bit against the numpy restatement of
tests/tridiag_model.py, which tests/test_tridiag_host.py holds to the reference's own outputs."""
import os

import numpy as np
import pytest

import std1d_model as M1
import tridiag_model as M
import xinvert_amd as xa
from xinvert_amd import _lib
from xinvert_amd.field import Field

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNDEF = -9.99e8
BCS = M.BCS


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


def on_device(*arrs):
    import torch
    return [torch.tensor(np.asarray(v), dtype=torch.float64, device='cuda') for v in arrs]


def both_front_ends(a, b, c, d, a0=None, cn=None):
    """-> [x from numpy arrays (host entry), x from CUDA tensors (device entry)]"""
    if a0 is None:
        return [xa.trace(a, b, c, d), xa.trace(*on_device(a, b, c, d)).cpu().numpy()]
    return [xa.traceCyclic(a, b, c, d, a0, cn), xa.traceCyclic(*on_device(a, b, c, d, a0, cn)).cpu().numpy()]


def test_golden_systems_bitwise_both_entries_both_front_ends(gold):
    for p in ['pin_'] + ['t%d_' % k for k in range(len(gold['tn']))]:
        g = lambda k: gold[p + k]
        for x in both_front_ends(g('a'), g('b'), g('c'), g('d')):
            assert bits_equal(x, g('x')), p
        for x in both_front_ends(g('a'), g('b'), g('c'), g('d'), float(g('a0')), float(g('cn'))):
            assert bits_equal(x, g('xc')), p


@pytest.mark.parametrize('nb', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('n', [2, 37, 64])                 # (the chunk is 16 points)
def test_batches_shared_and_per_member_coefficients(nb, n):
    rng = np.random.default_rng(nb * 100 + n)
    a, c = rng.uniform(-1, 1, n - 1), rng.uniform(-1, 1, (nb, n - 1))
    b = rng.uniform(2.5, 4.0, (nb, n)) * rng.choice([-1.0, 1.0], (nb, n))
    d = rng.standard_normal((nb, n))
    a0, cn = rng.uniform(-1, 1, nb), 0.375
    for x in both_front_ends(a, b, c, d):
        assert bits_equal(x, M.trace(a, b, c, d))
    for x in both_front_ends(a, b, c, d, a0, cn):
        assert bits_equal(x, M.traceCyclic(a, b, c, d, a0, cn))
    # every array per member; every coefficient array shared (only d per member)
    am = rng.uniform(-1, 1, (nb, n - 1))
    assert bits_equal(xa.trace(am, b, c, d), M.trace(am, b, c, d))
    assert bits_equal(xa.traceCyclic(a, b[0], c[0], d, 0.5, cn), M.traceCyclic(a, b[0], c[0], d, 0.5, cn))


def test_non_finite_systems_keep_their_nans_in_place():
    n = 40
    rng = np.random.default_rng(1)
    a, c, d = rng.uniform(-1, 1, n - 1), rng.uniform(-1, 1, n - 1), rng.standard_normal((3, n))
    b = rng.uniform(2.5, 4.0, (3, n))
    b[1, 17] = np.nan
    b[2, 0] = 0.0                                            # a zero pivot
    assert bits_equal(xa.trace(a, b, c, d), M.trace(a, b, c, d))
    assert bits_equal(xa.traceCyclic(a, b, c, d, 0.3, 0.2), M.traceCyclic(a, b, c, d, 0.3, 0.2))


def test_c_abi_argument_errors():
    L = _lib.require_gpu()
    one = np.ones(4)
    st7 = _lib.strides_arg([4, 0, 0, 0, 0, 0, 0])
    h = _lib.hptr
    assert L.xinv_tridiag_f64(h(one.copy()), h(one), h(one), h(one), h(one), None, None, 1, st7, 1) == -1      # n < 2
    assert L.xinv_tridiag_f64(h(one.copy()), h(one), h(one), h(one), h(one), h(one), None, 1, st7, 4) == -1   # one corner
    assert L.xinv_tridiag_f64(h(one.copy()), h(one), h(one), h(one), h(one), None, h(one), 1, st7, 4) == -1
    assert b'a0 and cn' in L.xinv_last_error()
    assert L.xinv_tridiag_f64(h(one.copy()), h(one), h(one), h(one), h(one), None, None, 0, st7, 4) == -1      # nbatch
    assert L.xinv_tridiag_f64(h(one.copy()), h(one), h(one), h(one), h(one), None, None, 1, None, 4) == -1     # strides
    assert L.xinv_tridiag_f64(h(one.copy()), None, h(one), h(one), h(one), None, None, 1, st7, 4) == -1


# ------------------------------------------------------------------ the direct path of the 1-D standard form
def entries(S0, A, B, F, BCx, delxSqr, which, optArg=1.5, mxLoop=7, tol=1e-3, path=_lib.PATH_DIRECT1D):
    """One of the three xinv_standard_1d_f64* entries on [nbatch, xc] arrays (A, B, F: [xc] = shared) -> (rc, S, flags)."""
    L = _lib.require_gpu()
    S = np.array(np.atleast_2d(S0), dtype=np.float64)
    nb, xc = S.shape
    arrs = [S] + [np.ascontiguousarray(v, dtype=np.float64) for v in (A, B, F)]
    strides = _lib.strides_arg([xc if v.ndim == 2 else 0 for v in arrs])
    fl = np.tile([0.0, 1.0, 0.0], (nb, 1))
    opt = _lib.options(path=path)
    tail = (1.0, _lib.bc(BCx), delxSqr, optArg, UNDEF, _lib.hptr(fl), mxLoop, tol, opt)
    if which == 'single':
        assert nb == 1
        rc = L.xinv_standard_1d_f64(*[_lib.hptr(v.reshape(-1)[:xc] if v.ndim == 2 else v) for v in arrs], xc, *tail)
    elif which == 'batched':
        rc = L.xinv_standard_1d_f64_batched(*[_lib.hptr(v) for v in arrs], nb, strides, xc, *tail)
    else:
        import torch
        t = on_device(*arrs)
        rc = L.xinv_standard_1d_f64_dev(*[v.data_ptr() for v in t], nb, strides, xc, *tail,
                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        S = t[0].cpu().numpy()
    return rc, S, fl


def test_three_entries_bitwise_on_the_std1d_matrix_and_the_converged_cases(gold, gold1d):
    bad, nan_flags = [], {}
    for g in (gold1d, gold):
        for k, name in enumerate(g['names']):
            p = 'c%d_' % k
            par = g[p + 'par']
            BCx, dsq = BCS[int(par[0])], float(par[1])
            Sm, flm = M.direct_solve(g[p + 'S0'], g[p + 'A'], g[p + 'B'], g[p + 'F'], BCx, dsq, UNDEF)
            for which in ('single', 'batched', 'dev'):
                rc, S, fl = entries(g[p + 'S0'], g[p + 'A'], g[p + 'B'], g[p + 'F'], BCx, dsq, which)
                if rc != 0 or not bits_equal(S[0], Sm) or not bits_equal(fl[0], flm):
                    bad.append((str(name), which, rc, fl[0], flm))
                if str(name).endswith('_nan'):
                    nan_flags[(str(name), which)] = list(fl[0])
    assert not bad, bad[:5]
    assert len(nan_flags) == 9 and all(v == [1.0, 0.0, 0.0] for v in nan_flags.values()), nan_flags
    assert _lib.last_stats()['path'] == _lib.PATH_DIRECT1D == 5


@pytest.mark.parametrize('nb', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('BCx', BCS)
def test_direct_path_batches_with_per_member_masks(nb, BCx):
    xc = 37                                                   # (two chunks and five points)
    rng = np.random.default_rng(nb + len(BCx))
    A, B = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, -0.1, (nb, xc))
    F, S0 = rng.standard_normal((nb, xc)), rng.standard_normal((nb, xc)) * 0.1
    # the end rows differ from member to member: live, masked at 0, at xc-1, at both; an undef first guess beside an end
    F[1::4, 0] = UNDEF
    F[2::4, xc - 1] = UNDEF
    F[3::8, [0, xc - 1]] = UNDEF
    F[5::7, 11] = UNDEF
    S0[4::9, 1] = UNDEF
    S0[6::9, xc - 2] = UNDEF
    Sm, flm = M.direct_solve(S0, A, B, F, BCx, 0.49, UNDEF)
    for which in ('batched', 'dev'):
        rc, S, fl = entries(S0, A, B, F, BCx, 0.49, which)
        assert rc == 0 and bits_equal(S, Sm) and bits_equal(fl, flm), which
    Am = rng.uniform(0.5, 1.5, (nb, xc))                      # every array per member
    Am[::5, 0] = UNDEF
    Sm, flm = M.direct_solve(S0, Am, B, F, BCx, 0.49, UNDEF)
    rc, S, fl = entries(S0, Am, B, F, BCx, 0.49, 'batched')
    assert rc == 0 and bits_equal(S, Sm) and bits_equal(fl, flm)


@pytest.mark.parametrize('BCx', BCS)
def test_a_member_longer_than_the_sweeps_take(BCx):
    xc = 20001
    rng = np.random.default_rng(xc)
    A, B, F = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, -0.1, xc), rng.standard_normal(xc)
    F[xc // 2] = UNDEF
    S0 = np.zeros(xc)
    rc, S, fl = entries(S0, A, B, F, BCx, 0.49, 'batched')
    Sm, flm = M.direct_solve(S0, A, B, F, BCx, 0.49, UNDEF)
    assert rc == 0 and bits_equal(S[0], Sm) and bits_equal(fl[0], flm) and fl[0, 0] == 0
    rc, _, _ = entries(S0, A, B, F, BCx, 0.49, 'batched', path=_lib.PATH_AUTO)
    assert rc == -1 and str(M1.MAX_XC) in _lib.load().xinv_last_error().decode()


@pytest.mark.parametrize('BCx', ['extend', 'periodic'])
def test_the_headline_batch_23040_members_of_181_points(BCx):
    nb, xc = 23040, 181
    rng = np.random.default_rng(181)
    A, B = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, -0.1, (nb, xc))
    F, S0 = rng.standard_normal((nb, xc)), np.zeros((nb, xc))
    F[::97, 0] = UNDEF
    rc, S, fl = entries(S0, A, B, F, BCx, 0.49, 'dev')
    Sm, flm = M.direct_solve(S0, A, B, F, BCx, 0.49, UNDEF)
    assert rc == 0 and bits_equal(S, Sm) and bits_equal(fl, flm) and not fl[:, 0].any()


def test_other_forms_refuse_the_direct_path():
    L = _lib.require_gpu()
    yc = xc = 8
    S, A, F = np.zeros((yc, xc)), np.ones((yc, xc)), np.ones((yc, xc))
    fl = np.array([0.0, 1.0, 0.0])
    h = _lib.hptr
    rc = L.xinv_standard_2d_f64_batched(h(S), h(A), None, h(A), h(F), 1, _lib.strides_arg([64, 64, 0, 64, 64]), yc, xc,
                                        1.0, 1.0, 0, 0, 1.0, 0.25, 1.0, 1.5, UNDEF, h(fl), 5, 1e-8,
                                        _lib.options(path=_lib.PATH_DIRECT1D))
    assert rc == -1 and b'DIRECT1D' in L.xinv_last_error()


def test_default_path_is_still_the_sweeps(gold1d):
    names = [str(n) for n in gold1d['names']]
    p = 'c%d_' % names.index('periodic_65_F')
    g = lambda k: gold1d[p + k]
    par = g('par')
    rc, S, fl = entries(g('S0'), g('A'), g('B'), g('F'), 'periodic', par[1], 'batched', optArg=par[2], mxLoop=int(par[3]),
                        tol=par[4], path=_lib.PATH_AUTO)
    assert rc == 0 and _lib.last_stats()['path'] == _lib.PATH_WAVE1D
    Sm, flm = M1.rb_solve(g('S0'), g('A'), g('B'), g('F'), 'periodic', par[1], par[2], UNDEF, int(par[3]), par[4])
    assert bits_equal(S[0], Sm) and bits_equal(fl[0], flm)


def test_front_end_method_direct(gold1d):
    lat = gold1d['geo_lat']
    h0 = Field(gold1d['geo_h0'], ('lat',), {'lat': lat})
    ip = {'BCs': ['extend'], 'undef': -9999, 'printInfo': False, 'method': 'direct'}
    h = xa.invert_GeoAdjustment(h0, dims=['lat'], coords='lat', iParams=ip)
    ref = gold1d['geo_S']
    assert np.linalg.norm(np.asarray(h.values) - ref) / np.linalg.norm(ref) < 1e-6
    assert list(h.iParams['flags']) == [0.0, 0.0, 0.0]
    assert h.iParams['stats']['path'] == _lib.PATH_DIRECT1D
    # slices of a larger array are members of one batched call: each equals its solve alone
    nt, nx = 2, 3
    h0v = 1500 + 20 * np.random.default_rng(2).random((nt, len(lat), nx))
    hb = xa.invert_GeoAdjustment(Field(h0v, ('time', 'lat', 'lon'), {'time': np.arange(nt), 'lat': lat,
                                                                      'lon': np.arange(nx) * 1.0}),
                                 dims=['lat'], coords='lat', iParams=dict(ip))
    h1 = xa.invert_GeoAdjustment(Field(h0v[1, :, 2], ('lat',), {'lat': lat}), dims=['lat'], coords='lat', iParams=dict(ip))
    assert hb.iParams['flags'].shape == (nt * nx, 3) and bits_equal(np.asarray(h1.values), hb.values[1, :, 2])
