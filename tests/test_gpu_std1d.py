"""The 1-D standard form on the GPU (k_std1d, xinvert_amd/csrc/xinv_std1d.h): bit for bit against the red-black model of
tests/std1d_model.py (S and all three flags), independent of batch, budget and stream, converged against the reference's
own lexicographic solutions (tests/golden/std1d_cases.npz), and the front end (apps.invert_GeoAdjustment /
invert_RefStateSWM, core.inv_standard1D)."""
import os

import numpy as np
import pytest

import std1d_model as M
from xinvert_amd import _lib
import xinvert_amd as xa
from xinvert_amd.field import Field

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNDEF = -9.99e8
BCS = ['fixed', 'extend', 'periodic']


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'std1d_cases.npz'))


def batched(S, A, B, F, BCx, delxSqr, optArg, mxLoop, tol, strides=None, **opt):
    """xinv_standard_1d_f64_batched on host arrays; S [nbatch, xc] is solved in place -> (rc, flags [nbatch, 3])."""
    L = _lib.require_gpu()
    S = np.ascontiguousarray(S, dtype=np.float64)
    nb, xc = S.shape if S.ndim == 2 else (1, S.shape[0])
    arrs = [S] + [np.ascontiguousarray(a, dtype=np.float64) for a in (A, B, F)]
    if strides is None:
        strides = [xc if a.ndim == 2 else 0 for a in arrs]
    fl = np.tile([0.0, 1.0, 0.0], (nb, 1))
    rc = L.xinv_standard_1d_f64_batched(*[_lib.hptr(a) for a in arrs], nb, _lib.strides_arg(strides), xc, 1.0,
                                        _lib.bc(BCx), delxSqr, optArg, UNDEF, _lib.hptr(fl), int(mxLoop), float(tol),
                                        _lib.options(**opt))
    return rc, fl, arrs[0]


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb_ = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb_) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb_])


def golden_cases(g):
    for k, name in enumerate(g['names']):
        p = 'c%d_' % k
        par = g[p + 'par']
        yield str(name), dict(S0=g[p + 'S0'], A=g[p + 'A'], B=g[p + 'B'], F=g[p + 'F'], BCx=BCS[int(par[0])],
                              delxSqr=par[1], optArg=par[2], mxLoop=int(par[3]), tol=par[4])


def check_vs_model(c, **opt):
    rc, fl, S = batched(c['S0'][None, :].copy(), c['A'], c['B'], c['F'], c['BCx'], c['delxSqr'], c['optArg'],
                        c['mxLoop'], c['tol'], **opt)
    assert rc == 0, _lib.load().xinv_last_error()
    Sm, flm = M.rb_solve(c['S0'], c['A'], c['B'], c['F'], c['BCx'], c['delxSqr'], c['optArg'], UNDEF, c['mxLoop'],
                         c['tol'])
    return bits_equal(S[0], Sm) and bits_equal(fl[0], flm), (fl[0], flm)


def test_golden_matrix_bitwise_vs_red_black_model(gold):
    bad = []
    for name, c in golden_cases(gold):
        ok, info = check_vs_model(c)
        if not ok:
            bad.append((name, info))
    assert not bad, bad[:5]


@pytest.mark.parametrize('xc', [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049,
                                M.MAX_XC])
@pytest.mark.parametrize('BCx', ['fixed', 'extend', 'periodic'])
def test_edges_of_lanes_and_waves_bitwise(xc, BCx):
    rng = np.random.default_rng(xc * 7 + len(BCx))
    c = dict(S0=rng.standard_normal(xc) * 0.1, A=rng.uniform(0.5, 1.5, xc), B=rng.uniform(-0.5, 0, xc),
             F=rng.standard_normal(xc), BCx=BCx, delxSqr=0.49, optArg=1.5, mxLoop=12, tol=-1.0)
    c['F'][xc // 3] = UNDEF
    ok, info = check_vs_model(c, sweeps_per_launch=5)
    assert ok, info


def test_above_the_maximum_is_an_argument_error():
    xc = M.MAX_XC + 1
    rc, fl, S = batched(np.zeros((1, xc)), np.ones(xc), -np.ones(xc), np.ones(xc), 'fixed', 1.0, 1.5, 3, -1.0)
    assert rc == -1
    assert str(M.MAX_XC) in _lib.load().xinv_last_error().decode()


@pytest.mark.parametrize('opt', [dict(ndev=2), dict(f32_mask=1), dict(fma=1)])
def test_unsupported_options_are_argument_errors(opt):
    xc = 33
    o = dict(opt)
    ndev = o.pop('ndev', None)
    kw = dict(devices=[0, 0]) if ndev else o
    rc, fl, S = batched(np.zeros((1, xc)), np.ones(xc), -np.ones(xc), np.ones(xc), 'fixed', 1.0, 1.5, 3, -1.0, **kw)
    assert rc == -1
    rc, _, _ = batched(np.zeros((1, 2)), np.ones(2), -np.ones(2), np.ones(2), 'fixed', 1.0, 1.5, 3, -1.0)
    assert rc == -1                                         # xc < 3


@pytest.mark.parametrize('nb', [1, 3, 1000])
def test_batch_members_equal_their_solves_alone(nb):
    xc = 73
    rng = np.random.default_rng(nb)
    A = rng.uniform(0.5, 1.5, xc)
    B = rng.uniform(-0.5, 0.0, (nb, xc))
    F = rng.standard_normal((nb, xc))
    if nb > 1:
        B[1, 7] = np.nan                                    # member 1 overflows, the others do not
    S0 = np.zeros((nb, xc))
    rc, fl, S = batched(S0.copy(), A, B, F, 'periodic', 1.0, 1.6, 300, 1e-7)
    assert rc == 0
    for m in range(nb):
        rc1, fl1, S1 = batched(S0[m:m + 1].copy(), A, B[m], F[m], 'periodic', 1.0, 1.6, 300, 1e-7)
        assert rc1 == 0
        assert bits_equal(S[m], S1[0]) and bits_equal(fl[m], fl1[0]), m
    if nb > 1:
        assert fl[1, 0] == 1.0 and fl[0, 0] == 0.0
        assert len(set(fl[:, 2])) > 1                       # the stop sweep is per member


def test_budget_independence_including_a_tolerance_stop():
    xc = 181
    rng = np.random.default_rng(5)
    A, B, F = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, -0.1, (4, xc)), rng.standard_normal((4, xc))
    res = []
    for spl in (1, 7, 0):
        rc, fl, S = batched(np.zeros((4, xc)), A, B, F, 'extend', 1.0, 1.7, 5000, 1e-6, sweeps_per_launch=spl)
        assert rc == 0
        res.append((S, fl))
    assert 0 < res[0][1][0, 2] < 5000 and res[0][1][0, 2] % 7 != 6        # stopped inside a launch of 7
    for S, fl in res[1:]:
        assert bits_equal(S, res[0][0]) and bits_equal(fl, res[0][1])


def test_launches_and_stats():
    xc = 65
    rng = np.random.default_rng(9)
    A, B, F = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, 0, xc), rng.standard_normal(xc)
    rc, fl, S = batched(np.zeros((1, xc)), A, B, F, 'fixed', 1.0, 1.5, 99, -1.0, sweeps_per_launch=10, check_every=3,
                        timing=1)
    st = _lib.last_stats()
    assert rc == 0 and fl[0, 2] == 99
    assert st['path'] == _lib.PATH_WAVE1D and st['sweeps_max'] == 100 and st['sweep_launches'] == 10
    assert st['sweep_ms'] > 0


def test_dev_on_a_side_stream_and_positional_twin_equal_batched():
    import torch
    L = _lib.require_gpu()
    xc, nb = 101, 5
    rng = np.random.default_rng(3)
    A, B, F = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, 0, (nb, xc)), rng.standard_normal((nb, xc))
    S0 = rng.standard_normal((nb, xc)) * 0.1
    rc, fl, S = batched(S0.copy(), A, B, F, 'periodic', 1.0, 1.5, 400, 1e-9)
    assert rc == 0
    dev = torch.device('cuda')
    t = [torch.tensor(a, dtype=torch.float64, device=dev) for a in (S0, A, B, F)]
    torch.cuda.synchronize()                                  # (the uploads ran on the default stream)
    st = torch.cuda.Stream()
    fld = np.tile([0.0, 1.0, 0.0], (nb, 1))
    with torch.cuda.stream(st):
        rc = L.xinv_standard_1d_f64_dev(*[x.data_ptr() for x in t], nb, _lib.strides_arg([xc, 0, xc, xc]), xc, 1.0, 2,
                                        1.0, 1.5, UNDEF, _lib.hptr(fld), 400, 1e-9, _lib.options(), st.cuda_stream)
    st.synchronize()
    assert rc == 0
    assert bits_equal(t[0].cpu().numpy(), S) and bits_equal(fld, fl)
    S1 = S0[2].copy()
    fl1 = np.array([0.0, 1.0, 0.0])
    rc = L.xinv_standard_1d_f64(_lib.hptr(S1), _lib.hptr(A), _lib.hptr(np.ascontiguousarray(B[2])),
                                _lib.hptr(np.ascontiguousarray(F[2])), xc, 1.0, 2, 1.0, 1.5, UNDEF, _lib.hptr(fl1), 400,
                                1e-9, None)
    assert rc == 0 and bits_equal(S1, S[2]) and bits_equal(fl1, fl[2])


def rel_l2(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize('tag', ['geo', 'swm'])
def test_converged_kernel_vs_reference_lexicographic(gold, tag):
    g = lambda k: gold['%s_%s' % (tag, k)]
    BCx = str(g('BCx'))
    xc = len(g('lat'))
    rc, fl, S = batched(np.zeros((1, xc)), g('A'), g('B'), g('F'), BCx, float(g('delxSqr')), float(g('optArg')),
                        int(g('mxLoop')), float(g('tol')))
    assert rc == 0 and fl[0, 0] == 0
    assert rel_l2(S[0], g('S')) < 1e-6
    if tag == 'geo':                                          # the discrete residual, independent of any solver
        A, B, F, d = g('A'), g('B'), g('F'), float(g('delxSqr'))
        s = S[0]
        r = (A[2:] * (s[2:] - s[1:-1]) - A[1:-1] * (s[1:-1] - s[:-2])) / d + (B[1:-1] * s[1:-1] - F[1:-1])
        assert np.linalg.norm(r) / np.linalg.norm(F[1:-1]) <= 1e-9


def test_apps_on_the_golden_inputs(gold):
    lat = gold['geo_lat']
    h0 = Field(gold['geo_h0'], ('lat',), {'lat': lat})
    h = xa.invert_GeoAdjustment(h0, dims=['lat'], coords='lat',
                                iParams={'BCs': ['extend'], 'mxLoop': 100000, 'tolerance': -1e-11, 'optArg': 1.8,
                                         'undef': -9999, 'printInfo': False})
    assert rel_l2(np.asarray(h.values), gold['geo_S']) < 1e-6
    lat = gold['swm_lat']
    Q = Field(gold['swm_Q'], ('lat',), {'lat': lat})
    mp = {'M0': Field(gold['swm_M0'], ('lat',), {'lat': lat}), 'C0': Field(gold['swm_C0'], ('lat',), {'lat': lat})}
    S = xa.invert_RefStateSWM(Q, dims=['lat'], coords='lat', mParams=mp,
                              iParams={'mxLoop': 20000, 'tolerance': -1.0, 'printInfo': False})
    assert rel_l2(np.asarray(S.values), gold['swm_S']) < 1e-6


def test_front_end_batched_slices(capsys):
    nt, yc, nx = 2, 91, 3
    lat = np.linspace(-60, -15, yc)
    rng = np.random.default_rng(1)
    h0v = 1500 + 20 * rng.random((nt, yc, nx))
    h0v[1, 40, 2] = np.nan                                     # masked: de-masked to undef as the reference does
    h0 = Field(h0v, ('time', 'lat', 'lon'), {'time': np.arange(nt), 'lat': lat, 'lon': np.arange(nx) * 1.0})
    ip = {'BCs': ['extend'], 'mxLoop': 3000, 'tolerance': 1e-9}
    h = xa.invert_GeoAdjustment(h0, dims=['lat'], coords='lat', iParams=ip)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == nt * nx and 'loops' in out[0]
    assert h.dims == ('time', 'lat', 'lon') and h.shape == h0v.shape
    fl = h.iParams['flags']
    assert fl.shape == (nt * nx, 3)
    assert np.isnan(h.values[1, 40, 2])
    # every slice is its own 1-D solve: slice (0, :, 1) alone gives the same bits
    h1 = xa.invert_GeoAdjustment(Field(h0v[0, :, 1], ('lat',), {'lat': lat}), dims=['lat'], coords='lat',
                                 iParams=dict(ip, printInfo=False))
    assert bits_equal(np.asarray(h1.values), h.values[0, :, 1])
