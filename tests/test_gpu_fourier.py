"""The direct Fourier solve on the GPU (k_rowdft, k_fourier_tri, k_fourier_check): the row transform against
a long-double DFT under the error of numpy's own transform, the solve's backward error through the residual kernel against
the numpy restatement's (tests/fourier_model.py, computed here on the CPU), the undef refusal, the overflow word, the host
entry and the front end.

Measured on an MI355X (python -m pytest tests/test_gpu_fourier.py -s prints every figure; DESIGN.md 4.16 records them).
"""
import ctypes

import numpy as np
import pytest

import fourier_model as M
import resid_model as RM
import xinvert_amd as xa
from fourier_ld import dft_longdouble, err_ld
from xinvert_amd import _lib, fourier, synthetic

pytestmark = pytest.mark.gpu
U = -9.99e8


# ------------------------------------------------------------------ the row transform
def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def gpu_rfft(x):
    import torch
    return fourier.rfft_rows(torch.from_numpy(x).cuda()).cpu().numpy()


def gpu_roundtrip(x):
    import torch
    return fourier.irfft_rows(fourier.rfft_rows(torch.from_numpy(x).cuda()), x.shape[-1]).cpu().numpy()


def check_transform(n, rows):
    """The kernel's relative L2 error is at most 8x numpy's on the same rows, both against the long-double sum (both are
    O(eps log n); the butterfly order differs); the round trip under the same rule, numpy's round trip beside it."""
    x = np.random.default_rng(1000 * n + rows).standard_normal((rows, n))
    truth = dft_longdouble(x)
    e_np, e_k = err_ld(np.fft.rfft(x), truth), err_ld(gpu_rfft(x), truth)
    r_np, r_k = rel(np.fft.irfft(np.fft.rfft(x), n), x), rel(gpu_roundtrip(x), x)
    print('rowdft n %4d rows %3d: error kernel %.2e numpy %.2e (x%.2f); round trip kernel %.2e numpy %.2e (x%.2f)'
          % (n, rows, e_k, e_np, e_k / e_np, r_k, r_np, r_k / r_np if r_np else np.inf))
    assert e_k <= 8 * e_np, (n, rows, e_k, e_np)
    assert r_k <= 8 * r_np, (n, rows, r_k, r_np)


@pytest.mark.parametrize('n', [3, 4, 5, 12, 30, 45, 64, 360])
def test_rowdft_within_8x_of_numpys_error(n):
    for rows in (1, 2, 3, 130):                             # an odd count for the paired rows; more pairs than one round of workgroups
        check_transform(n, rows)


def test_rowdft_3600():
    check_transform(3600, 3)
    x = np.random.default_rng(3600003).standard_normal((3, 3600))
    print('rowdft n 3600: rel-L2(kernel, numpy.fft.rfft) %.2e' % rel(gpu_rfft(x), np.fft.rfft(x)))


def test_rowdft_refuses_other_lengths_and_ignores_the_dc_imaginary_part():
    import torch
    L = _lib.require_gpu()
    x = torch.zeros((2, 14), dtype=torch.float64, device='cuda')
    out = torch.zeros((2, 8), dtype=torch.complex128, device='cuda')
    rc = L.xinv_rowdft_f64_dev(_lib.dptr(out), _lib.dptr(x), 2, 14, 0, None)
    assert rc == -1 and b'row length 14 has the prime factor 7' in L.xinv_last_error()
    rc = L.xinv_rowdft_f64_dev(_lib.dptr(out), _lib.dptr(x), 2, 4500, 0, None)
    assert rc == -1 and b'4500' in L.xinv_last_error() and b'LDS budget' in L.xinv_last_error()
    with pytest.raises(_lib.XinvError, match='prime factor 7'):
        fourier.rfft_rows(x)
    X = np.fft.rfft(np.random.default_rng(3).standard_normal((3, 12)))
    X[:, 0] += 2j
    X[:, -1] -= 5j
    got = fourier.irfft_rows(torch.from_numpy(X).cuda(), 12).cpu().numpy()
    assert rel(got, np.fft.irfft(X, 12)) < 1e-15


# ------------------------------------------------------------------ the solve
def problem(yc, xc, nb, shared, seed, latlon=False):
    """-> dict(S0, F [nb, yc, xc], A, C [yc] or [nb, yc], delxSqr, ratioSqr, ...): random boundary rows and first guess."""
    rng = np.random.default_rng(seed)
    if latlon:
        p = synthetic.poisson_latlon(yc, xc, mask=False, seed=seed, members=nb)
        A, C = np.ascontiguousarray(np.asarray(p['coefs'][0])[:, 0]), np.ascontiguousarray(np.asarray(p['coefs'][2])[:, 0])
        F = np.ascontiguousarray(p['coefs'][3], dtype=np.float64).reshape(nb, yc, xc)
        sc = dict(delxSqr=p['delxSqr'], ratioSqr=p['ratioSqr'], ratioQtr=p['ratioQtr'], delx=p['delx'], dely=p['dely'])
    else:
        A, C = rng.uniform(0.5, 1.5, (nb, yc)), rng.uniform(0.5, 1.5, (nb, yc))
        if shared:
            A, C = A[0].copy(), C[0].copy()
        F = rng.standard_normal((nb, yc, xc))
        sc = dict(delxSqr=1.21, ratioSqr=(1.1 / 1.3) ** 2, ratioQtr=1.1 / 1.3 / 4, delx=1.1, dely=1.3)
    S0 = rng.standard_normal((nb, yc, xc)) * np.abs(F).max() * sc['delxSqr']
    return dict(sc, S0=S0, F=F, A=A, C=C, nb=nb, yc=yc, xc=xc)


def strides(p):
    n = p['yc'] * p['xc']
    return [n, p['yc'] if p['A'].ndim == 2 else 0, p['yc'] if p['C'].ndim == 2 else 0, n]


def run_dev(p, stream=None):
    """xinv_fourier_standard_2d_f64_dev on torch tensors -> (rc, S, flags, the tensors)."""
    import torch
    L = _lib.require_gpu()
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        t = {k: torch.from_numpy(np.ascontiguousarray(p[k])).cuda() for k in ('S0', 'A', 'C', 'F')}
    st.synchronize()
    fl = np.full((p['nb'], 3), -1.0)
    rc = L.xinv_fourier_standard_2d_f64_dev(_lib.dptr(t['S0']), _lib.dptr(t['A']), _lib.dptr(t['C']), _lib.dptr(t['F']), p['nb'],
                                            _lib.strides_arg(strides(p)), p['yc'], p['xc'], p['delxSqr'], p['ratioSqr'], U,
                                            _lib.hptr(fl), ctypes.c_void_p(st.cuda_stream))
    return rc, t['S0'].cpu().numpy(), fl, t


def full(p, name):
    """A or C as the residual takes it: [nb or 1][yc][xc]."""
    a = np.asarray(p[name]).reshape(-1, p['yc'])
    return np.ascontiguousarray(np.broadcast_to(a[:, :, None], a.shape + (p['xc'],)))


def gpu_backward_error(p, S):
    """[nb] max|R| / max|F| of S by xinv_residual_standard_2d_f64_dev (bitwise the numpy restatement)."""
    import torch
    L = _lib.require_gpu()
    n = p['yc'] * p['xc']
    Af, Cf = full(p, 'A'), full(p, 'C')
    tS, tA, tC, tF = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S, Af, Cf, p['F']))
    R = torch.empty_like(tS)
    norms = np.zeros((p['nb'], 4))
    st = [n, n, n if Af.shape[0] > 1 else 0, 0, n if Cf.shape[0] > 1 else 0, n]
    rc = L.xinv_residual_standard_2d_f64_dev(_lib.dptr(R), _lib.dptr(tS), _lib.dptr(tA), None, _lib.dptr(tC), _lib.dptr(tF),
                                             p['nb'], _lib.strides_arg(st), p['yc'], p['xc'], p['dely'], p['delx'], 0, 2,
                                             p['delxSqr'], p['ratioQtr'], p['ratioSqr'], 1.0, U, _lib.hptr(norms), None)
    _lib.check(rc)
    assert (norms[:, 0] == (p['yc'] - 2) * p['xc']).all()
    return norms[:, 2] / norms[:, 3]


def model_backward_error(p, S):
    Af, Cf = full(p, 'A'), full(p, 'C')
    out = []
    for m in range(p['nb']):
        R, live = RM.residual('std2d', S[m], [Af[m % Af.shape[0]], None, Cf[m % Cf.shape[0]], p['F'][m]], p, True, U)
        nrm = RM.norms(R, p['F'][m], live)
        out.append(nrm[2] / nrm[3])
    return np.array(out)


def check_solve(p, stream=None):
    Sm, flm = M.solve(p['S0'], p['A'], p['C'], p['F'], p['delxSqr'], p['ratioSqr'], U)
    rc, S, fl, _ = run_dev(p, stream)
    assert rc == 0, _lib.load().xinv_last_error()
    assert _lib.last_stats()['path'] == _lib.PATH_FOURIER2D
    assert np.array_equal(fl, flm) and not fl.any()
    assert np.array_equal(S[:, 0], p['S0'][:, 0]) and np.array_equal(S[:, -1], p['S0'][:, -1])      # rows 0 and yc-1: untouched
    be_k, be_m, fe = gpu_backward_error(p, S), model_backward_error(p, Sm), rel(S, Sm)
    print('fourier %3d x %3d x %d %s: max|R|/max|F| kernel %.2e model %.2e; rel-L2(kernel, model) %.1e'
          % (p['yc'], p['xc'], p['nb'], 'shared' if p['A'].ndim == 1 else 'per-member', be_k.max(), be_m.max(), fe))
    assert (be_k <= 4 * be_m).all(), (be_k, be_m)
    assert fe <= 1e-6
    return S


@pytest.mark.parametrize('yc', [3, 4, 37])
@pytest.mark.parametrize('xc', [12, 45, 64, 360])
def test_solve_shapes(yc, xc):
    check_solve(problem(yc, xc, 1, True, 100 * yc + xc))


def test_solve_latlon_181_by_360():
    check_solve(problem(181, 360, 1, True, 7, latlon=True))


@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-member'])
def test_solve_batches(shared):
    check_solve(problem(37, 45, 5, shared, 11))
    check_solve(problem(4, 64, 5, shared, 12))


def test_solve_on_a_second_stream_and_twice_the_same_bits():
    import torch
    p = problem(37, 64, 5, False, 13)
    S1 = check_solve(p)
    S2 = check_solve(p, torch.cuda.Stream())
    assert np.array_equal(S1, S2)


def test_undef_in_one_member_touches_no_members_field():
    p = problem(9, 30, 3, False, 14)
    p['F'][1, 4, 7] = U
    rc, S, fl, _ = run_dev(p)
    assert rc == -1
    msg = _lib.load().xinv_last_error().decode()
    assert 'member 1 holds undef at 1 of the points the solve reads' in msg, msg
    assert np.array_equal(S, p['S0'])
    for name, idx in (('S0', (2, 0, 3)), ('S0', (0, 8, 29)), ('A', (2, 8)), ('C', (0, 1))):
        q = problem(9, 30, 3, False, 14)
        q[name][idx] = U
        rc, S, fl, _ = run_dev(q)
        assert rc == -1 and ('member %d holds undef' % idx[0]).encode() in _lib.load().xinv_last_error(), (name, idx)
        assert np.array_equal(S, q['S0'])
    q = problem(9, 30, 3, False, 14)                       # points the solve does not read
    q['F'][1, 0, 3] = q['F'][1, 8, 3] = q['S0'][1, 4, 4] = q['A'][1, 0] = q['C'][1, 0] = q['C'][1, 8] = U
    rc, S, fl, _ = run_dev(q)
    assert rc == 0 and not fl.any()
    assert np.array_equal(S[:, 1:-1], run_dev(problem(9, 30, 3, False, 14))[1][:, 1:-1])


def test_nan_in_a_sets_the_members_overflow_word_alone():
    p = problem(9, 30, 3, False, 15)
    good = run_dev(p)[1]
    p['A'][1, 4] = np.nan
    rc, S, fl, _ = run_dev(p)
    assert rc == 0
    assert fl.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0]]
    assert np.array_equal(S[[0, 2]], good[[0, 2]]) and not np.isfinite(S[1, 1:-1]).all()


def test_host_entry_gives_the_device_entrys_bits():
    L = _lib.require_gpu()
    for shared in (True, False):
        p = problem(37, 45, 3, shared, 16)
        Sd = run_dev(p)[1]
        S = p['S0'].copy()
        fl = np.full((3, 3), -1.0)
        rc = L.xinv_fourier_standard_2d_f64_batched(_lib.hptr(S), _lib.hptr(p['A']), _lib.hptr(p['C']), _lib.hptr(p['F']), 3,
                                                    _lib.strides_arg(strides(p)), 37, 45, p['delxSqr'], p['ratioSqr'], U,
                                                    _lib.hptr(fl), _lib.options())
        _lib.check(rc)
        assert np.array_equal(S, Sd) and not fl.any()
        assert _lib.last_stats()['path'] == _lib.PATH_FOURIER2D
    p['F'][2, 5, 5] = U                                     # an error leaves the caller's S alone
    S = p['S0'].copy()
    rc = L.xinv_fourier_standard_2d_f64_batched(_lib.hptr(S), _lib.hptr(p['A']), _lib.hptr(p['C']), _lib.hptr(p['F']), 3,
                                                _lib.strides_arg(strides(p)), 37, 45, p['delxSqr'], p['ratioSqr'], U,
                                                _lib.hptr(fl), _lib.options())
    assert rc == -1 and np.array_equal(S, p['S0'])
    rc = L.xinv_fourier_standard_2d_f64_batched(_lib.hptr(S), _lib.hptr(p['A']), _lib.hptr(p['C']), _lib.hptr(p['F']), 3,
                                                _lib.strides_arg(strides(p)), 37, 14, p['delxSqr'], p['ratioSqr'], U,
                                                _lib.hptr(fl), _lib.options())
    assert rc == -1 and b'row length 14 has the prime factor 7' in L.xinv_last_error()


def test_front_end_quick_start_problem(capsys):
    """The README's quick start at 4 x 37 x 72: 'fourier' against 'sor' swept to 1e-13, and the residual of both."""
    lat, lon = np.linspace(-88.0, 88.0, 37), np.arange(72) * 5.0
    vor = xa.Field(1e-5 * np.random.default_rng(0).standard_normal((4, 37, 72)), ('time', 'lat', 'lon'), {'lat': lat, 'lon': lon})
    base = {'BCs': ['fixed', 'periodic']}
    run = lambda **kw: xa.invert_Poisson(vor, dims=['lat', 'lon'], coords='lat-lon', iParams=dict(base, **kw))
    sf = run(method='fourier', residual=True)
    assert 'fourier solve' in capsys.readouterr().out
    fl = sf.iParams['flags']
    assert fl.shape == (4, 3) and (fl[:, 2] == 0).all() and not fl.any()
    assert sf.iParams['stats']['path'] == _lib.PATH_FOURIER2D
    ref = run(method='sor', tolerance=1e-13, mxLoop=100000, printInfo=False)
    assert (ref.iParams['flags'][:, 2] < 100000).all()
    err = rel(sf.values, ref.values)
    sor = run(method='sor', residual=True, printInfo=False)
    ratio = lambda ip: (ip['resid'][:, 2] / ip['resid'][:, 3]).max()
    r_f, r_s = ratio(sf.iParams), ratio(sor.iParams)
    print('front end 4 x 37 x 72: rel-L2(fourier, sor at 1e-13) %.1e; max|R|/max|F| fourier %.1e, sor at the default tolerance %.1e'
          % (err, r_f, r_s))
    assert err <= 1e-6
    assert r_f * 100 <= r_s
    plain = run(method='fourier', printInfo=False)            # (without the residual: the same field)
    assert np.array_equal(plain.values, sf.values)
