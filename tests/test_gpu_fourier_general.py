"""The direct Fourier solve of the 2-D general form on the GPU (k_fourier_gcheck, k_fourier_cfactor, k_fourier_csubst around
k_rowdft; DESIGN.md 4.16, "General form"): the solve against a long-double truth (tests/fourier_general_ld.py) under the
error of the numpy restatement (tests/fourier_general_model.py), on both sides of the 64 lanes and of the rows-ahead batch;
the entries, the members, `undef` and NaN; repeats and workspace growth; the front end on Gill-Matsuno.

The bars are the multiples of tests/test_gpu_fourier_edges.py: forward distance (relative L2 to the truth) within 8x the
model's, long-double backward error within 4x the model's, one rounding of the truth (2^-53) as the floor of both; the
residual kernel's max|R| / max|G| of the kernel's field within 4x that of the model's field by the same stencil in numpy
(tests/resid_model.py) with the same floor.

Measured on an MI355X (python -m pytest tests/test_gpu_fourier_general.py -s prints every figure; DESIGN.md 4.16 records them).
"""
import ctypes

import numpy as np
import pytest

import fourier_general_ld as T
import fourier_general_model as GM
import fourier_ld
import resid_model as RM
import xinvert_amd as xa
from xinvert_amd import _lib, core, synthetic
from xinvert_amd.field import Field

pytestmark = pytest.mark.gpu
U = -9.99e8
HALF_ULP = 2.0 ** -53
AHEAD = 8                             # XINV_CSUB_AHEAD of xinvert_amd/csrc/xinv_cfourier.h
NAMES = ('S0', 'A', 'C', 'D', 'E', 'Fc', 'G')


def arrays(p):
    return [p['S0']] + list(p['c']) + [p['G']]


def strides(p):
    n = p['yc'] * p['xc']
    return [n] + [p['yc'] if np.ndim(x) == 2 else 0 for x in p['c']] + [n]


def dev_call(arrs, st, p, stream=None):
    """xinv_fourier_general_2d_f64_dev on flat host buffers (S, A, C, D, E, Fc, G) with the strides `st` -> (rc, S buffer, flags)."""
    import torch
    L = _lib.require_gpu()
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        t = [torch.from_numpy(np.array(a, dtype=np.float64, order='C')).cuda() for a in arrs]
    s.synchronize()
    fl = np.full((p['nb'], 3), -1.0)
    rc = L.xinv_fourier_general_2d_f64_dev(*[_lib.dptr(a) for a in t], p['nb'], _lib.strides_arg(st), p['yc'], p['xc'], *p['sc'],
                                           U, _lib.hptr(fl), ctypes.c_void_p(s.cuda_stream))
    return rc, t[0].cpu().numpy(), fl


def host_call(arrs, st, p):
    L = _lib.require_gpu()
    S = np.array(arrs[0], copy=True)
    fl = np.full((p['nb'], 3), -1.0)
    rc = L.xinv_fourier_general_2d_f64_batched(_lib.hptr(S), *[_lib.hptr(np.ascontiguousarray(a)) for a in arrs[1:]], p['nb'],
                                               _lib.strides_arg(st), p['yc'], p['xc'], *p['sc'], U, _lib.hptr(fl), _lib.options())
    return rc, S, fl


def run_dev(p, stream=None):
    rc, S, fl = dev_call(arrays(p), strides(p), p, stream)
    return rc, S.reshape(p['S0'].shape), fl


def last_error():
    return _lib.load().xinv_last_error().decode()


def full(p, q):
    """Coefficient q as the residual takes it: [nb or 1][yc][xc]."""
    a = np.asarray(p['c'][q]).reshape(-1, p['yc'])
    return np.ascontiguousarray(np.broadcast_to(a[:, :, None], a.shape + (p['xc'],)))


def resid_scalars(p):
    delx, dx2, ratio, rs = p['sc']
    return dict(dely=delx / ratio, delx=delx, delxSqr=dx2, ratio=ratio, ratioQtr=ratio / 4, ratioSqr=rs)


def gpu_backward_error(p, S):
    """[nb] max|R| / max|G| of S by xinv_residual_general_2d_f64_dev."""
    import torch
    L = _lib.require_gpu()
    n = p['yc'] * p['xc']
    cf = [full(p, q) for q in range(5)]
    sc = resid_scalars(p)
    tS, tG = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S, p['G']))
    tc = [torch.from_numpy(a).cuda() for a in cf]
    R = torch.empty_like(tS)
    norms = np.zeros((p['nb'], 4))
    cs = [n if a.shape[0] > 1 else 0 for a in cf]
    st = [n, n, cs[0], 0, cs[1], cs[2], cs[3], cs[4], n]
    rc = L.xinv_residual_general_2d_f64_dev(_lib.dptr(R), _lib.dptr(tS), _lib.dptr(tc[0]), None, *[_lib.dptr(a) for a in tc[1:]],
                                            _lib.dptr(tG), p['nb'], _lib.strides_arg(st), p['yc'], p['xc'], sc['dely'], sc['delx'],
                                            0, 2, sc['delxSqr'], sc['ratio'], sc['ratioQtr'], sc['ratioSqr'], 1.0, U,
                                            _lib.hptr(norms), None)
    _lib.check(rc)
    assert (norms[:, 0] == (p['yc'] - 2) * p['xc']).all()
    return norms[:, 2] / norms[:, 3]


def model_backward_error(p, S):
    cf = [full(p, q) for q in range(5)]
    out = []
    for m in range(p['nb']):
        A, C, D, E, Fc = (a[m % a.shape[0]] for a in cf)
        R, live = RM.residual('gen2d', S[m], [A, None, C, D, E, Fc, p['G'][m]], resid_scalars(p), True, U)
        nrm = RM.norms(R, p['G'][m], live)
        out.append(nrm[2] / nrm[3])
    return np.array(out)


def rel_ld(S, truth):
    d = np.asarray(S).astype(T.LD) - truth
    return float(np.sqrt((d * d).sum() / (truth * truth).sum()))


def check_solve_ld(p, stream=None, what='general'):
    St = T.ld_solve(p['S0'], p['c'], p['G'], p['sc'])
    Sm, flm = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    rc, S, fl = run_dev(p, stream)
    assert rc == 0, last_error()
    assert _lib.last_stats()['path'] == _lib.PATH_FOURIER2D
    assert not fl.any() and not flm.any()
    assert np.array_equal(S[:, 0], p['S0'][:, 0]) and np.array_equal(S[:, -1], p['S0'][:, -1])
    fe_k, fe_m = rel_ld(S, St), rel_ld(Sm, St)
    be_k, be_m = (T.ld_backward(X, p['c'], p['G'], p['sc']).astype(np.float64) for X in (S, Sm))
    rk, rm = gpu_backward_error(p, S), model_backward_error(p, Sm)
    print('%s %3d x %4d x %d %-10s: rel-L2 to the truth kernel %.2e model %.2e; backward error in long double kernel %.2e model '
          '%.2e; residual kernel %.2e model %.2e; bits %s'
          % (what, p['yc'], p['xc'], p['nb'], 'shared' if np.ndim(p['c'][0]) == 1 else 'per-member', fe_k, fe_m, be_k.max(),
             be_m.max(), rk.max(), rm.max(), 'equal' if np.array_equal(S, Sm) else 'differ'))
    assert fe_k <= 8 * max(fe_m, HALF_ULP), (fe_k, fe_m)
    assert (be_k <= 4 * np.maximum(be_m, HALF_ULP)).all(), (be_k, be_m)
    assert (rk <= 4 * np.maximum(rm, HALF_ULP)).all(), (rk, rm)
    return S


# ------------------------------------------------------------------ the solve against the long-double truth
@pytest.mark.parametrize('yc', [3, 4, 5, 6])
def test_solve_against_the_long_double_truth(yc):
    """1 .. 4 interior rows; K = 2 .. 5, 61, 63, 65 and 129 wavenumbers (the last lane of a workgroup, one lane into the
    second, a third workgroup); one, two and three members with shared and with their own coefficients.  (The row lengths
    are looped here, not parametrised: 48 small solves, well under a second.)"""
    for xc in (3, 4, 6, 8, 120, 125, 128, 256):
        for nb in (1, 2, 3):
            for shared in (True, False):
                check_solve_ld(GM.problem(yc, xc, nb, shared, 7000 + 10 * xc + yc + 100000 * nb))


def test_rows_at_and_one_above_each_multiple_of_the_batch():
    for rows in (AHEAD, AHEAD + 1, 2 * AHEAD, 2 * AHEAD + 1, 3 * AHEAD, 3 * AHEAD + 1):
        check_solve_ld(GM.problem(rows + 2, 12, 2, False, 8000 + rows))
        check_solve_ld(GM.problem(rows + 2, 12, 2, True, 8100 + rows))


@pytest.mark.parametrize('yc,xc', [(300, 12), (130, 45)])
def test_tall_solve_against_the_long_double_truth(yc, xc):
    check_solve_ld(GM.problem(yc, xc, 1, False, 7000 + 10 * xc + yc))


@pytest.mark.parametrize('yc,xc', [(5, 4096), (4, 2160)])
def test_solve_at_the_lds_edges(yc, xc):
    try:
        check_solve_ld(GM.problem(yc, xc, 1, True, 100 * yc + xc))
    finally:
        fourier_ld._MAT.pop(xc, None)                        # (the truth's xc x xc matrix: not kept for the rest of the run)


# ------------------------------------------------------------------ entries, members and undef
def one_member(p, m):
    c = [x[m:m + 1] if np.ndim(x) == 2 else x for x in p['c']]
    return dict(p, S0=p['S0'][m:m + 1], G=p['G'][m:m + 1], c=c, nb=1)


def test_host_entry_gives_the_device_entrys_bits():
    for shared in (True, False):
        p = GM.problem(37, 45, 3, shared, 16)
        rc, Sd, fld = run_dev(p)
        assert rc == 0 and not fld.any()
        rc, S, fl = host_call(arrays(p), strides(p), p)
        assert rc == 0, last_error()
        assert np.array_equal(S, Sd) and not fl.any()
        assert _lib.last_stats()['path'] == _lib.PATH_FOURIER2D
    p['G'][2, 5, 5] = U                                     # an error leaves the caller's S alone
    rc, S, fl = host_call(arrays(p), strides(p), p)
    assert rc == -1 and np.array_equal(S, p['S0']) and 'member 2 holds undef' in last_error()
    q = dict(p, xc=14)
    rc, S, fl = host_call(arrays(p), strides(p), q)
    assert rc == -1 and 'row length 14 has the prime factor 7' in last_error()
    rc, S, fl = dev_call(arrays(p), strides(p), q)
    assert rc == -1 and 'row length 14 has the prime factor 7' in last_error() and np.array_equal(S.reshape(p['S0'].shape), p['S0'])


def test_shared_coefficients_equal_the_same_values_per_member():
    p = GM.problem(37, 125, 3, True, 17)
    rc, S, fl = run_dev(p)
    assert rc == 0 and not fl.any()
    per = dict(p, c=[np.ascontiguousarray(np.broadcast_to(x, (3, 37))) for x in p['c']])
    rc, S2, fl = run_dev(per)
    assert rc == 0 and not fl.any() and np.array_equal(S, S2)
    mixed = dict(p, c=[per['c'][0]] + list(p['c'][1:]))      # (one array per member, four shared: one set per member)
    rc, S3, fl = run_dev(mixed)
    assert rc == 0 and not fl.any() and np.array_equal(S, S3)


def test_more_members_than_one_launch_takes():
    """32768 members per launch of the three kernels: members 32768 .. 32770 are the second launch, whose member offset is
    not zero."""
    nb = 32768 + 3
    p = GM.problem(3, 4, nb, False, 21)
    rc, S, fl = run_dev(p)
    assert rc == 0 and not fl.any()
    for m in (0, 32767, 32768, 32770):
        rc1, S1, fl1 = run_dev(one_member(p, m))
        assert rc1 == 0 and not fl1.any() and np.array_equal(S1[0], S[m]), m
    Sm, _ = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    fe = float(np.linalg.norm((S - Sm).ravel()) / np.linalg.norm(Sm.ravel()))
    print('general 3 x 4 x %d: rel-L2(kernel, model) %.1e' % (nb, fe))
    assert fe <= 1e-12
    q = dict(p, G=p['G'].copy())
    q['G'][32769, 1, 2] = U
    rc, Sq, _ = run_dev(q)
    assert rc == -1 and 'member 32769 holds undef at 1 of the points the solve reads' in last_error(), last_error()
    assert np.array_equal(Sq, p['S0'])


WHERE = [('G', (1, 4, 7)), ('A', (1, 4)), ('C', (2, 1)), ('D', (0, 7)), ('E', (1, 3)), ('Fc', (2, 5)), ('S0', (2, 0, 3)),
         ('S0', (0, 8, 29))]


def with_value(p, name, idx, v):
    q = dict(p, S0=p['S0'].copy(), G=p['G'].copy(), c=[x.copy() for x in p['c']])
    arr = q[name] if name in ('S0', 'G') else q['c'][NAMES.index(name) - 1]
    arr[idx] = v
    return q


def test_undef_in_one_member_touches_no_members_field():
    p = GM.problem(9, 30, 3, False, 14)
    for name, idx in WHERE:
        q = with_value(p, name, idx, U)
        for entry in ('dev', 'host'):
            rc, S, fl = run_dev(q) if entry == 'dev' else host_call(arrays(q), strides(q), q)
            assert rc == -1, (entry, name, idx)
            assert 'member %d holds undef at 1 of the points the solve reads' % idx[0] in last_error(), (name, idx, last_error())
            assert np.array_equal(S, q['S0']), (entry, name, idx)


def test_undef_on_rows_that_are_not_read_changes_nothing():
    p = GM.problem(9, 30, 3, False, 14)
    rc, clean, fl = run_dev(p)
    assert rc == 0 and not fl.any()
    q = p
    for name in ('G', 'A', 'C', 'D', 'E', 'Fc'):
        for j in (0, 8):
            q = with_value(q, name, (slice(None), j), U)
    q = with_value(q, 'S0', (1, 4, 4), U)                   # (an interior first guess is not read either)
    rc, S, fl = run_dev(q)
    assert rc == 0 and not fl.any(), last_error()
    assert np.array_equal(S[:, 1:-1], clean[:, 1:-1])


def test_nan_in_one_members_forcing_sets_its_word_alone():
    p = GM.problem(9, 30, 3, False, 15)
    rc, good, fl = run_dev(p)
    assert rc == 0 and not fl.any()
    solo = [run_dev(one_member(p, m))[1][0] for m in range(3)]
    q = with_value(p, 'G', (1, 4, 7), np.nan)
    rc, S, fl = run_dev(q)
    assert rc == 0
    assert fl.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0]]
    for m in (0, 2):
        assert np.array_equal(S[m], solo[m]) and np.array_equal(S[m], good[m])
    assert not np.isfinite(S[1, 1:-1]).all()


def spread(a, stride):
    """[nb, ...] -> a flat buffer of nb * stride values, member m at m * stride, `undef` in between."""
    nb, n = a.shape[0], a[0].size
    buf = np.full(nb * stride, U)
    for m in range(nb):
        buf[m * stride:m * stride + n] = a[m].ravel()
    return buf


def test_members_that_lie_apart():
    """Members 1.5 slices apart in S and G and yc + 3 apart in the coefficients, `undef` in the gaps: a gap that is read makes
    the check pass refuse, a gap that is written differs afterwards."""
    yc, xc, nb = 6, 45, 3
    p = GM.problem(yc, xc, nb, False, 31)
    n = yc * xc
    rc, packed, fl = run_dev(p)
    assert rc == 0 and not fl.any()
    st = [n + n // 2] + [yc + 3] * 5 + [n + n // 2]
    wide = [spread(a, s) for a, s in zip(arrays(p), st)]
    for call in (dev_call, host_call):
        rc, Sbuf, fl = call(wide, st, p)
        assert rc == 0, (call.__name__, last_error())
        assert not fl.any()
        got = np.stack([Sbuf[m * st[0]:m * st[0] + n].reshape(yc, xc) for m in range(nb)])
        gap = np.concatenate([Sbuf[m * st[0] + n:(m + 1) * st[0]] for m in range(nb)])
        assert np.array_equal(got, packed), call.__name__
        assert (gap == U).all(), call.__name__


# ------------------------------------------------------------------ repeats and workspace growth
def test_a_queue_of_solves_of_different_lengths_repeats_its_bits():
    import torch
    st = torch.cuda.Stream()
    order = [(5, 4096), (6, 12), (5, 2160), (5, 4096), (6, 12), (37, 128), (6, 12), (37, 128)]
    ps = {s: GM.problem(s[0], s[1], 2, s[1] != 12, 900 + s[1]) for s in set(order)}
    first = {}
    for s in order:
        rc, S, fl = run_dev(ps[s], st)
        assert rc == 0 and not fl.any(), (s, last_error())
        if s in first:
            assert np.array_equal(S, first[s]), s
        first.setdefault(s, S)


def test_workspace_grows_between_two_solves_of_a_small_shape():
    """(4, 12) x 1 needs a few hundred doubles, 73 x 144 x 5 some 160 thousand: the buffer grows (unless an earlier test grew
    it) behind the first solve's event, on another stream; the third solve finds the larger buffer and the cached tables."""
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    small, large = GM.problem(4, 12, 1, False, 51), GM.gill_matsuno(73, 144, 5)
    S1 = check_solve_ld(small, a)
    rc, Sl, fl = run_dev(large, b)
    assert rc == 0 and not fl.any() and np.isfinite(Sl).all()
    S3 = check_solve_ld(small, a)
    assert np.array_equal(S1, S3)


# ------------------------------------------------------------------ the front end
def gm_field(ny, nx, members):
    """The heating of synthetic.gill_matsuno(ny, nx, members) as a Field (the same draws in the same order)."""
    rng = np.random.default_rng(synthetic.SEED)
    lat, lon = np.linspace(-90, 90, ny), np.linspace(0, 360, nx)
    la, lo = np.meshgrid(lat, lon, indexing='ij')
    Q = np.stack([0.05 * np.exp(-((la - rng.uniform(-20, 20)) ** 2 + (lo - rng.uniform(60, 300)) ** 2) / 100.0)
                  for _ in range(members)])
    return Field(Q, ('member', 'lat', 'lon'), {'lat': lat, 'lon': lon})


def rel(a, b):
    return float(np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel()))


@pytest.mark.parametrize('coords', ['lat-lon', 'cartesian'])
def test_front_end_gill_matsuno(capsys, coords):
    lines = [front_end_gill_matsuno(capsys, ny, nx, members, coords) for ny, nx, members in ((37, 72, 2), (73, 144, 3))]
    print('\n'.join(lines))                                  # (after the last read of the capture)


def front_end_gill_matsuno(capsys, ny, nx, members, coords):
    Q = gm_field(ny, nx, members)
    if coords == 'cartesian':
        Q = Field(Q.values, ('member', 'y', 'x'), {'y': np.deg2rad(np.asarray(Q['lat'])) * 6.371e6,
                                                    'x': np.deg2rad(np.asarray(Q['lon'])) * 6.371e6})
    dims = ['lat', 'lon'] if coords == 'lat-lon' else ['y', 'x']
    mP = {'epsilon': 1e-5, 'Phi': 5000}
    if coords == 'cartesian':
        mP = dict(mP, f0=0.0, beta=2.3e-11)
    run = lambda **kw: xa.invert_GillMatsuno(Q, dims=dims, coords=coords, mParams=mP, iParams=dict({'BCs': ['fixed', 'periodic']}, **kw))
    h = run(method='cfourier', residual=True)
    assert 'fourier solve' in capsys.readouterr().out
    fl = h.iParams['flags']
    assert fl.shape == (members, 3) and not fl.any()
    assert h.iParams['stats']['path'] == _lib.PATH_FOURIER2D and np.isfinite(h.values).all()
    # (optArg 1.4: the reference notebook's over-relaxation for this model; the front end's default overflows at 37 x 72)
    ref = run(method='sor', tolerance=1e-14, mxLoop=200000, optArg=1.4, printInfo=False)
    assert (ref.iParams['flags'][:, 0] == 0).all(), ref.iParams['flags']      # (a sweep count at mxLoop is rounding's floor)
    err = rel(h.values, ref.values)
    r = h.iParams['resid']
    line = ('front end gill-matsuno %s %d x %d x %d: rel-L2(cfourier, sor at 1e-14) %.1e (sor loops %d); max|R|/max|G| cfourier %.1e'
            % (coords, ny, nx, members, err, ref.iParams['flags'][:, 2].max(), (r[:, 2] / r[:, 3]).max()))
    assert err <= 1e-6
    plain = run(method='cfourier', printInfo=False)           # (without the residual: the same field)
    assert np.array_equal(plain.values, h.values)
    return line


def test_front_end_answers_where_the_reference_sweeps_overflow():
    """synthetic.gill_matsuno(19, 30, 1): the oracle's lexicographic sweeps overflow; the direct solve returns a finite field
    whose backward error meets the 4x bar.  (Nothing is asserted about how the GPU's 'sor' fails.)"""
    p = GM.gill_matsuno(19, 30, 1)
    Q = gm_field(19, 30, 1)
    h = xa.invert_GillMatsuno(Q, dims=['lat', 'lon'], coords='lat-lon', mParams={'epsilon': 1e-5, 'Phi': 5000},
                              iParams={'BCs': ['fixed', 'periodic'], 'method': 'cfourier', 'printInfo': False})
    assert np.isfinite(h.values).all() and not np.asarray(h.iParams['flags']).any()
    Sm, _ = GM.solve(p['S0'], p['c'], p['G'], p['sc'], U)
    be_k = T.ld_backward(h.values, p['c'], p['G'], p['sc']).astype(np.float64)
    be_m = T.ld_backward(Sm, p['c'], p['G'], p['sc']).astype(np.float64)
    print('front end gill-matsuno 19 x 30: backward error in long double cfourier %.2e model %.2e' % (be_k.max(), be_m.max()))
    assert (be_k <= 4 * np.maximum(be_m, HALF_ULP)).all(), (be_k, be_m)


def test_inv_general2d_on_bare_arrays_is_the_abi_call():
    p = GM.gill_matsuno(37, 72, 2)
    full_p = synthetic.gill_matsuno(37, 72, 2)
    dims3 = ('member', 'lat', 'lon')
    co = {'lat': full_p['lat'], 'lon': full_p['lon']}
    G, S = Field(p['G'].copy(), dims3, co), Field(p['S0'].copy(), dims3, co)
    A, B, C, D, E, Fc = full_p['coefs'][:6]
    ip = dict(BCs=['fixed', 'periodic'], method='cfourier', printInfo=False, del1=p['sc'][0], del1Sqr=p['sc'][1], ratio=p['sc'][2],
              ratioSqr=p['sc'][3], mxLoop=1, tolerance=1e-9)
    out = core.inv_general2D(A, B, C, D, E, Fc, G, S, ['lat', 'lon'], ip)
    rc, Sd, fl = run_dev(p)
    assert rc == 0 and not fl.any()
    assert np.array_equal(out.values, Sd) and np.array_equal(np.asarray(ip['flags']), fl)
