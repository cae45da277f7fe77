"""The direct Fourier solve at the edges of its parameter space (k_rowdft, k_fourier_tri, k_fourier_check):
every radix schedule of fourier_factor, the dynamic-LDS limit raised and lowered, the refusals, the solve against a
long-double truth (tests/fourier_ld.py) at every pairing of interior rows and on both sides of k_fourier_tri's 64 lanes,
more members than one launch takes, members that lie apart in memory, a non-finite row at a member's border, and the
workspace shared between shapes and streams.  The helpers are those of tests/test_gpu_fourier.py.

Measured on an MI355X (python -m pytest tests/test_gpu_fourier_edges.py -s prints every figure; DESIGN.md 4.16 records them).
"""
import ctypes

import numpy as np
import pytest

import fourier_ld as T
import fourier_model as M
from xinvert_amd import _lib, fourier
from test_gpu_fourier import U, check_solve, gpu_rfft, gpu_roundtrip, problem, rel, run_dev, strides

pytestmark = pytest.mark.gpu
HALF_ULP = 2.0 ** -53                 # the relative error of rounding the long-double truth to double


# ------------------------------------------------------------------ the row transform
SCHEDULES = {2: [2], 8: [4, 2], 2048: [4] * 5 + [2], 2160: [4, 4, 3, 3, 3, 5], 2187: [3] * 7, 4096: [4] * 6}
LENGTHS = [2, 6, 8, 9, 10, 16, 25, 27, 32, 120, 125, 128, 243, 256, 625, 1024, 2048, 2160, 2187, 3125, 4000, 4050, 4096]


def within_8x(what, n, rows, mine, numpys):
    """The rule of test_gpu_fourier.check_transform with a floor: numpy's error, or one rounding of the truth."""
    bar = 8 * max(numpys, HALF_ULP)
    assert mine <= bar, (what, n, rows, mine, numpys)


def check_transform_floor(n, rows):
    x = np.random.default_rng(1000 * n + rows).standard_normal((rows, n))
    truth = T.dft_longdouble(x)
    e_np, e_k = T.err_ld(np.fft.rfft(x), truth), T.err_ld(gpu_rfft(x), truth)
    r_np, r_k = rel(np.fft.irfft(np.fft.rfft(x), n), x), rel(gpu_roundtrip(x), x)
    print('rowdft n %4d rows %3d %-22s: error kernel %.2e numpy %.2e (x%.2f); round trip kernel %.2e numpy %.2e (x%.2f)'
          % (n, rows, M.factor(n), e_k, e_np, e_k / max(e_np, HALF_ULP), r_k, r_np, r_k / max(r_np, HALF_ULP)))
    within_8x('error', n, rows, e_k, e_np)
    within_8x('round trip', n, rows, r_k, r_np)


@pytest.mark.parametrize('n', LENGTHS)
def test_rowdft_every_schedule(n):
    if n in SCHEDULES:
        assert M.factor(n) == SCHEDULES[n]                  # (the schedules these lengths were chosen for)
    for rows in ((1, 2, 3, 130) if n <= 256 else (1, 2, 3) if n <= 1024 else (1, 3)):
        check_transform_floor(n, rows)


def test_schedules_cover_what_they_were_chosen_for():
    """The lengths above, by the property each one brings: a lone radix-2 pass, radix 2 behind radix 4, pure radix 3 and 5,
    seven passes, both parities of the pass count (the ping-pong buffer the result ends in), 256 butterflies in a pass, a
    last pass of fewer butterflies than one wavefront."""
    f = {n: M.factor(n) for n in LENGTHS}
    assert f[2] == [2] and f[8] == [4, 2] and f[32] == [4, 4, 2] and f[128] == [4, 4, 4, 2]
    assert all(set(f[n]) == {3} for n in (9, 27, 243, 2187)) and all(set(f[n]) == {5} for n in (25, 125, 625, 3125))
    assert max(len(v) for v in f.values()) == 7 == len(f[2187]) == len(f[4050])
    assert {len(v) % 2 for v in f.values()} == {0, 1}
    assert 1024 // 4 == 256 and f[1024] == [4] * 5
    assert 120 // f[120][-1] < 64 and 10 // f[10][-1] < 64


def test_lds_limit_raised_and_lowered_on_one_stream():
    """n = 2048 takes exactly 64 KiB and leaves the limit alone, 2160 is the smallest length that raises it, 4096 the
    largest: long, shorter, long again, short, all queued on one stream; every repeat gives the bits of its first run."""
    import torch
    order = [4096, 2160, 4096, 2048, 12, 4096, 12]
    x = {n: np.random.default_rng(77 + n).standard_normal((3, n)) for n in set(order)}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dev = {n: torch.from_numpy(x[n]).cuda() for n in x}
        spec = [fourier.rfft_rows(dev[n]) for n in order]
        back = [fourier.irfft_rows(X, n) for X, n in zip(spec, order)]
    st.synchronize()
    first = {}
    for n, X, b in zip(order, spec, back):
        X, b = X.cpu().numpy(), b.cpu().numpy()
        if n in first:
            assert np.array_equal(X, first[n][0]) and np.array_equal(b, first[n][1]), n
            continue
        first[n] = (X, b)
        truth = T.dft_longdouble(x[n])
        e_np, e_k = T.err_ld(np.fft.rfft(x[n]), truth), T.err_ld(X, truth)
        r_np, r_k = rel(np.fft.irfft(np.fft.rfft(x[n]), n), x[n]), rel(b, x[n])
        print('lds limit n %4d: error kernel %.2e numpy %.2e; round trip kernel %.2e numpy %.2e' % (n, e_k, e_np, r_k, r_np))
        within_8x('error', n, 3, e_k, e_np)
        within_8x('round trip', n, 3, r_k, r_np)


def test_refused_lengths_leave_the_output_and_the_next_call_alone():
    import torch
    L = _lib.require_gpu()
    x = np.random.default_rng(5).standard_normal((2, 12))
    good = gpu_rfft(x)
    for n, words in ((1, [b'at least 2 points']), (4320, [b'4320', b'LDS budget']), (4097, [b'4097', b'prime factor 17'])):
        src = torch.ones((2, n), dtype=torch.float64, device='cuda')
        out = torch.full((2, 2 * (n // 2 + 1)), 7.0, dtype=torch.float64, device='cuda')
        for inverse in (0, 1):
            rc = L.xinv_rowdft_f64_dev(_lib.dptr(out), _lib.dptr(src), 2, n, inverse, None)
            msg = L.xinv_last_error()
            assert rc == -1 and all(w in msg for w in words), (n, msg)
        torch.cuda.synchronize()
        assert (out == 7.0).all()
        with pytest.raises(_lib.XinvError, match=words[-1].decode()):
            fourier.rfft_rows(src)
        # a good call behind the refusal: rc 0, the bits of before, and xinv_last_error untouched by it
        dx = torch.from_numpy(x).cuda()
        dX = torch.empty((2, 7), dtype=torch.complex128, device='cuda')
        assert L.xinv_rowdft_f64_dev(_lib.dptr(dX), _lib.dptr(dx), 2, 12, 0, None) == 0
        assert np.array_equal(dX.cpu().numpy(), good)
        assert L.xinv_last_error() == msg
    for n, word in ((1, 'at least 2 points'), (4320, 'LDS budget'), (4097, 'prime factor 17')):      # the model, in the same words
        with pytest.raises(ValueError, match=word):
            M.factor(n)


# ------------------------------------------------------------------ the solve against the long-double truth
def rel_ld(S, truth):
    d = np.asarray(S).astype(T.LD) - truth
    return float(np.sqrt((d * d).sum() / (truth * truth).sum()))


def check_solve_ld(p):
    """Forward error (relative L2 against ld_solve) within 8x the model's, backward error (ld_backward, per member) within
    4x the model's -- the margins of check_transform and check_solve --, each with one rounding of the truth as its floor."""
    sc = (p['delxSqr'], p['ratioSqr'])
    St = T.ld_solve(p['S0'], p['A'], p['C'], p['F'], *sc)
    Sm, flm = M.solve(p['S0'], p['A'], p['C'], p['F'], *sc, U)
    rc, S, fl, _ = run_dev(p)
    assert rc == 0, _lib.load().xinv_last_error()
    assert _lib.last_stats()['path'] == _lib.PATH_FOURIER2D
    assert not fl.any() and not flm.any()
    assert np.array_equal(S[:, 0], p['S0'][:, 0]) and np.array_equal(S[:, -1], p['S0'][:, -1])
    fe_k, fe_m = rel_ld(S, St), rel_ld(Sm, St)
    be_k, be_m = (T.ld_backward(X, p['A'], p['C'], p['F'], *sc).astype(np.float64) for X in (S, Sm))
    print('fourier %3d x %3d x %d: rel-L2 to the truth kernel %.2e model %.2e; max|R|/max|F| in long double kernel %.2e model %.2e'
          % (p['yc'], p['xc'], p['nb'], fe_k, fe_m, be_k.max(), be_m.max()))
    assert fe_k <= 8 * max(fe_m, HALF_ULP), (fe_k, fe_m)
    assert (be_k <= 4 * np.maximum(be_m, HALF_ULP)).all(), (be_k, be_m)
    return S


@pytest.mark.parametrize('xc', [3, 4, 6, 8, 120, 125, 128, 256])
@pytest.mark.parametrize('yc', [3, 4, 5, 6])
def test_solve_against_the_long_double_truth(yc, xc):
    """1 .. 4 interior rows (a lone row, a pair, a pair and a lone row, two pairs); K = 2 .. 5, 61, 63, 65 and 129
    wavenumbers (the last lane of a workgroup of k_fourier_tri, one lane into the second, a third workgroup)."""
    check_solve_ld(problem(yc, xc, 2, False, 7000 + 10 * xc + yc))


@pytest.mark.parametrize('yc,xc', [(300, 12), (130, 45)])
def test_tall_solve_against_the_long_double_truth(yc, xc):
    check_solve_ld(problem(yc, xc, 1, False, 7000 + 10 * xc + yc))


@pytest.mark.parametrize('yc,xc', [(5, 2048), (4, 2160), (5, 4096)])
def test_solve_at_the_lds_edges(yc, xc):
    check_solve(problem(yc, xc, 1, True, 100 * yc + xc))


def test_workspace_grows_between_two_solves_of_a_small_shape():
    """ws->four holds 3 * yc * K doubles per member: (4, 12) x 1 needs 84, (37, 360) x 5 needs 100455, so the buffer grows --
    behind the first solve's event, on another stream -- and the third solve finds the larger buffer and the cached table.
    (This test stands before the 32771 members below, and 181 x 360 x 1 of tests/test_gpu_fourier.py needs 98283: in the
    suite's order the buffer does grow here.)"""
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    small, large = problem(4, 12, 1, False, 51), problem(37, 360, 5, False, 52)
    S1 = check_solve(small, a)
    check_solve(large, b)
    S3 = check_solve(small, a)
    assert np.array_equal(S1, S3)


# ------------------------------------------------------------------ members
def one_member(p, m):
    return dict(p, S0=p['S0'][m:m + 1], A=p['A'][m:m + 1], C=p['C'][m:m + 1], F=p['F'][m:m + 1], nb=1)


def test_more_members_than_one_launch_takes():
    """FOURIER_MEMBER_CHUNK = 32768 members per launch of k_fourier_tri and k_fourier_check: members 32768 .. 32770 are the
    second launch, whose member offset is not zero."""
    nb = 32768 + 3
    p = problem(3, 4, nb, False, 21)
    rc, S, fl, _ = run_dev(p)
    assert rc == 0 and not fl.any()
    for m in (0, 32767, 32768, 32770):
        rc1, S1, fl1, _ = run_dev(one_member(p, m))
        assert rc1 == 0 and not fl1.any() and np.array_equal(S1[0], S[m]), m
    Sm, _ = M.solve(p['S0'], p['A'], p['C'], p['F'], p['delxSqr'], p['ratioSqr'], U)
    fe = rel(S, Sm)
    print('fourier 3 x 4 x %d: rel-L2(kernel, model) %.1e' % (nb, fe))
    assert fe <= 1e-12

    q = dict(p, F=p['F'].copy())
    q['F'][32769, 1, 2] = U
    rc, Sq, _, _ = run_dev(q)
    assert rc == -1
    msg = _lib.load().xinv_last_error().decode()
    assert 'member 32769 holds undef at 1 of the points the solve reads' in msg, msg
    assert np.array_equal(Sq, p['S0'])

    q = dict(p, A=p['A'].copy())
    q['A'][32768, 1] = np.nan
    rc, Sq, fl, _ = run_dev(q)
    assert rc == 0
    want = np.zeros((nb, 3))
    want[32768, 0] = 1
    assert np.array_equal(fl, want)
    others = np.arange(nb) != 32768
    assert np.array_equal(Sq[others], S[others]) and not np.isfinite(Sq[32768, 1]).all()


def spread(a, stride):
    """[nb, ...] -> a flat buffer of nb * stride values, member m at m * stride, `undef` in between."""
    nb, n = a.shape[0], a[0].size
    buf = np.full(nb * stride, U)
    for m in range(nb):
        buf[m * stride:m * stride + n] = a[m].ravel()
    return buf


def gaps(buf, nb, n, stride):
    return np.concatenate([buf[m * stride + n:(m + 1) * stride] for m in range(nb)])


def members(buf, nb, shape, stride):
    n = int(np.prod(shape))
    return np.stack([buf[m * stride:m * stride + n].reshape(shape) for m in range(nb)])


def dev_call(arrays, st, p):
    """xinv_fourier_standard_2d_f64_dev on flat host buffers (S, A, C, F) with the strides `st` -> (rc, S buffer, flags)."""
    import torch
    L = _lib.require_gpu()
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    fl = np.full((p['nb'], 3), -1.0)
    rc = L.xinv_fourier_standard_2d_f64_dev(*[_lib.dptr(a) for a in t], p['nb'], _lib.strides_arg(st), p['yc'], p['xc'],
                                            p['delxSqr'], p['ratioSqr'], U, _lib.hptr(fl),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, t[0].cpu().numpy(), fl


def host_call(arrays, st, p):
    L = _lib.require_gpu()
    S = arrays[0].copy()
    fl = np.full((p['nb'], 3), -1.0)
    rc = L.xinv_fourier_standard_2d_f64_batched(_lib.hptr(S), *[_lib.hptr(np.ascontiguousarray(a)) for a in arrays[1:]], p['nb'],
                                                _lib.strides_arg(st), p['yc'], p['xc'], p['delxSqr'], p['ratioSqr'], U,
                                                _lib.hptr(fl), _lib.options())
    return rc, S, fl


def test_members_that_lie_apart_and_a_shared_forcing():
    """Members 1.5 slices apart in S and F and yc + 3 apart in A and C, `undef` in the gaps: a gap that is read makes the
    check pass refuse, a gap that is written differs afterwards.  Then one forcing for three pairs of boundary rows."""
    yc, xc, nb = 6, 45, 3
    p = problem(yc, xc, nb, False, 31)
    n = yc * xc
    rc, packed, fl, _ = run_dev(p)
    assert rc == 0 and not fl.any()
    st = [n + n // 2, yc + 3, yc + 3, n + n // 2]
    wide = [spread(p[k], s) for k, s in zip(('S0', 'A', 'C', 'F'), st)]
    for call in (dev_call, host_call):
        rc, Sbuf, fl = call(wide, st, p)
        assert rc == 0, (call.__name__, _lib.load().xinv_last_error())
        assert not fl.any()
        assert np.array_equal(members(Sbuf, nb, (yc, xc), st[0]), packed), call.__name__
        assert (gaps(Sbuf, nb, n, st[0]) == U).all(), call.__name__

    # F with stride 0: the bits of three packed copies of it
    one_f = dict(p, F=np.ascontiguousarray(np.broadcast_to(p['F'][1], p['F'].shape)))
    rc, copies, fl, _ = run_dev(one_f)
    assert rc == 0 and not fl.any()
    assert not np.array_equal(copies[0], copies[2])             # (the boundary rows and the coefficients differ)
    shared = [p['S0'].ravel(), p['A'].ravel(), p['C'].ravel(), p['F'][1].ravel()]
    for call in (dev_call, host_call):
        rc, Sbuf, fl = call(shared, strides(p)[:3] + [0], p)
        assert rc == 0, (call.__name__, _lib.load().xinv_last_error())
        assert not fl.any() and np.array_equal(Sbuf.reshape(nb, yc, xc), copies), call.__name__


def test_a_non_finite_row_stays_in_its_member():
    """Three interior rows: rows 1 and 2 of a member share a transform, row 3 is transformed alone -- never with row 1 of
    the next member; rows 0 and yc-1 of S are a pair of their own."""
    p = problem(5, 30, 3, False, 41)
    rc, good, fl, _ = run_dev(p)
    assert rc == 0 and not fl.any()
    for name, idx in (('F', (0, 3, 7)), ('F', (1, 1, 7)), ('S0', (2, 4, 7))):
        q = dict(p, **{name: p[name].copy()})
        q[name][idx] = np.inf
        rc, S, fl, _ = run_dev(q)
        assert rc == 0, (name, idx)
        want = np.zeros((3, 3))
        want[idx[0], 0] = 1
        assert np.array_equal(fl, want), (name, idx, fl)
        keep = [m for m in range(3) if m != idx[0]]
        assert np.array_equal(S[keep], good[keep]), (name, idx)
        assert not np.isfinite(S[idx[0], 1:-1]).all()
