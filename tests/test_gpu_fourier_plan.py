"""Fourier plans on the GPU (k_fourier_factor, k_fourier_subst, k_rowdft's per-member skip; DESIGN.md 4.16, "Plans"): every
result is compared BITWISE, on all of S, with the one-shot entry xinv_fourier_standard_2d_f64_dev, which the existing files
hold to the long-double truth.  The stored-factor march evaluates the one-shot kernel's expressions in its order, so no
tolerance appears anywhere in this file.
"""
import ctypes

import numpy as np
import pytest

import xinvert_amd as xa
from xinvert_amd import _lib, synthetic
from xinvert_amd.resident import ResidentProblem

pytestmark = pytest.mark.gpu
U = -9.99e8
SC = dict(delxSqr=1.21, ratioSqr=(1.1 / 1.3) ** 2)


def problem(yc, xc, nb, shared, seed):
    """-> dict(S0, F [nb, yc, xc], A, C [yc] or [nb, yc], ...): random boundary rows and first guess."""
    rng = np.random.default_rng(seed)
    A, C = rng.uniform(0.5, 1.5, (nb, yc)), rng.uniform(0.5, 1.5, (nb, yc))
    if shared:
        A, C = A[0].copy(), C[0].copy()
    F = rng.standard_normal((nb, yc, xc))
    S0 = rng.standard_normal((nb, yc, xc)) * np.abs(F).max() * SC['delxSqr']
    return dict(SC, S0=S0, F=F, A=A, C=C, nb=nb, yc=yc, xc=xc)


def solo(p, m):
    """Member m of a batch as a problem of its own."""
    pick = lambda a: a if a.ndim == 1 else a[m].copy()
    return dict(p, S0=p['S0'][m:m + 1].copy(), F=p['F'][m:m + 1].copy(), A=pick(p['A']), C=pick(p['C']), nb=1)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def one_shot(p):
    """xinv_fourier_standard_2d_f64_dev -> (rc, S, flags)"""
    import torch
    L = _lib.require_gpu()
    t = {k: dev(p[k]) for k in ('S0', 'A', 'C', 'F')}
    torch.cuda.synchronize()
    n = p['yc'] * p['xc']
    st = [n, p['yc'] if p['A'].ndim == 2 else 0, p['yc'] if p['C'].ndim == 2 else 0, n]
    fl = np.full((p['nb'], 3), -1.0)
    rc = L.xinv_fourier_standard_2d_f64_dev(_lib.dptr(t['S0']), _lib.dptr(t['A']), _lib.dptr(t['C']), _lib.dptr(t['F']), p['nb'],
                                            _lib.strides_arg(st), p['yc'], p['xc'], p['delxSqr'], p['ratioSqr'], U,
                                            _lib.hptr(fl), None)
    return rc, t['S0'].cpu().numpy(), fl


def reference(p):
    rc, S, fl = one_shot(p)
    assert rc == 0, _lib.load().xinv_last_error()
    return S, fl


def make_plan(p):
    return xa.FourierPlan(p['A'], p['C'], p['nb'], p['yc'], p['xc'], p['delxSqr'], p['ratioSqr'], undef=U)


def plan_solve(plan, p, F=None, stream=None):
    """One solve of `plan` on fresh copies of the problem's S0 and forcing -> (S, flags, bad)."""
    S, Ft = dev(p['S0']), dev(p['F'] if F is None else F)
    import torch
    torch.cuda.synchronize()
    plan.solve(S, Ft, stream=stream)
    fl, bad = plan.status()
    return S.cpu().numpy(), fl, bad


def check(p):
    ref, flr = reference(p)
    plan = make_plan(p)
    S, fl, bad = plan_solve(plan, p)
    plan.close()
    assert not bad.any() and np.array_equal(fl, flr), (p['yc'], p['xc'], p['nb'])
    assert np.array_equal(S, ref), (p['yc'], p['xc'], p['nb'], int((S != ref).sum()))


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-member'])
@pytest.mark.parametrize('xc', [3, 4, 6, 8, 60, 64, 120, 125, 128, 256])
def test_short_marches_around_the_wavefront_edges(xc, shared):
    """2K = 62, 66, 122, 126, 130, 258 lie around 64, 128 and 256 lanes; yc = 3 has one interior row, the first and the last
    of the march at once; yc = 4 .. 6 lie within one batch of rows loaded ahead."""
    for yc in (3, 4, 5, 6):
        for nb in (1, 2, 3):
            check(problem(yc, xc, nb, shared, 10000 * yc + 10 * xc + nb))


@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-member'])
@pytest.mark.parametrize('yc,xc', [(300, 12), (130, 45), (10, 12), (11, 12), (18, 12), (19, 12)],
                         ids=lambda v: str(v))
def test_tall_marches(yc, xc, shared):
    """Many batches of rows; yc - 2 = 8, 9, 16, 17 are the batch length, its multiple, and one more."""
    check(problem(yc, xc, 2, shared, 100 * yc + xc))


@pytest.mark.parametrize('yc,xc', [(5, 4096), (4, 2160)], ids=['5x4096', '4x2160'])
def test_lds_edge_of_the_transform_under_skip(yc, xc):
    p = problem(yc, xc, 2, False, yc + xc)
    check(p)
    want = reference(solo(p, 1))[0]
    p['F'][0, 1, xc - 1] = U                                 # member 0 is skipped by the inverse transform
    plan = make_plan(p)
    S = dev(p['S0'])
    plan.solve(S, dev(p['F']))
    with pytest.raises(_lib.XinvError, match='member 0 holds undef at 1 of the points'):
        plan.status()
    plan.close()
    S = S.cpu().numpy()
    assert np.array_equal(S[0], p['S0'][0]) and np.array_equal(S[1], want[0])


# ------------------------------------------------------------------ reuse
def test_one_plan_three_forcings():
    p = problem(37, 45, 3, False, 21)
    F2 = np.random.default_rng(22).standard_normal(p['F'].shape)
    ref1, ref2 = reference(p)[0], reference(dict(p, F=F2))[0]
    plan = make_plan(p)
    a, b, c = plan_solve(plan, p)[0], plan_solve(plan, p, F=F2)[0], plan_solve(plan, p)[0]
    plan.close()
    assert np.array_equal(a, ref1) and np.array_equal(b, ref2) and np.array_equal(c, a)


def test_two_plans_alive_together_interleaved_on_two_streams():
    import torch
    p, q = problem(37, 45, 2, False, 23), problem(6, 128, 3, True, 24)
    ref_p, ref_q = reference(p)[0], reference(q)[0]
    plan_p, plan_q = make_plan(p), make_plan(q)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    Sp = [dev(p['S0']) for _ in range(3)]
    Sq = [dev(q['S0']) for _ in range(3)]
    Fp, Fq = dev(p['F']), dev(q['F'])
    torch.cuda.synchronize()
    for k in range(3):
        plan_p.solve(Sp[k], Fp, stream=s1)
        plan_q.solve(Sq[k], Fq, stream=s2)
    assert not plan_p.status()[0].any() and not plan_q.status()[0].any()
    for k in range(3):
        assert np.array_equal(Sp[k].cpu().numpy(), ref_p) and np.array_equal(Sq[k].cpu().numpy(), ref_q), k
    plan_p.close()
    plan_q.close()


def test_one_plan_on_two_streams_without_a_host_wait():
    """The spectrum is the plan's: the solve on s2 is ordered behind the one on s1 by the plan's event."""
    import torch
    p = problem(130, 45, 3, False, 25)
    F2 = np.random.default_rng(26).standard_normal(p['F'].shape)
    ref1, ref2 = reference(p)[0], reference(dict(p, F=F2))[0]
    plan = make_plan(p)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    Sa, Sb, Fa, Fb = dev(p['S0']), dev(p['S0']), dev(p['F']), dev(F2)
    torch.cuda.synchronize()
    plan.solve(Sa, Fa, stream=s1)
    plan.solve(Sb, Fb, stream=s2)
    fl, bad = plan.status()
    s1.synchronize()
    plan.close()
    assert not fl.any() and not bad.any()
    assert np.array_equal(Sa.cpu().numpy(), ref1) and np.array_equal(Sb.cpu().numpy(), ref2)


# ------------------------------------------------------------------ layout
def test_members_one_and_a_half_slices_apart_and_the_gaps_stay():
    import torch
    p = problem(9, 30, 3, False, 27)
    ref = reference(p)[0]
    n = 9 * 30
    gap = n + n // 2
    buf = torch.full((3 * gap,), U, dtype=torch.float64, device='cuda')
    S = torch.as_strided(buf, (3, 9, 30), (gap, 30, 1))
    S.copy_(dev(p['S0']))
    plan = make_plan(p)
    plan.solve(S, dev(p['F']))
    fl, bad = plan.status()
    plan.close()
    assert not fl.any() and not bad.any()
    out = buf.cpu().numpy().reshape(3, gap)
    assert np.array_equal(out[:, :n].reshape(3, 9, 30), ref)
    assert (out[:, n:] == U).all()


def test_one_forcing_for_three_members_with_their_own_boundary_rows():
    p = problem(9, 30, 3, True, 28)
    p['F'] = np.ascontiguousarray(np.broadcast_to(p['F'][0], p['F'].shape))
    ref = reference(p)[0]
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])
    plan = make_plan(p)
    S, fl, bad = plan_solve(plan, p, F=p['F'][0])            # [yc, xc]: sF = 0
    plan.close()
    assert not fl.any() and np.array_equal(S, ref)


# ------------------------------------------------------------------ faults in the data
def test_undef_in_one_members_forcing_leaves_that_member_alone():
    p = problem(9, 30, 3, False, 29)
    want = [reference(solo(p, m))[0][0] for m in (0, 2)]
    p['F'][1, 4, 7] = U
    plan = make_plan(p)
    S = dev(p['S0'])
    plan.solve(S, dev(p['F']))
    with pytest.raises(_lib.XinvError, match='member 1 holds undef at 1 of the points the solve reads') as ei:
        plan.status()
    assert str(ei.value).endswith('a masked problem is for the sweeps')
    assert plan.bad.tolist() == [0, 1, 0]
    S = S.cpu().numpy()
    assert np.array_equal(S[1], p['S0'][1])
    assert np.array_equal(S[0], want[0]) and np.array_equal(S[2], want[1])
    # the boundary rows of S are read too; the plan goes on working afterwards
    q = problem(9, 30, 3, False, 29)
    q['S0'][2, 8, 29] = U
    Sq = dev(q['S0'])
    plan.solve(Sq, dev(q['F']))
    with pytest.raises(_lib.XinvError, match='member 2 holds undef'):
        plan.status()
    assert plan.bad.tolist() == [0, 0, 1] and np.array_equal(Sq.cpu().numpy()[2], q['S0'][2])
    clean = problem(9, 30, 3, False, 29)
    S, fl, bad = plan_solve(plan, clean)
    plan.close()
    assert not bad.any() and np.array_equal(S, reference(clean)[0])


def test_nan_in_one_members_forcing_sets_that_members_flag_alone():
    p = problem(9, 30, 3, False, 30)
    good = reference(p)[0]
    p['F'][2, 3, 3] = np.nan
    ref, flr = reference(p)
    plan = make_plan(p)
    S, fl, bad = plan_solve(plan, p)
    plan.close()
    assert fl.tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]] and np.array_equal(fl, flr) and not bad.any()
    assert np.array_equal(S[[0, 1]], good[[0, 1]]) and np.array_equal(S, ref, equal_nan=True)


def test_nan_in_shared_a_sets_every_members_flag():
    p = problem(9, 30, 3, True, 31)
    p['A'][4] = np.nan
    plan = make_plan(p)
    S, fl, bad = plan_solve(plan, p)
    plan.close()
    assert fl[:, 0].tolist() == [1, 1, 1] and not bad.any()
    assert np.array_equal(fl, reference(p)[1])


def test_undef_in_a_refuses_the_plan_and_the_next_create_works():
    L = _lib.require_gpu()
    p = problem(9, 30, 3, False, 32)
    ref = reference(p)[0]
    for name, idx, member in (('A', (2, 8), 2), ('C', (1, 1), 1), ('A', (0, 1), 0)):
        q = problem(9, 30, 3, False, 32)
        q[name][idx] = U
        with pytest.raises(_lib.XinvError, match='member %d holds undef at 1 of the points the plan reads' % member):
            make_plan(q)
    A, C = dev(p['A']), dev(p['C'])
    A[1, 3] = U
    h = ctypes.c_void_p()
    rc = L.xinv_fourier_plan_create_standard_2d_f64_dev(ctypes.byref(h), _lib.dptr(A), _lib.dptr(C), 3, _lib.strides_arg([9, 9]),
                                                        9, 30, p['delxSqr'], p['ratioSqr'], U, None)
    assert rc == -1 and h.value is None                        # (no handle: nothing for the caller to free)
    q = problem(9, 30, 3, False, 32)                         # rows the solve never reads
    q['A'][1, 0] = q['C'][1, 0] = q['C'][2, 8] = U
    plan = make_plan(q)
    S, fl, bad = plan_solve(plan, q)
    plan.close()
    assert not fl.any() and np.array_equal(S, ref)


def test_solve_refuses_what_does_not_fit_the_plan():
    import torch
    p = problem(9, 30, 3, False, 33)
    plan = make_plan(p)
    S, F = dev(p['S0']), dev(p['F'])
    with pytest.raises(_lib.XinvError, match='S must be'):
        plan.solve(S[:2], F)
    with pytest.raises(_lib.XinvError, match='S must be'):
        plan.solve(S.transpose(1, 2), F)
    with pytest.raises(_lib.XinvError, match='F must be'):
        plan.solve(S, F[:, :, :12])
    with pytest.raises(_lib.XinvError, match='float64'):
        plan.solve(S, F.float())
    before = _lib.last_stats()
    plan.solve(S, F)
    assert _lib.last_stats() == before                         # a solve knows nothing yet: the stats stay
    assert not plan.status()[0].any()
    plan.close()
    with pytest.raises(_lib.XinvError, match='closed'):
        plan.solve(S, F)


# ------------------------------------------------------------------ the front end
def quick_start(seed, ny=19, nx=30, nb=2):
    return synthetic.poisson_latlon(ny, nx, mask=False, seed=seed, members=nb)


def front_end(p):
    vor = xa.Field(p['zeta'], ('member', 'lat', 'lon'), {'lat': p['lat'], 'lon': p['lon']})
    out = xa.invert_Poisson(vor, dims=['lat', 'lon'], coords='lat-lon',
                            iParams={'BCs': ['fixed', 'periodic'], 'method': 'fourier', 'printInfo': False})
    return np.asarray(out.values)


def test_resident_problem_solves_the_quick_start_with_the_front_ends_bits():
    import torch
    p, p2 = quick_start(41), quick_start(42)
    want, want2 = front_end(p), front_end(p2)
    rp = ResidentProblem(p)
    fl = rp.solve_fourier()
    assert fl.shape == (2, 3) and not fl.any()
    assert np.array_equal(rp.result(), want)
    plan = rp._fplan
    # a new forcing written in place: no refresh, the same plan
    rp.coefs[-1].copy_(torch.from_numpy(np.ascontiguousarray(p2['coefs'][-1], dtype=np.float64)))
    assert rp.solve_fourier(wait=False) is None
    assert not rp.fourier_status().any() and rp._fplan is plan
    assert np.array_equal(rp.result(), want2)
    # the sweeps and the direct solve alternate on one object; the direct solve does not read the interior
    rp.reset()
    rp.solve(20, 1e-30)
    assert not np.array_equal(rp.result(), want2)
    rp.solve_fourier(stream=torch.cuda.Stream())
    assert np.array_equal(rp.result(), want2)
    fl, _ = rp.solve(5, 1e-30)
    assert (fl[:, 2] <= 5).all() and np.isfinite(rp.result()).all()
    rp.refresh()
    assert rp._fplan is None
    rp.solve_fourier()
    assert np.array_equal(rp.result(), want2)
    rp.close()
    assert rp._fplan is None


def test_resident_problem_refuses_what_the_front_end_refuses():
    base = quick_start(43, 9, 12)
    dense = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    cases = {
        'non-zero B': (dict(base, coefs=[base['coefs'][0], np.full((9, 12), 0.01)] + base['coefs'][2:]), 'B must be identically zero'),
        'extend y': (dict(base, BCy='extend'), "along y is 'extend'"),
        'fixed x': (dict(base, BCx='fixed'), "along x is 'fixed'"),
        'A varies': (dict(base, coefs=[dense(base['coefs'][0]) * (1 + 0.01 * (np.arange(12) == 5))] + base['coefs'][1:]),
                     'A must be constant along x'),
        'xc = 14': (quick_start(43, 9, 14), 'the row length 14 has the prime factor 7'),
    }
    for name, (p, words) in cases.items():
        rp = ResidentProblem(p)
        with pytest.raises(Exception, match=words) as ei:
            rp.solve_fourier()
        assert "'sor' solves this case" in str(ei.value), name
        rp.solve(3, 1e-30)                                   # ... and the sweeps do
        rp.close()
    rp = ResidentProblem(dict(base, coefs=[dense(c) for c in base['coefs']]), plan=False)     # dense arrays, constant along x
    assert not rp.solve_fourier().any()
    want = front_end(base)
    assert np.array_equal(rp.result(), want)
    rp.close()
    g = synthetic.gill_matsuno(9, 12, 1)
    rp = ResidentProblem(g)
    with pytest.raises(_lib.XinvError, match='not for kind %r' % g['kind']):
        rp.solve_fourier()
    rp.close()
