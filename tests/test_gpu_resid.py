"""The residual R = L(S) - F on the GPU (k_resid2d / k_resid3d, xinvert_amd/csrc/xinv_resid.h): bit for bit
against the numpy restatement tests/resid_model.py, which tests/test_resid_host.py holds to the reference's own kernels.
Shapes are the smallest at which the kernels can go wrong: one interior row / column, the wavefront width, odd periodic
xc, two strips meeting, three planes."""
import ctypes
import os
import re

import numpy as np
import pytest

import resid_model as M
import xinvert_amd as xa
from xinvert_amd import _lib, apps, core, forms
from xinvert_amd.field import Field
from xinvert_amd.resident import ResidentProblem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDEF = -9.99e8
_hdr = open(os.path.join(ROOT, 'xinvert_amd', 'csrc', 'xinv_resid.h')).read()
ROWS = int(re.search(r'#define XINV_RESID_ROWS (\d+)', _hdr).group(1))          # rows a 2-D workgroup marches
PLANES = int(re.search(r'#define XINV_RESID_PLANES (\d+)', _hdr).group(1))      # planes a 3-D workgroup marches


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def problem(kind, shape, nb, seed, per, shared=True, null_B=False, zero_B=False, blobs=False, coef_undef=False,
            coef_nan=False):
    """-> dict(kind, S [nb, *shape], coefs (forcing last; shared ones core-shaped, B None when null_B), sc, per)."""
    rng = np.random.default_rng(seed)
    f = forms.FORMS[kind]
    three = f.rank == 3
    delx = float(rng.uniform(0.6, 1.4))
    sc = dict(delx=delx, delxSqr=delx * delx)
    if three:
        r2, r1 = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))
        sc.update(ratio2=r2, ratio1=r1, ratio2Sqr=r2 * r2, ratio1Sqr=r1 * r1)
    else:
        r = float(rng.uniform(0.5, 2.0))
        sc.update(ratio=r, ratioQtr=r / 4.0, ratioSqr=r * r)
    coefs = []
    for q, a in enumerate(f.arrays):
        shp = ((nb,) if (not shared or q == len(f.arrays) - 1) else ()) + tuple(shape)
        coefs.append(rng.uniform(0.5, 1.5, shp) if a in 'AC' else rng.standard_normal(shp))
    if f.null_B and null_B:
        coefs[1] = None
    elif f.null_B and zero_B:
        coefs[1] = np.zeros_like(coefs[1])
    F = coefs[-1]
    if blobs:                                                  # blobs of undef in the forcing
        F[..., 1:3, 1:3] = UNDEF
        F[0].reshape(-1)[rng.choice(F[0].size, max(1, F[0].size // 11), replace=False)] = UNDEF
    if coef_undef:
        c = coefs[0]
        c.reshape(-1)[rng.choice(c.size, max(1, c.size // 13), replace=False)] = UNDEF
        c2 = coefs[2]
        c2.reshape(-1)[rng.choice(c2.size, max(1, c2.size // 17), replace=False)] = UNDEF
    if coef_nan:                                               # one NaN coefficient at a live point of the last member
        centre = tuple(n // 2 for n in shape)
        (coefs[2][-1] if coefs[2].ndim > len(shape) else coefs[2])[centre] = np.nan
        F[-1][centre] = 0.5
    S = rng.standard_normal((nb,) + tuple(shape))
    S.reshape(-1)[rng.choice(S.size, 2, replace=False)] = 0.0   # (exact zeros: the sign of a zero result)
    return dict(kind=kind, S=S, coefs=coefs, sc=sc, per=per, shape=tuple(shape), nb=nb)


def model(p):
    Rs, ns = [], []
    for m in range(p['nb']):
        cs = [None if c is None else (c[m] if c.ndim == len(p['shape']) + 1 else c) for c in p['coefs']]
        R, live = M.residual(p['kind'], p['S'][m], cs, p['sc'], p['per'], UNDEF)
        Rs.append(R)
        ns.append(M.norms(R, cs[-1], live))
    return np.stack(Rs), np.stack(ns)


def scalars(p):
    f = forms.FORMS[p['kind']]
    d = dict(p['sc'], kind=p['kind'], optArg=1.7, undef=UNDEF, dely=1.0, delz=1.0, BCy='fixed', BCz='fixed',
             BCx='periodic' if p['per'] else 'fixed')
    d.update(zip(('zc', 'yc', 'xc')[-f.rank:], p['shape']))
    return forms.scalars(d)


def strides(p):
    n = int(np.prod(p['shape']))
    return [n, n] + [0 if (c is None or c.ndim == len(p['shape'])) else n for c in p['coefs']]


def run_dev(p, want_norms=True, stream=None):
    """The _dev entry on torch tensors -> (R, norms); checks that no input changed."""
    import torch
    L = _lib.require_gpu()
    dev = [torch.tensor(p['S'], dtype=torch.float64, device='cuda')] + \
          [None if c is None else torch.tensor(c, dtype=torch.float64, device='cuda') for c in p['coefs']]
    R = torch.full(p['S'].shape, 12345.0, dtype=torch.float64, device='cuda')
    norms = np.full((p['nb'], 4), -1.0)
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream()
    rc = getattr(L, forms.symbol(p['kind'], 'resid_dev'))(
        _lib.dptr(R), *[_lib.dptr(t) for t in dev], p['nb'], _lib.strides_arg(strides(p)), *scalars(p),
        _lib.hptr(norms) if want_norms else None, ctypes.c_void_p(st.cuda_stream))
    _lib.check(rc)
    st.synchronize()
    for t, h in zip(dev, [p['S']] + p['coefs']):
        assert t is None or bits_equal(t.cpu().numpy(), h)             # the inputs are bitwise unchanged
    return R.cpu().numpy(), norms


def run_host(p):
    L = _lib.require_gpu()
    R = np.full(p['S'].shape, 12345.0)
    norms = np.full((p['nb'], 4), -1.0)
    arrs = [R, p['S'].copy()] + [None if c is None else np.ascontiguousarray(c) for c in p['coefs']]
    rc = getattr(L, forms.symbol(p['kind'], 'resid_batched'))(
        *[_lib.hptr(a) for a in arrs], p['nb'], _lib.strides_arg(strides(p)), *scalars(p), _lib.hptr(norms),
        ctypes.byref(_lib.options()))
    _lib.check(rc)
    return R, norms


def check_norms(got, want):
    """n_live, max|R| and max|F| exactly; mean|R| within n_live * 2^-53 relative (non-negative terms in another order)."""
    for g, w in zip(got, want):
        assert g[0] == w[0]
        assert bits_equal(g[2], w[2]) and bits_equal(g[3], w[3])
        if np.isnan(w[1]):
            assert np.isnan(g[1])
        else:
            assert abs(g[1] - w[1]) <= w[0] * 2.0 ** -53 * abs(w[1]), (g, w)


SHAPES_2D = [(3, 3), (3, 64), (5, 63), (4, 65), (5, 129), (ROWS + 1, 7), (ROWS + 2, 66), (2 * ROWS + 1, 5), (7, 257)]
# (the 3-D kernels tile x on their own: one tile short of a lane, exactly one tile, one lane into the second and the third)
SHAPES_3D = [(3, 3, 3), (4, 5, 5), (3, 4, 63), (4, 5, 64), (3, 4, 65), (3, 4, 129), (5, 6, 67), (PLANES + 1, 5, 9),
             (PLANES + 2, 9, 4)]


@pytest.mark.parametrize('kind', ['std2d', 'gen2d', 'std2dt'])
def test_2d_bitwise_at_the_shapes_that_can_break_the_kernel(kind):
    seed = 0
    for shape in SHAPES_2D:
        for per in (False, True):
            seed += 1
            p = problem(kind, shape, 1, seed, per, blobs=min(shape) > 3)
            R, n = run_dev(p)
            Rm, nm = model(p)
            assert bits_equal(R, Rm), (kind, shape, per)
            check_norms(n, nm)
    # periodic x with odd xc
    for xc in (5, 65):
        p = problem(kind, (6, xc), 2, 100 + xc, True)
        R, n = run_dev(p)
        Rm, nm = model(p)
        assert bits_equal(R, Rm), (kind, xc)
        check_norms(n, nm)


@pytest.mark.parametrize('kind', ['std3d', 'gen3d'])
def test_3d_bitwise_at_the_shapes_that_can_break_the_kernel(kind):
    seed = 0
    for shape in SHAPES_3D:
        for per in (False, True):
            seed += 1
            p = problem(kind, shape, 1, seed, per, blobs=min(shape) > 3)
            R, n = run_dev(p)
            Rm, nm = model(p)
            assert bits_equal(R, Rm), (kind, shape, per)
            check_norms(n, nm)


@pytest.mark.parametrize('kind', list(forms.RESIDUAL))
def test_batches_masks_null_B_nan_and_streams(kind):
    import torch
    shape = (ROWS + 3, 70) if forms.FORMS[kind].rank == 2 else (4, 6, 67)
    variants = [dict(shared=True), dict(shared=False), dict(shared=True, blobs=True, coef_undef=True),
                dict(shared=False, coef_nan=True, blobs=True)]
    if forms.FORMS[kind].null_B:
        variants += [dict(null_B=True), dict(null_B=True, blobs=True, shared=False), dict(zero_B=True)]
    for k, v in enumerate(variants):
        for per in (False, True):
            p = problem(kind, shape, 3, 1000 + 10 * k + per, per, **v)
            R, n = run_dev(p)
            Rm, nm = model(p)
            assert bits_equal(R, Rm), (kind, v, per)
            check_norms(n, nm)
            if v.get('coef_nan'):
                assert np.isnan(Rm).any() and np.isnan(nm[:, 1]).any()
    # a non-default stream, with and without norms; two calls give identical bits
    p = problem(kind, shape, 3, 77, True, shared=False, blobs=True)
    Rm, nm = model(p)
    s = torch.cuda.Stream()
    R1, n1 = run_dev(p, stream=s)
    R2, n2 = run_dev(p, stream=s)
    R3, _ = run_dev(p, want_norms=False, stream=s)
    assert bits_equal(R1, Rm) and bits_equal(R2, Rm) and bits_equal(R3, Rm)
    assert np.array_equal(n1.view(np.int64), n2.view(np.int64))
    check_norms(n1, nm)


@pytest.mark.parametrize('kind', list(forms.RESIDUAL))
def test_host_pointer_entry_equals_the_device_entry(kind):
    shape = (ROWS + 1, 65) if forms.FORMS[kind].rank == 2 else (3, 5, 66)
    for v in (dict(shared=True, blobs=True), dict(shared=False, coef_undef=True)):
        p = problem(kind, shape, 3, 5, True, **v)
        Rd, nd = run_dev(p)
        Rh, nh = run_host(p)
        assert bits_equal(Rh, Rd) and np.array_equal(nh.view(np.int64), nd.view(np.int64))


def test_argument_errors():
    import torch
    L = _lib.require_gpu()
    p = problem('std2d', (5, 8), 2, 3, False)
    dev = [torch.tensor(p['S'], device='cuda')] + [torch.tensor(c, device='cuda') for c in p['coefs']]
    R = torch.empty_like(dev[0])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = getattr(L, forms.symbol('std2d', 'resid_dev'))
    ptrs = [_lib.dptr(t) for t in dev]

    def call(Rp=None, ps=None, strd=None, sc=None):
        return fn(Rp if Rp is not None else _lib.dptr(R), *(ps or ptrs), 2, _lib.strides_arg(strd or strides(p)),
                  *(sc or scalars(p)), None, st)
    assert call() == 0
    assert call(Rp=ptrs[0]) == -1 and b'overlaps' in L.xinv_last_error()            # R aliases S
    assert call(Rp=ptrs[4]) == -1                                                     # R aliases the forcing
    assert call(ps=[ptrs[0], None] + ptrs[2:]) == -1                                  # a null array that is not B
    bad = scalars(p); bad[0] = 2                                                      # yc < 3, as the solve entries refuse
    assert call(sc=bad) == -1
    bad = scalars(p); bad[5] = 7                                                      # an unknown BC code
    assert call(sc=bad) == -1
    assert call(strd=[3] + strides(p)[1:]) == -1                                      # R stride shorter than a slice
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- front end
def _front_state(coef_func, F, dims, coords, mParams, iParams, S_vals):
    """What apps.residual rebuilds, from the front end's own coefficient builders -> (coeffs, maskF, state, iParams)."""
    iP = apps._update(apps.default_iParams, iParams)
    maskF, initS, coeffs = coef_func(F, dims, coords, mParams, iP, None)
    if len(dims) == 2:
        ps = apps._cal_params2D(maskF[dims[0]], maskF[dims[1]], coords, Rearth=mParams['Rearth'])
    else:
        ps = apps._cal_params3D(maskF[dims[0]], maskF[dims[1]], maskF[dims[2]], coords, Rearth=mParams['Rearth'])
    iP = apps._update(ps, iP)
    return coeffs, maskF, maskF.like(apps._solver_state(S_vals, maskF.values, initS.values)), iP


def _front_model(coef_func, F, dims, coords, mParams, iParams, S_vals, kind):
    """The model on that state -> (R de-masked, R with the solver's undef, norms)."""
    coeffs, maskF, state, iP = _front_state(coef_func, F, dims, coords, mParams, iParams, S_vals)
    sc = {s: float(iP[forms.IPARAM.get(s, s)]) for s in forms.FORMS[kind].scalars
          if not s.startswith('BC') and s not in ('undef', 'optArg', 'xc', 'yc', 'zc')}
    cs = []
    for k, c in enumerate(coeffs):
        v = np.broadcast_to(np.asarray(c.values if hasattr(c, 'values') else c, dtype=np.float64), maskF.shape)
        null = k == 1 and forms.FORMS[kind].null_B and all(s == 0 for s in v.strides) and v.flat[0] == 0.0
        cs.append(None if null else np.array(v))
    cs.append(np.asarray(maskF.values, dtype=np.float64))
    R, live = M.residual(kind, state.values, cs, sc, iP['BCs'][-1] == 'periodic', UNDEF)
    return np.where(R != UNDEF, R, iP['undef']), R, M.norms(R, cs[-1], live)


def _resident_residual(inv_name, coef_func, F, dims, coords, mParams, iParams, S_vals):
    """ResidentProblem.residual() on the same state, uploaded as the front end uploads a resident batch (core.Resident:
    coefficients that depend on latitude alone travel as one value per row) -> (R with the solver's undef, norms)."""
    coeffs, maskF, state, iP = _front_state(coef_func, F, dims, coords, mParams, iParams, S_vals)
    res = core.Resident(inv_name, coeffs, maskF, state, dims, iP)
    try:
        R, n = res.rp.residual()
        assert bits_equal(res.rp.result(), state.values[None])         # residual() leaves S alone
        return R.cpu().numpy()[0], n, res.rp.rowconst
    finally:
        res.rp.close()


def test_front_end_poisson_masked_latlon():
    rng = np.random.default_rng(11)
    lat, lon = np.linspace(-57.5, 57.5, 24), np.arange(36) * 10.0
    v = rng.standard_normal((24, 36)) * 1e-9
    v[8:12, 5:9] = np.nan; v[15, 20] = np.nan
    F = Field(v, ('lat', 'lon'), {'lat': lat, 'lon': lon})
    dims = ['lat', 'lon']
    base = {'BCs': ['fixed', 'periodic'], 'tolerance': 1e-14, 'printInfo': False}
    mP = apps._update(apps.default_mParams, {}, None)
    maxR = []
    for mx in (5, 60):
        ip = dict(base, mxLoop=mx, residual=True)
        sf = xa.invert_Poisson(F, dims, iParams=ip)
        opt_in = np.array(sf.iParams['resid'], copy=True)
        ip2 = dict(base, mxLoop=mx)
        R = apps.residual('Poisson', sf, F, dims, iParams=ip2)
        Rm, Ru, nm = _front_model(apps._coeffs_Poisson, F, dims, 'lat-lon', mP, ip2, sf.values, 'std2d')
        assert bits_equal(R.values, Rm)
        assert np.isnan(R.values[0]).all() and np.isnan(R.values[9, 6]) and not np.isnan(R.values[3, 0])
        check_norms(ip2['resid'], [nm])
        assert np.array_equal(opt_in.view(np.int64), np.asarray(ip2['resid']).view(np.int64))    # opt-in == separate call
        # ResidentProblem.residual() on the same state agrees with both, R and norms bit for bit
        Rr, nr, rowconst = _resident_residual('inv_standard2D', apps._coeffs_Poisson, F, dims, 'lat-lon', mP, ip2, sf.values)
        assert rowconst                                        # (A and C depend on latitude alone: the expansion ran)
        assert bits_equal(Rr, Ru) and np.array_equal(nr.view(np.int64), opt_in.reshape(-1, 4).view(np.int64))
        # without the key nothing changes: the same solution, and no 'resid'
        plain = xa.invert_Poisson(F, dims, iParams=dict(base, mxLoop=mx))
        assert bits_equal(plain.values, sf.values) and 'resid' not in plain.iParams
        maxR.append(ip2['resid'][0][2])
    assert maxR[1] < maxR[0]                                   # more sweeps: a smaller max|R| (ordering only)


def test_front_end_omega_and_resident_problem():
    rng = np.random.default_rng(12)
    lev, lat, lon = np.linspace(1e5, 1e4, 6), np.linspace(-45.0, 45.0, 10), np.arange(12) * 30.0
    v = 1e-17 * rng.standard_normal((6, 10, 12))
    v[1:3, 4:6, 3:5] = np.nan
    F = Field(v, ('lev', 'lat', 'lon'), {'lev': lev, 'lat': lat, 'lon': lon})
    dims = ['lev', 'lat', 'lon']
    base = {'BCs': ['fixed', 'fixed', 'periodic'], 'tolerance': 1e-14, 'printInfo': False}
    mPu = {'N2': 2e-5}
    mP = apps._update(apps.default_mParams, mPu, None)
    maxR = []
    for mx in (3, 40):
        ip = dict(base, mxLoop=mx, residual=True)
        w = xa.invert_omega(F, dims, mParams=mPu, iParams=ip)
        opt_in = np.array(w.iParams['resid'], copy=True)
        ip2 = dict(base, mxLoop=mx)
        R = apps.residual('omega', w, F, dims, mParams=mPu, iParams=ip2)
        Rm, Ru, nm = _front_model(apps._coeffs_omega, F, dims, 'lat-lon', mP, ip2, w.values, 'std3d')
        assert bits_equal(R.values, Rm)
        check_norms(ip2['resid'], [nm])
        assert np.array_equal(opt_in.view(np.int64), np.asarray(ip2['resid']).view(np.int64))
        Rr, nr, rowconst = _resident_residual('inv_standard3D', apps._coeffs_omega, F, dims, 'lat-lon', mP, ip2, w.values)
        assert rowconst
        assert bits_equal(Rr, Ru) and np.array_equal(nr.view(np.int64), opt_in.reshape(-1, 4).view(np.int64))
        maxR.append(ip2['resid'][0][2])
    assert maxR[1] < maxR[0]

    # the resident batch: residual() of its state agrees with the device entry and the model, before and after a solve
    p = problem('std2d', (ROWS + 4, 40), 2, 21, True, shared=True, null_B=True, blobs=True)
    p['coefs'][0] = np.broadcast_to(np.linspace(0.8, 1.2, ROWS + 4)[:, None], p['shape'])    # one value per row
    q = dict(forms.from_iparams('std2d', dict(gc2=p['shape'][0], gc1=p['shape'][1], del2=1.0, del1=p['sc']['delx'],
                                              del1Sqr=p['sc']['delxSqr'], ratioQtr=p['sc']['ratioQtr'],
                                              ratioSqr=p['sc']['ratioSqr'], optArg=1.2, BCs=['fixed', 'periodic']), UNDEF),
             S0=p['S'], coefs=[np.zeros(p['shape']) if c is None else c for c in p['coefs']], shared=(0, 1, 2))
    rp = ResidentProblem(q)
    for sweeps in (0, 4):
        if sweeps:
            rp.solve(sweeps - 1, 0.0)
        R, n = rp.residual()
        p['S'] = rp.result()
        Rm, nm = model(p)
        assert bits_equal(R.cpu().numpy(), Rm)
        check_norms(n, nm)
        Rd, nd = run_dev(p)
        assert bits_equal(Rd, Rm) and np.array_equal(nd.view(np.int64), n.view(np.int64))
        assert bits_equal(rp.result(), p['S'])                 # residual() leaves S alone
    rp.close()
