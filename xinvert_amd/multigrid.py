"""invert_MultiGrid: coarse-to-fine SOR solves (nested iteration) for the 2-D and 3-D `invert_*` apps.

The reference's `invert_MultiGrid` (apps.py:1061-1135) cannot run (it imports a module that does not exist and passes
arguments the apps no longer take).  This version keeps its name, argument shape and return tuple with semantics of
its own:

  * levels use the ratios ratio**(gridNo-1), ..., ratio, 1; per core dim a level is coarsened only when the coarse
    length n // r is at least 3 and, on a 'periodic' dim, r divides n -- otherwise that dim keeps ratio 1 there.  A
    coarse level that coarsens no dim at all would repeat the finest solve and is left out;
  * a coarse grid keeps n // r blocks of r consecutive fine points from index 0 (the trailing n % r points belong to no
    block); its coordinates are the block means; the app's own coefficient builder and _cal_params2D/3D run on it;
  * the caller's raw forcing goes to the device once and every coarse forcing is restricted from it there
    (k_mg_restrict: the block mean over the defined points); labelled mParams arrays over core dims and a labelled icbc
    are restricted on the host in the same way (the finest level uses the caller's icbc as it is);
  * every level runs with the caller's tolerance and mxLoop as a device-resident batch (core.Resident), and
    k_mg_prolong writes the d-linear interpolation of its solver state straight into the next level's resident S,
    except where the ordinary solve keeps its starting value (undefined forcing, the edges of non-periodic dims);
  * a single level (gridNo = 1, ratio = 1, or a grid too small to coarsen) is exactly the app's own call.
"""
import inspect

import numpy as np

from . import _lib, apps, core
from .apps import _undeftmp, default_iParams, default_mParams
from .field import Field, from_any, to_like, undef_as

# app -> (coefficient builder, core function name, valid mParams, checks N2)   (the apps' own _template arguments)
_APPS = {
    apps.invert_Poisson: (apps._coeffs_Poisson, 'inv_standard2D', ['g', 'Omega', 'Rearth'], False),
    apps.invert_Stommel: (apps._coeffs_Stommel, 'inv_general2D',
                          ['beta', 'R', 'D', 'rho0', 'g', 'Omega', 'Rearth'], False),
    apps.invert_StommelMunk: (apps._coeffs_StommelMunk, 'inv_general2D_bih',
                              ['A4', 'beta', 'R', 'D', 'rho0', 'g', 'Omega', 'Rearth'], False),
    apps.invert_Fofonoff: (apps._coeffs_Fofonoff, 'inv_standard2D_test',
                           ['c0', 'c1', 'f0', 'beta', 'g', 'Omega', 'Rearth'], False),
    apps.invert_BrethertonHaidvogel: (apps._coeffs_Bretherton, 'inv_standard2D_test',
                                      ['f0', 'beta', 'D', 'lambda', 'g', 'Omega', 'Rearth'], False),
    apps.invert_GillMatsuno: (apps._coeffs_GillMatsuno, 'inv_general2D',
                              ['f0', 'beta', 'epsilon', 'Phi', 'g', 'Omega', 'Rearth'], False),
    apps.invert_RefState: (apps._coeffs_RefState, 'inv_standard2D', ['Ang0', 'Gamma', 'g', 'Omega', 'Rearth'], False),
    apps.invert_PV2D: (apps._coeffs_PV2D, 'inv_standard2D', ['f0', 'beta', 'N2', 'g', 'Omega', 'Rearth'], False),
    apps.invert_Eliassen: (apps._coeffs_Eliassen, 'inv_standard2D', ['A', 'B', 'C', 'g', 'Omega', 'Rearth'], False),
    apps.invert_GillMatsuno_test: (apps._coeffs_GillMatsuno_test, 'inv_standard2D_test',
                                   ['f0', 'beta', 'epsilon', 'Phi', 'g', 'Omega', 'Rearth'], False),
    apps.invert_Stommel_test: (apps._coeffs_Stommel_test, 'inv_standard2D_test',
                               ['beta', 'R', 'D', 'rho0', 'g', 'Omega', 'Rearth'], False),
    apps.invert_StommelArons: (apps._coeffs_StommelArons, 'inv_general2D',
                               ['f0', 'beta', 'epsilon', 'g', 'Omega', 'Rearth'], False),
    apps.invert_geostrophic: (apps._coeffs_geostrophic, 'inv_standard2D',
                              ['f0', 'beta', 'Omega', 'g', 'Omega', 'Rearth'], False),
    apps.invert_omega: (apps._coeffs_omega, 'inv_standard3D', ['f0', 'beta', 'N2', 'g', 'Omega', 'Rearth'], True),
    apps.invert_3DOcean: (apps._coeffs_3DOcean, 'inv_general3D',
                          ['f0', 'beta', 'epsilon', 'N2', 'k', 'g', 'Omega', 'Rearth'], True),
}
_ONE_D = (apps.invert_GeoAdjustment, apps.invert_RefStateSWM)


# ------------------------------------------------------------------------------ grid hierarchy (host)
def level_ratios(lengths, BCs, ratio=3, gridNo=3):
    """Per-dim ratios of every level, coarsest first, the finest (all 1) last.  lengths / BCs: the core dims'."""
    ratio, gridNo = _positive_int(ratio, 'ratio'), _positive_int(gridNo, 'gridNo')
    levels = []
    for k in range(gridNo - 1, 0, -1):
        r = ratio ** k
        rs = tuple(r if n // r >= 3 and (BC != 'periodic' or n % r == 0) else 1 for n, BC in zip(lengths, BCs))
        if any(x > 1 for x in rs):
            levels.append(rs)
    levels.append((1,) * len(lengths))
    return levels


def _positive_int(v, name):
    if isinstance(v, bool) or int(v) != v or v < 1:
        raise Exception('%s must be an integer >= 1, got %r' % (name, v))
    return int(v)


def coarse_coord(c, r):
    """Block means of r consecutive coordinates from index 0 (the trailing len(c) % r are dropped)."""
    c = np.asarray(c, dtype=np.float64)
    if r == 1:
        return c
    m = len(c) // r
    return c[:m * r].reshape(m, r).mean(axis=1)


def prolong_table(xf, xc, periodic):
    """(lo, hi, w) per fine index: the fine coordinate xf[i] between the coarse coordinates xc[lo], xc[hi], weight w of
    xc[hi].  Clamped to the end values outside the coarse range; on a periodic dim wrapped across the seam with the
    period len(xf) * (xf[1] - xf[0]).  Equal grids (a dim neither level coarsens): the identity (lo = hi = i, w = 0)."""
    xf = np.asarray(xf, dtype=np.float64)
    xc = np.asarray(xc, dtype=np.float64)
    n, m = len(xf), len(xc)
    if n == m and np.array_equal(xf, xc):
        i = np.arange(n, dtype=np.int64)
        return i, i.copy(), np.zeros(n)
    if periodic:                                         # (positions taken modulo the period, as numpy.interp does)
        P = n * (xf[1] - xf[0])
        u = np.mod(xf, P)
        U = np.mod(xc, P)
        order = np.argsort(U, kind='stable')
        ext = np.concatenate(([order[-1]], order, [order[0]]))
        Ue = np.concatenate(([U[order[-1]] - P], U[order], [U[order[0]] + P]))
        j = np.clip(np.searchsorted(Ue, u, side='right') - 1, 0, m)
        w = (u - Ue[j]) / (Ue[j + 1] - Ue[j])
        return ext[j].astype(np.int64), ext[j + 1].astype(np.int64), w
    if xc[-1] < xc[0]:                                   # descending coordinates (lat from 90 to -90): the same
        return prolong_table(-xf, -xc, False)            # brackets and weights on the negated (exact) axis
    j = np.clip(np.searchsorted(xc, xf, side='right') - 1, 0, m - 2)
    lo, hi = j.astype(np.int64), (j + 1).astype(np.int64)
    w = (xf - xc[j]) / (xc[j + 1] - xc[j])
    below, above = xf <= xc[0], xf >= xc[-1]
    lo[below], hi[below], w[below] = 0, 0, 0.0
    lo[above], hi[above], w[above] = m - 1, m - 1, 0.0
    return lo, hi, w


def restrict_array(v, axes, undef=np.nan):
    """Host restriction (the arithmetic of k_mg_restrict): `axes` = [(axis, ratio)], block means over the points that
    are not `undef` (NaN: the NaN points), summed from 0.0 in lexicographic offset order; `undef` for an empty block."""
    v = np.asarray(v, dtype=np.float64)
    axes = sorted((int(a), int(r)) for a, r in axes if r > 1)
    m = {a: v.shape[a] // r for a, r in axes}
    acc = np.zeros(tuple(m.get(a, n) for a, n in enumerate(v.shape)))
    cnt = np.zeros_like(acc)
    for offs in np.ndindex(*[r for _, r in axes]):
        sl = [slice(None)] * v.ndim
        for (a, r), o in zip(axes, offs):
            sl[a] = slice(o, o + m[a] * r, r)
        x = v[tuple(sl)]
        ok = ~np.isnan(x) if np.isnan(undef) else x != undef
        acc = acc + np.where(ok, x, 0.0)
        cnt = cnt + ok
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(cnt > 0, acc / cnt, undef)


def restrict_field(g, rmap, undef=np.nan):
    """A labelled array (Field / DataArray) restricted along the dims named in rmap {dim: ratio}, coordinates included."""
    g = from_any(g)
    axes = [(g.axis(d), rmap[d]) for d in g.dims if rmap.get(d, 1) > 1]
    coords = {d: (coarse_coord(g[d], rmap[d]) if rmap.get(d, 1) > 1 else g[d]) for d in g.dims}
    return Field(restrict_array(g.values, axes, undef), g.dims, coords, name=g.name)


def _restrict_param(p, rmap, dims, core_shape):
    """An mParams entry on a coarse level: labelled arrays restricted along the core dims they share with the forcing, a
    bare array of the core shape along the core dims; scalars and everything else pass through."""
    if np.isscalar(p) or p is None:
        return p
    if hasattr(p, 'dims') and hasattr(p, 'values'):
        return restrict_field(p, rmap) if any(rmap.get(d, 1) > 1 for d in p.dims) else p
    v = np.asarray(p)
    if v.shape == tuple(core_shape):                            # a bare core-shaped array, dims in the order of `dims`
        return restrict_array(v, [(a, rmap[d]) for a, d in enumerate(dims)])
    return p


# ------------------------------------------------------------------------------ device transfers
def restrict_dev(fine, ratios, undef):
    """k_mg_restrict on a torch tensor [nbatch, *core] (float64, contiguous) -> the coarse tensor."""
    import torch
    assert fine.dtype == torch.float64 and fine.is_contiguous() and fine.is_cuda
    nd = fine.dim() - 1
    fshape = [int(x) for x in fine.shape[1:]]
    ratios = [int(r) for r in ratios]
    if len(ratios) != nd or not all(1 <= r <= n for r, n in zip(ratios, fshape)):
        raise Exception('ratios %r do not fit the core shape %r' % (ratios, fshape))
    out = torch.empty((fine.shape[0],) + tuple(n // r for n, r in zip(fshape, ratios)), dtype=torch.float64,
                      device=fine.device)
    L = _lib.require_gpu()
    with torch.cuda.device(fine.device):
        _lib.check(L.xinv_mg_restrict_f64_dev(_lib.dptr(fine), _lib.dptr(out),
                                              int(fine.shape[0]), nd, _lib.strides_arg(fshape),
                                              _lib.strides_arg(ratios), float(undef), _lib.stream_arg(fine)))
    return out


def prolong_dev(coarse, fine, tables, keep_edges=0, force=None, undef=_undeftmp):
    """k_mg_prolong: the d-linear blend of `coarse` [nbatch, *ccore] written into `fine` [nbatch, *fcore] in place,
    `tables` = [(lo, hi, w)] per core dim (prolong_table).  Points where `force` == undef, the edges of the dims whose
    bit is set in keep_edges, and points whose blend is not finite keep their value."""
    import torch
    nd = fine.dim() - 1
    fshape = [int(x) for x in fine.shape[1:]]
    cshape = [int(x) for x in coarse.shape[1:]]
    for t in (coarse, fine) + ((force,) if force is not None else ()):
        assert t.dtype == torch.float64 and t.is_contiguous() and t.device == fine.device
    if coarse.shape[0] != fine.shape[0] or len(cshape) != nd or len(tables) != nd or \
            (force is not None and tuple(force.shape) != tuple(fine.shape)):
        raise Exception('prolongation: coarse %r / fine %r / forcing shapes do not match'
                        % (tuple(coarse.shape), tuple(fine.shape)))
    idx, ws = [], []
    for (lo, hi, w), n, m in zip(tables, fshape, cshape):
        lo, hi, w = (np.asarray(x) for x in (lo, hi, w))
        if lo.shape != (n,) or hi.shape != (n,) or w.shape != (n,) or \
                lo.min() < 0 or hi.min() < 0 or lo.max() >= m or hi.max() >= m:
            raise Exception('prolongation table out of range')     # (the device reads them unchecked)
        idx += [lo.astype(np.int64), hi.astype(np.int64)]
        ws.append(w.astype(np.float64))
    idx_t = torch.from_numpy(np.concatenate(idx)).to(fine.device)
    w_t = torch.from_numpy(np.concatenate(ws)).to(fine.device)
    L, ptr = _lib.require_gpu(), _lib.dptr
    with torch.cuda.device(fine.device):
        _lib.check(L.xinv_mg_prolong_f64_dev(
            ptr(coarse), ptr(fine), ptr(force), int(fine.shape[0]), nd, _lib.strides_arg(cshape),
            _lib.strides_arg(fshape), ptr(idx_t), ptr(w_t), int(keep_edges), float(undef), _lib.stream_arg(fine)))
    # (the tables' blocks go back to torch's allocator on return: it reuses them in the order of this stream)
    return fine


# ------------------------------------------------------------------------------ public entry
def invert_MultiGrid(invert_func, F, dims, coords=None, icbc=None, mParams=default_mParams,
                     iParams=default_iParams, ratio=3, gridNo=3):
    """Solve `invert_func`'s problem on a hierarchy of grids, coarsest first, every finer grid starting from the
    interpolated solution of the coarser one (reference apps.py:1061-1135; semantics: module docstring).

    invert_func: one of this package's 2-D / 3-D `invert_*` apps; F, dims, coords (None: the app's default), icbc,
    mParams, iParams: that app's own arguments.  Returns (S, fs, os_): the finest result de-masked as the app de-masks
    it, the forcing of every level and the result of every level (coarsest first).  iParams['flags'] gets the finest
    level's flags and iParams['mg_flags'] those of every level."""
    if invert_func in _ONE_D:
        raise Exception('invert_MultiGrid needs a 2-D or 3-D app; %s is a 1-D app' % invert_func.__name__)
    if invert_func not in _APPS:
        raise Exception('invert_MultiGrid: %r is not one of the 2-D / 3-D invert_* apps of xinvert_amd'
                        % (invert_func,))
    coef_func, inv_name, validParams, checks_N2 = _APPS[invert_func]
    if coords is None:
        coords = inspect.signature(invert_func).parameters['coords'].default
    dimLen = 3 if inv_name.endswith('3D') else 2
    if len(dims) != dimLen:
        raise Exception('{0:2d} dimensional forcing are needed'.format(dimLen))
    ip_user = _update_iParams(iParams)
    devs = ip_user.get('devices')
    if devs is not None and (isinstance(devs, str) or len(list(devs)) > 1):
        raise NotImplementedError("invert_MultiGrid runs on one device: name it with iParams['device']")
    tmpl = F
    F = from_any(F)
    lengths = {d: F.shape[F.axis(d)] for d in dims}
    levels = level_ratios([lengths[d] for d in dims], list(ip_user['BCs']), ratio, gridNo)
    keep = isinstance(iParams, dict) and iParams is not default_iParams

    if len(levels) == 1:                                     # one level: the app's own call
        S = invert_func(tmpl, dims, coords, icbc, mParams, iParams)
        fl = getattr(S, 'iParams', {}).get('flags')
        if keep and fl is not None:
            iParams['flags'] = fl
            iParams['mg_flags'] = [fl]
        return S, [tmpl], [S]

    if checks_N2:
        apps._check_N2(mParams)
    mP = apps._update(default_mParams, mParams, list(validParams))
    if icbc is not None:
        icbc = from_any(icbc)
    import torch
    dev = ip_user.get('device')
    if dev is None and devs is not None:
        dev = list(devs)[0]
    dev = torch.cuda.current_device() if dev is None or int(dev) < 0 else int(dev)
    _lib.require_gpu()

    # 1. every coarse forcing restricted on the device from the raw fine forcing (uploaded once)
    perm, bdims, bshape = core._batch_layout(F, dims)
    nb = int(np.prod(bshape)) if bshape else 1
    core_shape = tuple(lengths[d] for d in dims)
    raw = np.asarray(F.values)
    undef_raw = undef_as(raw.dtype, ip_user['undef'])
    inv = np.argsort(perm)
    fine = torch.from_numpy(np.ascontiguousarray(np.transpose(raw.astype(np.float64, copy=False), perm)
                                                 ).reshape((nb,) + core_shape)).to(torch.device('cuda', dev))
    fs = []
    for rs in levels[:-1]:
        c = restrict_dev(fine, rs, undef_raw).cpu().numpy()
        c = np.transpose(c.reshape(tuple(bshape) + c.shape[1:]), inv)
        if raw.dtype == np.float32:                          # (undefined blocks hold the raw dtype's undef)
            c = c.astype(np.float32)
        crd = dict(F.coords)
        for d, r in zip(dims, rs):
            crd[d] = coarse_coord(F[d], r)
        fs.append(Field(np.ascontiguousarray(c), F.dims, crd, name=F.name))
    del fine
    fs.append(F)

    # 2. coarsest to finest: the app's builder on each grid, a resident solve, the prolongation into the next
    mg_flags, os_, prev = [], [], None
    for lev, (rs, Fl) in enumerate(zip(levels, fs)):
        finest = lev == len(levels) - 1
        rmap = dict(zip(dims, rs))
        mPl = mP if finest else {k: _restrict_param(v, rmap, dims, core_shape) for k, v in mP.items()}
        icl = icbc if (finest or icbc is None) else restrict_field(icbc, rmap)
        ipl = _update_iParams(iParams)
        ipl['device'] = dev
        maskF, initS, coeffs = coef_func(Fl, dims, coords, mPl, ipl, icl)
        if dimLen == 2:
            ps = apps._cal_params2D(maskF[dims[0]], maskF[dims[1]], coords, Rearth=mPl['Rearth'])
        else:
            ps = apps._cal_params3D(maskF[dims[0]], maskF[dims[1]], maskF[dims[2]], coords, Rearth=mPl['Rearth'])
        ipl = apps._update(ps, ipl)
        if ipl['debug']:
            print({k: v for k, v in ipl.items() if k != 'flags'})
        with torch.cuda.device(dev):
            res = core.Resident(inv_name, coeffs, maskF, initS, dims, ipl)
            if prev is not None:
                pres, pmask = prev
                tables = [prolong_table(maskF[d], pmask[d], BC == 'periodic') for d, BC in zip(dims, ipl['BCs'])]
                keep_edges = sum(1 << k for k, BC in enumerate(ipl['BCs']) if BC != 'periodic')
                prolong_dev(pres.rp.S, res.rp.S, tables, keep_edges, res.rp.coefs[-1], _undeftmp)
                for m in np.flatnonzero(np.reshape(mg_flags[-1], (-1, 3))[:, 0]):
                    res.rp.S[m].copy_(res.rp.S0[m])          # (a member whose coarse solve overflowed seeds nothing)
                pres.rp.close()
            fl = res.solve(int(ipl['mxLoop']), float(ipl['tolerance']))
            mg_flags.append(np.array(fl if res.rp.nb > 1 else fl[0], copy=True))
            Sv = res.values()
        if icbc is None:
            Sv = np.where(maskF.values != _undeftmp, Sv, ipl['undef'])
        S = maskF.like(Sv, 'inverted')
        S.iParams = ipl
        os_.append(S)
        if ipl.get('printInfo', True):
            print('MultiGrid level {0} ratios {1}: loops {2:4.0f} and tolerance is {3:e}'.format(
                lev, rs, np.max(mg_flags[-1][..., 2]), np.max(mg_flags[-1][..., 1])))
        prev = (res, maskF)
    res.rp.close()

    ipl['flags'] = mg_flags[-1]
    ipl['mg_flags'] = mg_flags
    if keep:
        iParams['flags'] = mg_flags[-1]
        iParams['mg_flags'] = mg_flags
    if not isinstance(tmpl, Field):
        fs = [to_like(f, tmpl) for f in fs[:-1]] + [tmpl]
        os_ = [to_like(o, tmpl) for o in os_]
    return os_[-1], fs, os_


def _update_iParams(iParams):
    return apps._update(default_iParams, iParams)
