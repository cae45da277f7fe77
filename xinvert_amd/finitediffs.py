"""Finite-difference operators of the reference (xinvert/finitediffs.py): FiniteDiff, deriv, deriv2, padBCs.

Every operator that differentiates is ONE launch of the HIP kernel k_fd (csrc/xinv_fd.h) through the C-ABI entries
xinv_fd_f64 (host arrays) / xinv_fd_f64_dev (device arrays): each input is read from HBM once, each output written
once, the boundary padding is evaluated in registers.  This module only builds the per-index tables (numpy.gradient's
weights on the padded coordinate, metric factors, cos / tan of latitude) with numpy, the way the reference's lines
compute them, so the device result equals the numpy restatement (tests/fd_model.py) bit for bit in float64.
`padBCs` is host-only numpy.

Inputs are `Field`, xarray.DataArray (converted at the boundary) or an ndarray with `dims=`; results come back in the
caller's container type.  `DeviceField` wraps a torch tensor already on the GPU: the same methods then run on the
device-resident data, on the current torch stream, without a host round trip.

Decided deviations from the reference:
  * grad and divg pass fill[dim] to deriv (the reference passes the whole fill dict, finitediffs.py:197 / :275), as
    vort and Laplacian do;
  * shear_strain, deformation_rate and Okubo_Weiss raise NotImplementedError (they raise TypeError in the reference);
  * float32 data and coordinates are widened to float64; results are float64;
  * coordinates must be numeric (datetime axes raise TypeError);
  * every input of one call must have the same dims in the same order (the reference aligns by name);
  * the derivative axis needs at least 2 points;
  * FiniteDiff does not modify the BCs / fill dicts it is given (the reference fills them in place).
"""
import ctypes

import numpy as np

from . import _lib
from .apps import gradient_tables, padded_coord
from .field import Field, from_any, to_like

_BC_CODES = {'fixed': 0, 'extend': 1, 'periodic': 2, 'reflect': 3}
_KINDS = {'center': 0, 'forward': 1, 'backward': 2}
_SECOND = 3
_EACH, _SUM, _DIFF = 0, 1, 2
_ITERM, _DTERM = 15, 6


# ------------------------------------------------------------------ device-resident fields
class DeviceField:
    """A float64 torch tensor on the GPU with ordered dims and 1-D host coordinates (numpy): FiniteDiff's methods,
    deriv and deriv2 take these and return these, computing on the device on the current torch stream."""

    def __init__(self, tensor, dims, coords=None, name=None):
        import torch
        if not tensor.is_cuda:
            raise ValueError('DeviceField needs a tensor on the GPU')
        if tensor.dtype != torch.float64:
            tensor = tensor.double()                   # (float32 is widened, as on the host)
        self.values = tensor.contiguous()
        self.dims = tuple(dims)
        if self.values.dim() != len(self.dims):
            raise ValueError('tensor.dim() %d != len(dims) %d' % (self.values.dim(), len(self.dims)))
        coords = {} if coords is None else dict(coords)
        self.coords = {}
        for ax, d in enumerate(self.dims):
            c = coords.get(d)
            c = np.arange(self.values.shape[ax], dtype=np.float64) if c is None else np.asarray(c)
            if c.ndim != 1 or c.shape[0] != self.values.shape[ax]:
                raise ValueError('coordinate %r does not match axis length' % d)
            self.coords[d] = c
        self.name = name

    @property
    def shape(self):
        return tuple(self.values.shape)

    def axis(self, dim):
        return self.dims.index(dim)

    def __getitem__(self, dim):
        return self.coords[dim]

    def __repr__(self):
        return 'DeviceField(name=%r, dims=%r, shape=%r)' % (self.name, self.dims, self.shape)


def _field(v, dims=None):
    if isinstance(v, DeviceField):
        return v
    f = from_any(v, dims)
    vals = np.asarray(f.values)
    if vals.dtype.kind not in 'fiub':
        raise TypeError('finite differences need numeric data, got dtype %s' % vals.dtype)
    return f


def _out(values, f, tmpl, name=None):
    """`values` in the container type of the caller's `tmpl` (f: its Field / DeviceField)."""
    if isinstance(f, DeviceField):
        return DeviceField(values, f.dims, f.coords, name)
    res = Field(values, f.dims, f.coords, name)
    if isinstance(tmpl, np.ndarray):
        return values
    return to_like(res, tmpl)


def _coord(f, dim):
    c = np.asarray(f.coords[dim])
    if c.dtype.kind in 'mM':
        raise TypeError('coordinate %r is a datetime axis: finite differences need a numeric coordinate' % dim)
    if c.dtype.kind not in 'fiu':
        raise TypeError('coordinate %r must be numeric, got dtype %s' % (dim, c.dtype))
    return np.asarray(c, dtype=np.float64)


def _BC_pair(BCs):
    """(low, high) BCs as padBCs checks them (reference finitediffs.py:577-593)."""
    if isinstance(BCs, str):
        BCs = (BCs, BCs)
    BCs = tuple(BCs)
    if 'periodic' in BCs:
        if BCs[0] != BCs[1]:
            raise Exception('\'periodic\' cannot be mixed with other BCs')
    else:
        for B in BCs:
            if B not in ('fixed', 'extend', 'reflect'):
                raise Exception('unsupported BC: ' + str(BCs))
    return BCs


def _fill_pair(fill):
    if np.ndim(fill) == 0:
        return float(fill), float(fill)
    fill = tuple(fill)
    return float(fill[0]), float(fill[-1])


def _vector(scale, f):
    """A divisor: python scalar -> (scalar, None); 1-D labelled array along a dim of f -> (values, dim)."""
    if isinstance(scale, tuple) and len(scale) == 2 and isinstance(scale[1], str):
        return np.asarray(scale[0], dtype=np.float64), scale[1]
    if np.ndim(scale) == 0 and not hasattr(scale, 'dims'):
        return scale, None
    if hasattr(scale, 'dims') and len(scale.dims) == 1 and scale.dims[0] in f.dims:
        return np.asarray(scale.values, dtype=np.float64), scale.dims[0]
    if hasattr(scale, 'dims') and len(scale.dims) == 0:
        return float(np.asarray(scale.values)), None
    raise NotImplementedError('scale must be a scalar or a 1-D labelled array along one dim of the field')


# ------------------------------------------------------------------ one call of k_fd
class _Call:
    """Terms, tables and mode of one launch (include/xinv.h, "finite differences")."""

    def __init__(self, f, mode):
        self.f = f
        self.mode = mode
        self.shape = tuple(int(s) for s in f.shape)
        self.iterm, self.dterm, self.tabs = [], [], []
        self.ntab = 0
        self.mask_axis, self.mask_off = -1, -1
        self.inputs = []

    def _table(self, a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
        off = self.ntab
        self.tabs.append(a)
        self.ntab += a.size
        return off

    def _input(self, g):
        for k, h in enumerate(self.inputs):
            if h is g:
                return k
        if isinstance(g, DeviceField) != isinstance(self.f, DeviceField):
            raise ValueError('mixing DeviceField and host inputs in one operator')
        if tuple(g.dims) != tuple(self.f.dims) or tuple(g.shape) != self.shape:
            raise ValueError('every input of one operator must have the same dims and shape: %r vs %r'
                             % (g.dims, self.f.dims))
        self.inputs.append(g)
        return len(self.inputs) - 1

    def term(self, g, dim, scheme='center', BCs=('extend', 'extend'), fill=(0, 0), scale=1, neg=False,
             weight=None, metric=0, msc=0.0, tan=None, R=0.0):
        """One derivative of input g along dim: (neg ? -g : g) * weight, padded by BCs, differenced by `scheme`
        ('center' / 'forward' / 'backward' / 'second'), divided by scale (second: by scale ** 2).
        weight / scale: scalar or (vector, dim)."""
        ax = g.axis(dim)
        n = self.shape[ax]
        if n < 2:
            raise ValueError('the derivative axis %r needs at least 2 points' % dim)
        c = _coord(g, dim)
        kind = _SECOND if scheme == 'second' else _KINDS[scheme]
        I = [-1] * _ITERM
        D = [0.0] * _DTERM
        I[0], I[1], I[2], I[3] = kind, self._input(g), int(bool(neg)), ax
        I[4], I[5], I[6], I[7] = 1, 1, 1, metric
        if kind in (0, _SECOND):
            BCs = _BC_pair(BCs)
            fl, fr = _fill_pair(fill)
            I[4], I[5] = _BC_CODES[BCs[0]], _BC_CODES[BCs[1]]
            D[0], D[1] = fl, fr
        if kind == 0 or metric == 2:
            tab, uniform = gradient_tables(c, padded=True)
            I[6] = int(uniform)
            D[2] = 2. * tab[-3]                           # numpy: (f[2:] - f[:-2]) / (2. * dx), dx = diff(x)[0]
            if not uniform:
                m = n + 2
                I[10] = self._table(np.concatenate([tab[1:m - 1], tab[m + 1:2 * m - 1], tab[2 * m + 1:3 * m - 1]]))
        if kind == 1:
            I[11] = self._table(np.concatenate([c[:-1] - c[1:], [np.nan]]))
        elif kind == 2:
            I[11] = self._table(np.concatenate([[np.nan], c[:-1] - c[1:]]))
        elif kind == _SECOND:
            h = np.diff(padded_coord(c))[:n]              # xarray aligns the two diffs on the lower labels
            I[11] = self._table(h ** 2)
        if weight is not None:
            wv, wd = weight
            I[8], I[12] = g.axis(wd), self._table(wv)
        sv, sd = _vector(scale, g)
        if kind == _SECOND:
            sv = sv ** 2
        if sd is None:
            D[3] = float(sv)
        else:
            I[9], I[13] = g.axis(sd), self._table(sv)
        if metric == 2:
            D[4], D[5] = float(msc), float(R)
            I[14] = self._table(tan)
        self.iterm.append(I)
        self.dterm.append(D)

    def mask(self, keep, dim):
        self.mask_axis, self.mask_off = self.f.axis(dim), self._table(keep)

    def run(self):
        nout = len(self.iterm) if self.mode == _EACH else 1
        if isinstance(self.f, DeviceField):
            return self._run_dev(nout)
        L = _lib.require_gpu()
        ins = [np.ascontiguousarray(np.asarray(g.values, dtype=np.float64)) for g in self.inputs]
        if min(self.shape) < 1:
            raise ValueError('empty field')
        outs = [np.empty(self.shape, dtype=np.float64) for _ in range(nout)]
        tab = np.concatenate(self.tabs) if self.tabs else np.zeros(1)
        self._call(L.xinv_fd_f64, [a.ctypes.data for a in ins], [a.ctypes.data for a in outs], tab.ctypes.data)
        return outs

    def _run_dev(self, nout):
        import torch
        L = _lib.require_gpu()
        ins = [g.values for g in self.inputs]
        for t in ins:
            if t.device != ins[0].device:
                raise ValueError('every input must be on the same device')
        dev = ins[0].device
        outs = [torch.empty(self.shape, dtype=torch.float64, device=dev) for _ in range(nout)]
        with torch.cuda.device(dev):
            tab = torch.from_numpy(np.concatenate(self.tabs) if self.tabs else np.zeros(1)).to(dev)
            self._call(L.xinv_fd_f64_dev, [_lib.dptr(t) for t in ins], [_lib.dptr(t) for t in outs], _lib.dptr(tab),
                       _lib.stream_arg(dev))
        return outs

    def _call(self, fn, ins, outs, tab, *stream):
        vp = ctypes.c_void_p
        inp = (vp * len(ins))(*ins)
        outp = (vp * len(outs))(*outs)
        shape = np.array(self.shape, dtype=np.int64)
        iterm = np.ascontiguousarray(np.array(self.iterm, dtype=np.int64).ravel())
        dterm = np.ascontiguousarray(np.array(self.dterm, dtype=np.float64).ravel())
        i64 = ctypes.POINTER(ctypes.c_int64)
        f64 = ctypes.POINTER(ctypes.c_double)
        args = [ctypes.cast(inp, ctypes.POINTER(vp)), len(ins), ctypes.cast(outp, ctypes.POINTER(vp)), len(outs),
                len(self.shape), shape.ctypes.data_as(i64), self.mode, len(self.iterm), iterm.ctypes.data_as(i64),
                dterm.ctypes.data_as(f64), tab, self.ntab, self.mask_axis, self.mask_off]
        _lib.check(fn(*args, *stream))


# ------------------------------------------------------------------ module functions
def padBCs(v, dim, BCs, fill=(0, 0), dims=None):
    """Pad `v` by one point per end along `dim` (reference finitediffs.py:548-606), on the host with numpy.

    BCs: 'fixed' (the fill), 'extend' (the edge value), 'reflect' (the first inner value) or 'periodic' (both ends),
    a str or a (low, high) pair.  The padded coordinate is extrapolated linearly at both ends."""
    tmpl = v
    f = from_any(v, dims)
    BCs = _BC_pair(BCs)
    vals = np.asarray(f.values)
    ax = f.axis(dim)
    c = _coord(f, dim)
    pw = [(0, 0)] * vals.ndim
    if BCs[0] == 'periodic':
        pw[ax] = (1, 1)
        p = np.pad(vals, pw, mode='wrap')
    else:
        p = vals
        fl, fr = _fill_pair(fill)
        for B, shp, fv in zip(BCs, [(1, 0), (0, 1)], (fl, fr)):
            pw[ax] = shp
            if B == 'fixed':
                p = np.pad(p, pw, mode='constant', constant_values=fv)
            elif B == 'extend':
                p = np.pad(p, pw, mode='edge')
            else:
                p = np.pad(p, pw, mode='reflect')
    coords = dict(f.coords)
    coords[dim] = padded_coord(c)
    res = Field(p, f.dims, coords, f.name)
    if isinstance(tmpl, np.ndarray):
        return p
    return to_like(res, tmpl)


def deriv(v, dim, BCs=('extend', 'extend'), fill=(0, 0), scale=1, scheme='center', dims=None):
    """First derivative along `dim` (reference finitediffs.py:609-659), one kernel launch.

    scheme 'center': numpy.gradient on the BC-padded field (xarray .differentiate), the padded points dropped;
    'forward' / 'backward': one-sided differences without padding, NaN at the far end.  The result is divided by
    `scale`: a scalar or a 1-D labelled array along one dim of v."""
    if scheme not in _KINDS:
        raise Exception('unsupported scheme: ' + str(scheme) +
                        ', should be in [\'center\', \'forward\', \'backward\']')
    f = _field(v, dims)
    call = _Call(f, _EACH)
    call.term(f, dim, scheme, BCs, fill, scale)
    return _out(call.run()[0], f, v)


def deriv2(v, dim, BCs=('extend', 'extend'), fill=(0, 0), scale=1, dims=None):
    """Second derivative along `dim` (reference finitediffs.py:662-702), one kernel launch: the second difference of
    the BC-padded field over the squared lower spacing of the padded coordinate, then over scale ** 2.

    That is the reference's formula, and it is a second derivative only where the spacing is uniform: on a stretched
    coordinate (pressure levels) the result does not converge to f'' however fine the grid."""
    f = _field(v, dims)
    call = _Call(f, _EACH)
    call.term(f, dim, 'second', BCs, fill, scale)
    return _out(call.run()[0], f, v)


# ------------------------------------------------------------------ FiniteDiff
def _overwriteBCs(BCsNew, BCsOld):
    """reference finitediffs.py:732-753"""
    if BCsNew is None:
        return BCsOld
    BCs = dict(BCsOld)
    if isinstance(BCsNew, str):
        for B in BCsOld:
            BCs[B] = (BCsNew, BCsNew)
    elif isinstance(BCsNew, dict):
        for B in BCsNew:
            if B in BCsOld:
                BCs[B] = (BCsNew[B], BCsNew[B]) if isinstance(BCsNew[B], str) else BCsNew[B]
    return BCs


def _overwriteFills(fillsNew, fillsOld):
    """reference finitediffs.py:755-772"""
    if fillsNew is None:
        return fillsOld
    fills = dict(fillsOld)
    if isinstance(fillsNew, (int, float)) and not isinstance(fillsNew, bool):
        for f in fillsOld:
            fills[f] = (fillsNew, fillsNew)
    elif isinstance(fillsNew, dict):
        for f in fillsNew:
            if f in fillsOld:
                fills[f] = fillsNew[f]
    return fills


class FiniteDiff:
    """Finite-difference operators on an Arakawa A grid, lat-lon or cartesian (reference finitediffs.py:13-545).

    dim_mapping maps 'T', 'Z', 'Y', 'X' to the field's dim names; BCs / fill are the defaults per mapped dim, a per-call
    argument overrides them.  Each method is one kernel launch per returned array.  See the module docstring for the
    deviations from the reference."""

    def __init__(self, dim_mapping, BCs='extend', coords='lat-lon', fill=0, R=6371200.0):
        if BCs is None:
            BCs = {dim: ('extend', 'extend') for dim in dim_mapping}
        elif isinstance(BCs, str):
            BCs = {dim: (BCs, BCs) for dim in dim_mapping}
        elif isinstance(BCs, dict):
            BCs = dict(BCs)
            for dim in dim_mapping:
                if dim not in BCs:
                    BCs[dim] = ('extend', 'extend')
                elif isinstance(BCs[dim], str):
                    BCs[dim] = (BCs[dim], BCs[dim])
        if fill is None:
            fill = {dim: (0, 0) for dim in dim_mapping}
        elif isinstance(fill, (int, float)) and not isinstance(fill, bool):
            fill = {dim: (fill, fill) for dim in dim_mapping}
        elif isinstance(fill, dict):
            fill = dict(fill)
            for dim in dim_mapping:
                if dim not in fill:
                    fill[dim] = (0, 0)
        self.dmap = dim_mapping
        self.BCs = BCs
        self.fill = fill
        self.coords = coords
        self.R = R
        if coords not in ['lat-lon', 'cartesian']:
            raise Exception('unsupported coords: ' + coords +
                            ', should be one of [\'lat-lon\', \'cartesian\']')

    def __repr__(self):
        typ = '     Name,               BCs (l-r),     fills  => \'{:s}\' coords\n'.format(self.coords)
        out = ['{:>1s}: {:>6s}  {:>24s}  {:>8s}\n'.format(str(dim), str(name), str(self.BCs[dim]), str(self.fill[dim]))
               for dim, name in self.dmap.items()]
        return typ + ''.join(out)

    def _cos(self, f):
        """cos(deg2rad(lat)) along the Y dim of f, or None when f has no Y dim."""
        if 'Y' in self.dmap and self.dmap['Y'] in f.dims:
            return np.cos(np.deg2rad(_coord(f, self.dmap['Y'])))
        return None

    def grad(self, v, dims=['X', 'Y'], BCs=None, fill=None):
        """Gradient components along `dims` (one launch, one output per dim): a single array for one dim, else a
        list in the order of dims."""
        BCs = _overwriteBCs(BCs, self.BCs)
        fill = _overwriteFills(fill, self.fill)
        llc = self.coords == 'lat-lon'
        if isinstance(dims, str):
            dims = [dims]
        f = _field(v)
        call = _Call(f, _EACH)
        for dim in dims:
            dimName = self.dmap[dim]
            if dim == 'Y' and llc:
                scale = np.pi * self.R / 180.0
            elif dim == 'X' and llc:
                cos = self._cos(f)
                scale = np.pi * self.R / 180.0 * (1 if cos is None else cos)
                if cos is not None:
                    scale = (scale, self.dmap['Y'])
            else:
                scale = 1
            call.term(f, dimName, 'center', BCs[dim], fill[dim], scale)
        re = [_out(o, f, v) for o in call.run()]
        return re[0] if len(re) == 1 else re

    def divg(self, vector, dims, BCs=None, fill=None):
        """Divergence: the sum of d(component)/d(dim) over the pairs (one launch); lat-lon Y components are weighted
        by cos(lat) before differencing."""
        return self._divg(vector, dims, BCs, fill, negate_second=False)

    def _divg(self, vector, dims, BCs, fill, negate_second):
        BCs = _overwriteBCs(BCs, self.BCs)
        fill = _overwriteFills(fill, self.fill)
        llc = self.coords == 'lat-lon'
        if isinstance(dims, str):
            dims = [dims]
        if not isinstance(vector, (list, tuple)):
            vector = [vector]
        if len(vector) != len(dims):
            raise Exception('lengths of vector and dims are not equal')
        comps = [_field(c) for c in vector]
        call = _Call(comps[0], _SUM)
        for k, (comp, dim) in enumerate(zip(comps, dims)):
            dimName = self.dmap[dim]
            weight = None
            if llc and dim == 'Y':
                cos = np.cos(np.deg2rad(_coord(comp, self.dmap['Y'])))
                scale = (np.pi * self.R / 180.0 * cos, self.dmap['Y'])
                weight = (cos, self.dmap['Y'])
            elif llc and dim == 'X':
                cos = self._cos(comps[0])
                scale = np.pi * self.R / 180.0 * (1 if cos is None else cos)
                if cos is not None:
                    scale = (scale, self.dmap['Y'])
            else:
                scale = 1
            call.term(comp, dimName, 'center', BCs[dim], fill[dim], scale, neg=negate_second and k == 1,
                      weight=weight)
        return _out(call.run()[0], comps[0], vector[0])

    def vort(self, u=None, v=None, w=None, components='k', BCs=None, fill=None):
        """Vorticity components 'i' (dw/dy - dv/dz), 'j' (du/dz - dw/dx), 'k' (dv/dx - du/dy), one launch each; a single
        array for one component, else a list in the order of components."""
        BCs = _overwriteBCs(BCs, self.BCs)
        fill = _overwriteFills(fill, self.fill)
        llc = self.coords == 'lat-lon'
        dims = self.dmap
        if isinstance(components, str):
            components = [components]
        fu, fv, fw = (None if a is None else _field(a) for a in (u, v, w))
        tmp = next(a for a in (fu, fv, fw) if a is not None)
        tmpl = next(a for a in (u, v, w) if a is not None)
        weight = None
        if llc:
            cos = np.cos(np.deg2rad(_coord(tmp, dims['Y']))) if dims['Y'] in tmp.dims else None
            if cos is None:
                scale = np.deg2rad(1.0) * self.R * 1
            else:
                scale = (np.deg2rad(1.0) * self.R * cos, dims['Y'])
                weight = (cos, dims['Y'])
        else:
            scale = 1.0
        vors = []
        for comp in components:
            if comp == 'i':      # wy - vz
                call = _Call(fw, _DIFF)
                call.term(fw, dims['Y'], 'center', BCs['Y'], fill['Y'], scale, weight=weight)
                call.term(fv, dims['Z'], 'center', BCs['Z'], fill['Z'], 1.0)
            elif comp == 'j':    # uz - wx
                call = _Call(fu, _DIFF)
                call.term(fu, dims['Z'], 'center', BCs['Z'], fill['Z'], 1.0)
                call.term(fw, dims['X'], 'center', BCs['X'], fill['X'], scale)
            elif comp == 'k':    # vx - uy
                call = _Call(fv, _DIFF)
                call.term(fv, dims['X'], 'center', BCs['X'], fill['X'], scale)
                call.term(fu, dims['Y'], 'center', BCs['Y'], fill['Y'], scale, weight=weight)
            else:
                raise Exception('invalid component ' + str(comp) + ', only in [i, j, k]')
            vors.append(_out(call.run()[0], tmp, tmpl))
        return vors if len(vors) != 1 else vors[0]

    def curl(self, u, v, BCs=None, fill=None):
        """Vertical vorticity: vort(u=u, v=v, components='k')."""
        return self.vort(u=u, v=v, components='k', BCs=BCs, fill=fill)

    def Laplacian(self, v, dims=['X', 'Y'], BCs=None, fill=None):
        """Laplacian of a scalar (one launch): the second derivatives along `dims` summed in their order, with the
        lat-lon metric term on Y and the points at |lat| == 90 set to 0.  Each second derivative is `deriv2`'s: along a
        non-uniform dim (pressure levels as 'Z') it is not consistent."""
        BCs = _overwriteBCs(BCs, self.BCs)
        fill = _overwriteFills(fill, self.fill)
        llc = self.coords == 'lat-lon'
        dmap = self.dmap
        if isinstance(dims, str):
            dims = [dims]
        f = _field(v)
        call = _Call(f, _SUM)
        for dim in dims:
            if llc and dim in ['X', 'Y']:
                dimN = dmap['Y']
                latR = np.deg2rad(_coord(f, dimN))
                cosL = np.cos(latR)
                if dim == 'Y':
                    scale = np.pi * self.R / 180.0
                    call.term(f, dmap['Y'], 'second', BCs['Y'], fill['Y'], scale, metric=2, msc=scale,
                              tan=np.tan(latR), R=self.R)
                    continue
                scale = (np.pi * self.R / 180.0 * cosL, dimN)
            else:
                scale = 1.0
            call.term(f, dmap[dim], 'second', BCs[dim], fill[dim], scale, metric=1)
        if llc and 'Y' in dims:
            call.mask((np.abs(_coord(f, dmap['Y'])) != 90).astype(np.float64), dmap['Y'])
        return _out(call.run()[0], f, v)

    def tension_strain(self, u, v, dims=['X', 'Y'], BCs=None, fill=None):
        """Tension strain du/dx - dv/dy = divg((u, -v), dims), the negation folded into the launch."""
        return self._divg((u, v), dims, BCs, fill, negate_second=True)

    def shear_strain(self, u, v, dims=['X', 'Y'], BCs=None, fill=None):
        raise NotImplementedError('shear_strain: the reference calls vort() with an unsupported `dims` argument '
                                  '(xinvert/finitediffs.py:488) and raises TypeError; not built here')

    def deformation_rate(self, u, v, dims=['X', 'Y'], BCs=None, fill=None):
        raise NotImplementedError('deformation_rate: the reference reaches shear_strain (xinvert/finitediffs.py:516), '
                                  'which raises TypeError; not built here')

    def Okubo_Weiss(self, u, v, dims=['X', 'Y'], BCs=None, fill=None):
        raise NotImplementedError('Okubo_Weiss: the reference reaches deformation_rate (xinvert/finitediffs.py:542), '
                                  'which raises TypeError; not built here')
