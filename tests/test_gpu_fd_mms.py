"""Manufactured fields on the device: the table of tests/fd_mms_cases.py through the public API (k_fd,
k_gm_flow), and k_fd's indexing at the shapes no other test runs.

Every row, at the three grids: the device result meets the order bounds of tests/test_fd_mms_host.py AND is bit for bit
the model's (tests/fd_model.py; NaN and the sign of zero included), so the figures of DESIGN.md 6.2, measured with the
model on the CPU, are the device's.

The indexing cases compare with the model bit for bit.  k_fd views the operand as rows of the last axis; a workgroup marches
rb = clamp(rows * workgroups per row / 4096, 1, 32) consecutive rows (xinv_fd_host.h) and steps a counter (r / srow) % n per
axis.  Below 8192 row-workgroups rb is 1 and every row starts from the division; the stepped branches -- an axis with
srow > 1 that wraps inside a march -- need four dims AND that many rows (`march()` below restates the rule, and the cases
assert that they do march)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_mms_cases as C  # noqa: E402
import fd_model as M  # noqa: E402
from test_fd_mms_host import assert_order  # noqa: E402
from test_gpu_fd import BC_PAIRS, coords_for, same  # noqa: E402
from xinvert_amd import apps  # noqa: E402
from xinvert_amd.field import Field  # noqa: E402

pytestmark = pytest.mark.gpu
ids = lambda k: '/'.join(k)
MODEL = C.ModelAPI()
DEVICE_KEYS = sorted(k for k, r in C.ROWS.items() if r.device)


class PublicAPI:
    """The package's own entry points, on host arrays or (device=True) on DeviceFields on the current stream."""
    name = 'public'

    def __init__(self, device=False):
        self.device = device

    def field(self, f):
        if not self.device:
            return f
        import torch
        from xinvert_amd.finitediffs import DeviceField
        dev = torch.device('cuda', torch.cuda.current_device())
        return DeviceField(torch.from_numpy(np.ascontiguousarray(f.values)).to(dev), f.dims, f.coords)

    def out(self, a):
        v = a.values if hasattr(a, 'values') else a
        return v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)

    def _scale(self, scale, f):
        return Field(scale[0], (scale[1],), {scale[1]: f.coords[scale[1]]}) if isinstance(scale, tuple) else scale

    def deriv(self, f, dim, BCs=('extend', 'extend'), fill=(0, 0), scale=1, scheme='center'):
        from xinvert_amd import deriv
        return deriv(f, dim, BCs, fill, self._scale(scale, f), scheme)

    def deriv2(self, f, dim, BCs=('extend', 'extend'), fill=(0, 0), scale=1):
        from xinvert_amd import deriv2
        return deriv2(f, dim, BCs, fill, self._scale(scale, f))

    def fd(self, dmap, BCs, fill, coords):
        from xinvert_amd import FiniteDiff
        return FiniteDiff(dmap, BCs=BCs, fill=fill, coords=coords)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('op', sorted({k[0] for k in DEVICE_KEYS}))
def test_rows_on_the_device_have_the_order_and_the_models_bits(op):
    """Every row of one operator (both coordinate branches, every variant), at the three grids."""
    api = PublicAPI()
    keys = [k for k in DEVICE_KEYS if k[0] == op]
    assert keys
    for key in keys:
        row = C.ROWS[key]
        es = None
        for n in C.GRIDS:
            p = row.problem(n)
            got = C.run(row, api, p)
            want = C.run(row, MODEL, p)
            for (nm, _, _), a, b in zip(row.outputs, got, want):
                assert same(a, b), (key, n, nm)
            e = C.errors(p, got)
            es = [[v] for v in e] if es is None else [a + [v] for a, v in zip(es, e)]
        for (nm, _, _), e in zip(row.outputs, es):
            assert_order(e, row.order, ids(key) + ' ' + nm)


def test_2d_lat_lon_rows_as_DeviceFields_on_a_side_stream():
    import torch
    keys = [k for k in DEVICE_KEYS if k[2] == 'lat-lon' and C.ROWS[k].rank == 2]
    assert len(keys) >= 8
    api = PublicAPI(device=True)
    s = torch.cuda.Stream()
    got, probs = {}, {}
    with torch.cuda.stream(s):
        for k in keys:
            probs[k] = C.ROWS[k].problem(32)
            got[k] = C.run(C.ROWS[k], api, probs[k])           # (.cpu() waits for the side stream's work)
    s.synchronize()
    for k in keys:
        want = C.run(C.ROWS[k], MODEL, probs[k])
        for (nm, _, _), a, b in zip(C.ROWS[k].outputs, got[k], want):
            assert same(a, b), (k, nm)


@pytest.mark.parametrize('coords', ['lat-lon', 'cartesian'])
def test_gill_matsuno_winds_on_the_device_against_the_analytic_winds(coords):
    """cal_flow_gm_device (k_gm_flow) on a uniform and on a non-uniform latitude axis: the order against the analytic
    winds, and apps.cal_flow's bits."""
    import torch
    keys = sorted(k for k in C.GM_ROWS if k[2] == coords)
    assert len(keys) == 2 and sum('warp' in k[1] for k in keys) == 1
    for key in keys:
        row = C.ROWS[key]
        es = [[], []]
        for n in C.GRIDS:
            p = row.problem(n)
            lat, lon = p['coords']['lat'], p['coords']['lon']
            assert apps.gradient_tables(lat)[1] == ('warp' not in key[1])
            S = torch.from_numpy(np.ascontiguousarray(p['F']['S'].values[None])).cuda()
            u, v = torch.empty_like(S), torch.empty_like(S)
            apps.cal_flow_gm_device(S.data_ptr(), u.data_ptr(), v.data_ptr(), 1, lat, lon, coords=coords,
                                    mParams=C.GM_PARAMS[coords])
            torch.cuda.synchronize()
            got = [u.cpu().numpy()[0], v.cpu().numpy()[0]]
            want = C.run(row, MODEL, p)
            for a, b in zip(got, want):
                assert same(a, b), (key, n)
            for k, e in enumerate(C.errors(p, got)):
                es[k].append(e)
        for nm, e in zip('uv', es):
            assert_order(e, 2, ids(key) + ' ' + nm)


# ------------------------------------------------------------------------------------------------ k_fd's indexing
def march(shape):
    """Rows a workgroup of k_fd marches for an operand of this shape (xinv_fd_host.h: rb)."""
    nx = shape[-1]
    nr = int(np.prod(shape[:-1], dtype=np.int64))
    nbx = (nx + 255) // 256
    return max(1, min(32, nr * nbx // 4096))


def _random(shape, dims, coords, k, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        v = rng.standard_normal(shape)
        v[tuple(rng.integers(0, s) for s in shape)] = np.nan
        out.append(Field(v, dims, coords))
    return out


# (time, lev, lat, lon): the first two are the issue's small shapes (rb = 1: every row starts from the division); the others
# march 5, 32 and 2 rows, with lev * lat no multiple of the march, so that lev (srow = lat > 1) and lat wrap inside a march
SHAPES_4D = [(3, 4, 9, 40), (2, 5, 37, 300), (976, 3, 7, 2), (2731, 4, 12, 2), (106, 3, 13, 257)]
MARCH_4D = [1, 1, 5, 32, 2]


@pytest.mark.parametrize('shape,rb', list(zip(SHAPES_4D, MARCH_4D)), ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else 'rb%d' % v)
def test_four_dims_equal_the_model(shape, rb):
    from xinvert_amd import FiniteDiff, deriv, deriv2
    from xinvert_amd.finitediffs import _Call, _EACH
    assert march(shape) == rb
    if rb > 1:
        assert (shape[1] * shape[2]) % rb != 0 and shape[2] % rb != 0
    dims = ('time', 'lev', 'lat', 'lon')
    nt, nz, ny, nx = shape
    crd = {'time': np.arange(nt, dtype=np.float64), 'lev': 1000.0 * 0.8 ** np.arange(nz),
           'lat': np.linspace(-75.0, 80.0, ny), 'lon': np.arange(nx) * (360.0 / nx)}
    u, v, w = _random(shape, dims, crd, 3, seed=sum(shape))
    cos = np.cos(np.deg2rad(crd['lat']))
    cosF = Field(cos, ('lat',), {'lat': crd['lat']})
    sc = M._along(cos, u, 'lat')
    fill = (1.5, -2.25)
    for dim, BCs in (('lev', ('fixed', 'reflect')), ('lev', ('extend', 'extend')), ('lat', ('reflect', 'fixed')),
                     ('lon', ('periodic', 'periodic')), ('time', ('extend', 'fixed'))):
        for scale, msc in ((1, 1), (cosF, sc)):                # the scale table runs along lat whatever the derivative's axis
            for scheme in ('center', 'forward', 'backward'):
                assert same(deriv(u, dim, BCs, fill, scale, scheme), M.deriv(u, dim, BCs, fill, msc, scheme)), (dim, BCs, scheme)
            assert same(deriv2(u, dim, BCs, fill, scale), M.deriv2(u, dim, BCs, fill, msc)), (dim, BCs)
    # a pre-weight along lat under a derivative along lev / lon: the kernel's pre-weight counter on another axis than the
    # derivative's (the public methods only ever weight the axis they differentiate)
    for dim, BCs in (('lev', ('reflect', 'extend')), ('lon', ('periodic', 'periodic'))):
        call = _Call(u, _EACH)
        call.term(u, dim, 'center', BCs, fill, (cos, 'lat'), weight=(cos, 'lat'))
        call.term(u, dim, 'second', BCs, fill, (cos, 'lat'), weight=(cos, 'lat'))
        g1, g2 = call.run()
        uw = u.like(u.values * sc)
        assert same(g1, M.deriv(uw, dim, BCs, fill, sc)) and same(g2, M.deriv2(uw, dim, BCs, fill, sc)), dim
    dm = {'T': 'time', 'Z': 'lev', 'Y': 'lat', 'X': 'lon'}
    for coords in ('lat-lon', 'cartesian'):
        fd = FiniteDiff(dm, BCs={'T': 'extend', 'Z': ('fixed', 'extend'), 'Y': ('reflect', 'fixed'), 'X': 'periodic'},
                        fill={'Z': (1.0, 2.0), 'Y': (0.5, -0.5)}, coords=coords)
        md = M.FiniteDiff(dm, fd.BCs, fd.fill, coords)
        assert same(fd.Laplacian(u, ['Z', 'Y', 'X']), md.Laplacian(u, ['Z', 'Y', 'X'])), coords
        assert same(fd.divg((v, u, w), ['Y', 'X', 'Z']), md.divg((v, u, w), ['Y', 'X', 'Z'])), coords
        for a, b in zip(fd.grad(u, ['Z', 'Y', 'X']), md.grad(u, ['Z', 'Y', 'X'])):
            assert same(a, b), coords
        for comp in ('i', 'j', 'k'):
            assert same(fd.vort(u=u, v=v, w=w, components=comp), md.vort(u=u, v=v, w=w, components=comp)), (coords, comp)


def test_one_dim_operand_equals_the_model():
    """nr == 1: one row, the derivative axis is the last and only axis."""
    from xinvert_amd import deriv, deriv2
    for n in (2, 3, 255, 256, 257, 513):
        rng = np.random.default_rng(n)
        fill = (1.5, -2.25)
        for ckind in ('uniform', 'linspace', 'levels'):
            f = Field(rng.standard_normal(n), ('x',), {'x': coords_for(ckind, n)})
            if n > 3:
                f.values[int(rng.integers(0, n))] = np.nan
            for scale in (1, 3.5):
                for BCs in BC_PAIRS:
                    assert same(deriv(f, 'x', BCs, fill, scale), M.deriv(f, 'x', BCs, fill, scale)), (n, ckind, BCs)
                    assert same(deriv2(f, 'x', BCs, fill, scale), M.deriv2(f, 'x', BCs, fill, scale)), (n, ckind, BCs)
                for scheme in ('forward', 'backward'):
                    assert same(deriv(f, 'x', scheme=scheme, scale=scale), M.deriv(f, 'x', scale=scale, scheme=scheme)), (n, ckind, scheme)


# rows x columns: the columns cross a 256-lane workgroup, the rows a 32-row march (rb = 1 at these sizes); the last
# shape has enough rows to march (3 rows, two workgroups per row, the last march cut short by the end of the field)
SHAPES_2D = [(nr, nx) for nr in (31, 32, 33, 65) for nx in (255, 256, 257)] + [(6145, 257)]


def test_two_dims_across_the_workgroup_and_the_march():
    from xinvert_amd import FiniteDiff, deriv, deriv2
    for shape in SHAPES_2D:
        ny, nx = shape
        if ny > 1000:
            assert march(shape) > 1 and ny % march(shape) != 0
        dims = ('lat', 'lon')
        crd = {'lat': np.linspace(-80.0, 85.0, ny), 'lon': np.arange(nx) * (360.0 / nx)}
        u, v = _random(shape, dims, crd, 2, seed=ny * 1000 + nx)
        fill = (1.5, -2.25)
        for dim, BCs in (('lat', ('fixed', 'reflect')), ('lat', ('extend', 'extend')), ('lon', ('periodic', 'periodic')),
                         ('lon', ('reflect', 'fixed'))):
            for scheme in ('center', 'forward', 'backward'):
                assert same(deriv(u, dim, BCs, fill, 1, scheme), M.deriv(u, dim, BCs, fill, 1, scheme)), (shape, dim, BCs, scheme)
            assert same(deriv2(u, dim, BCs, fill, 2.5), M.deriv2(u, dim, BCs, fill, 2.5)), (shape, dim, BCs)
        for coords in ('lat-lon', 'cartesian'):
            fd = FiniteDiff({'Y': 'lat', 'X': 'lon'}, BCs={'Y': ('reflect', 'fixed'), 'X': 'periodic'}, fill=0.75, coords=coords)
            md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill, coords)
            assert same(fd.curl(u, v), md.curl(u, v)), (shape, coords)
            assert same(fd.divg([u, v], ['X', 'Y']), md.divg([u, v], ['X', 'Y'])), (shape, coords)
            assert same(fd.Laplacian(u, ['Y', 'X']), md.Laplacian(u, ['Y', 'X'])), coords
