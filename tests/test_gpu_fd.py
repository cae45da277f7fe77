"""Finite differences on the GPU (k_fd, xinvert_amd/csrc/xinv_fd.h) against the numpy restatement tests/fd_model.py,
bit for bit in float64 (NaN where the model has NaN, the sign of zero included)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_model as M  # noqa: E402
from xinvert_amd.field import Field  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def same(a, b):
    a = np.asarray(a.values if hasattr(a, 'values') else a)
    b = np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def coords_for(kind, n):
    if kind == 'uniform':
        return np.arange(n) * 0.25 - 3.0
    if kind == 'linspace':                           # uniform up to the last bit
        return np.linspace(-90.0, 90.0, n)
    return 1000.0 * 0.93 ** np.arange(n)           # pressure-like levels, truly non-uniform


BC_PAIRS = [(a, b) for a in ('fixed', 'extend', 'reflect') for b in ('fixed', 'extend', 'reflect')] + \
           [('periodic', 'periodic')]


@pytest.mark.parametrize('n', [2, 3, 64, 1001])
@pytest.mark.parametrize('scheme', ['center', 'forward', 'backward', 'second'])
def test_deriv_and_deriv2_equal_the_model(n, scheme):
    from xinvert_amd import deriv, deriv2
    rng = np.random.default_rng(n)
    fill = (1.5, -2.25)
    for ckind in ('uniform', 'linspace', 'levels'):
        c = coords_for(ckind, n)
        for axis in (0, 1, 2):
            shape = [5, 6, 7]
            shape[axis] = n
            dims = ('a', 'b', 'c')
            f = Field(rng.standard_normal(shape), dims, {dims[axis]: c})
            f.values[tuple(rng.integers(0, s) for s in shape)] = np.nan
            dim = dims[axis]
            for BCs in (BC_PAIRS if scheme in ('center', 'second') else [('extend', 'extend')]):
                for scale in (1, 3.5):
                    if scheme == 'second':
                        got = deriv2(f, dim, BCs, fill, scale)
                        want = M.deriv2(f, dim, BCs, fill, scale)
                    else:
                        got = deriv(f, dim, BCs, fill, scale, scheme)
                        want = M.deriv(f, dim, BCs, fill, scale, scheme)
                    assert same(got, want), (ckind, axis, BCs, scale)


def test_deriv_scale_along_another_axis():
    from xinvert_amd import deriv, deriv2
    rng = np.random.default_rng(1)
    lat = np.linspace(-60, 60, 41)
    lon = np.arange(50) * 7.2
    f = Field(rng.standard_normal((3, 41, 50)), ('t', 'lat', 'lon'), {'lat': lat, 'lon': lon})
    cos = Field(np.cos(np.deg2rad(lat)), ('lat',), {'lat': lat})
    sc = M._along(cos.values, f, 'lat')
    assert same(deriv(f, 'lon', 'periodic', scale=cos), M.deriv(f, 'lon', 'periodic', scale=sc))
    assert same(deriv2(f, 'lon', 'periodic', scale=cos), M.deriv2(f, 'lon', 'periodic', scale=sc))
    assert same(deriv(f, 'lat', ('fixed', 'reflect'), (2, 3), scale=cos),
                M.deriv(f, 'lat', ('fixed', 'reflect'), (2, 3), scale=sc))


def _grid():
    d = np.load(os.path.join(HERE, 'golden', 'poisson_atmos.npz'))
    return d['lat'], d['lon']


def _fields(dims, coords, k, seed=0, nan=True):
    rng = np.random.default_rng(seed)
    shape = tuple(len(coords[d]) for d in dims)
    out = []
    for _ in range(k):
        v = rng.standard_normal(shape) * 10.0
        if nan:
            v[..., 10:14, 20:30] = np.nan                # land points
        out.append(Field(v, dims, coords))
    return out


CONFIGS = [
    dict(BCs={'Z': ('fixed', 'extend'), 'Y': ('reflect', 'fixed'), 'X': 'periodic'},
         fill={'Z': (1.0, 2.0), 'Y': (0.5, -0.5), 'X': (0, 0)}),
    dict(BCs='extend', fill=0),
    dict(BCs={'Y': ('fixed', 'fixed'), 'X': ('reflect', 'extend'), 'Z': 'reflect'}, fill=3.0),
]


@pytest.mark.parametrize('coords', ['lat-lon', 'cartesian'])
@pytest.mark.parametrize('cfg', range(len(CONFIGS)))
def test_FiniteDiff_equals_the_model(coords, cfg):
    from xinvert_amd import FiniteDiff
    lat, lon = _grid()
    lev = np.array([1000., 850., 700., 500., 300.])
    dims = ('lev', 'lat', 'lon')
    crd = {'lev': lev, 'lat': lat, 'lon': lon}
    u, v, w = _fields(dims, crd, 3, seed=cfg)
    dm = {'Z': 'lev', 'Y': 'lat', 'X': 'lon'}
    fd = FiniteDiff(dm, BCs=CONFIGS[cfg]['BCs'], fill=CONFIGS[cfg]['fill'], coords=coords)
    md = M.FiniteDiff(dm, fd.BCs, fd.fill, coords)
    assert same(fd.grad(u, ['X']), md.grad(u, ['X']))
    for a, b in zip(fd.grad(u, ['Y', 'X']), md.grad(u, ['Y', 'X'])):
        assert same(a, b)
    for a, b in zip(fd.grad(u, ['Z', 'Y', 'X']), md.grad(u, ['Z', 'Y', 'X'])):
        assert same(a, b)
    assert same(fd.divg([u, v], ['X', 'Y']), md.divg([u, v], ['X', 'Y']))
    assert same(fd.divg((v, u, w), ['Y', 'X', 'Z']), md.divg((v, u, w), ['Y', 'X', 'Z']))
    assert same(fd.divg(w, 'Z'), md.divg([w], ['Z']))
    for comp in ('i', 'j', 'k'):
        assert same(fd.vort(u=u, v=v, w=w, components=comp), md.vort(u=u, v=v, w=w, components=comp)), comp
    got = fd.vort(u=u, v=v, w=w, components=['k', 'i'])
    want = md.vort(u=u, v=v, w=w, components=['k', 'i'])
    assert all(same(a, b) for a, b in zip(got, want))
    assert same(fd.curl(u, v), md.curl(u, v))
    for dims_ in (['X', 'Y'], ['Y', 'X'], ['Z', 'Y', 'X']):
        assert same(fd.Laplacian(u, dims_), md.Laplacian(u, dims_)), dims_
    assert same(fd.tension_strain(u, v), md.tension_strain(u, v, ['X', 'Y']))
    assert same(fd.tension_strain(u, v, ['Y', 'X']), md.tension_strain(u, v, ['Y', 'X']))


def test_Laplacian_zero_at_the_poles_and_2d_lat_lon():
    from xinvert_amd import FiniteDiff
    lat, lon = _grid()
    (s,) = _fields(('lat', 'lon'), {'lat': lat, 'lon': lon}, 1, seed=5, nan=False)
    fd = FiniteDiff({'Y': 'lat', 'X': 'lon'}, BCs={'Y': 'extend', 'X': 'periodic'})
    md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill)
    got = fd.Laplacian(s, ['Y', 'X'])
    assert same(got, md.Laplacian(s, ['Y', 'X']))
    assert (got.values[0] == 0).all() and (got.values[-1] == 0).all() and not np.signbit(got.values[0]).any()


def test_reference_identities_on_the_fixture():
    # reference tests/test_FDs.py:40-64
    from xinvert_amd import FiniteDiff, deriv
    d = np.load(os.path.join(HERE, 'golden', 'poisson_atmos.npz'))
    T = Field(d['S60_ep'][0], ('lat', 'lon'), {'lat': d['lat'], 'lon': d['lon']})
    Tx1 = deriv(T, dim='lon', scheme='center').values
    Tx2 = deriv(T, dim='lon', scheme='forward').values
    Tx3 = deriv(T, dim='lon', scheme='backward').values
    assert np.isclose(Tx1[1:-1, 1:-1], (Tx2 + Tx3)[1:-1, 1:-1] / 2, rtol=5e-5).all()
    fd = FiniteDiff(dim_mapping={'T': 'time', 'Y': 'lat', 'X': 'lon'}, BCs={'Y': 'reflect', 'X': 'periodic'},
                    coords='lat-lon')
    Ty, Tx = fd.grad(T, dims=['Y', 'X'])
    Tcurl = fd.curl(Tx, Ty)
    assert (np.abs(Tcurl.values) < 5e-11).all()
    md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill)
    assert same(Tcurl, md.curl(Tx, Ty))


def test_float32_inputs_are_widened():
    from xinvert_amd import FiniteDiff
    d = np.load(os.path.join(HERE, 'golden', 'poisson_atmos.npz'))
    v32 = d['vor_f32'][0]
    assert v32.dtype == np.float32
    F = Field(v32, ('lat', 'lon'), {'lat': d['lat'], 'lon': d['lon']})
    F64 = Field(v32.astype(np.float64), ('lat', 'lon'), {'lat': d['lat'], 'lon': d['lon']})
    fd = FiniteDiff({'Y': 'lat', 'X': 'lon'}, BCs={'Y': 'fixed', 'X': 'periodic'})
    md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill)
    got = fd.Laplacian(F, ['X', 'Y'])
    assert got.values.dtype == np.float64
    assert same(got, md.Laplacian(F64, ['X', 'Y']))
    for a, b in zip(fd.grad(F, ['X', 'Y']), md.grad(F64, ['X', 'Y'])):
        assert same(a, b)


def test_device_fields_on_a_side_stream_equal_the_host_results():
    import torch
    from xinvert_amd import FiniteDiff, deriv
    from xinvert_amd.finitediffs import DeviceField
    lat, lon = _grid()
    lev = np.array([1000., 850., 700., 500.])
    dims = ('lev', 'lat', 'lon')
    crd = {'lev': lev, 'lat': lat, 'lon': lon}
    u, v, w = _fields(dims, crd, 3, seed=11)
    fd = FiniteDiff({'Z': 'lev', 'Y': 'lat', 'X': 'lon'}, BCs=CONFIGS[0]['BCs'], fill=CONFIGS[0]['fill'])
    dev = torch.device('cuda', torch.cuda.current_device())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        du, dv, dw = (DeviceField(torch.from_numpy(a.values).to(dev), dims, crd) for a in (u, v, w))
        res = {
            'curl': fd.curl(du, dv), 'divg': fd.divg([du, dv, dw], ['X', 'Y', 'Z']),
            'lap': fd.Laplacian(du, ['Y', 'X']), 'vi': fd.vort(u=du, v=dv, w=dw, components='i'),
            'ts': fd.tension_strain(du, dv), 'gy': fd.grad(du, ['Y', 'Z'])[0],
            'fw': deriv(du, 'lat', scheme='forward'),
        }
        out = {k: r.values.cpu().numpy() for k, r in res.items()}
    s.synchronize()
    host = {
        'curl': fd.curl(u, v), 'divg': fd.divg([u, v, w], ['X', 'Y', 'Z']), 'lap': fd.Laplacian(u, ['Y', 'X']),
        'vi': fd.vort(u=u, v=v, w=w, components='i'), 'ts': fd.tension_strain(u, v),
        'gy': fd.grad(u, ['Y', 'Z'])[0], 'fw': deriv(u, 'lat', scheme='forward'),
    }
    for k in res:
        assert isinstance(res[k], DeviceField)
        assert same(out[k], host[k].values), k


def test_full_size_curl_and_Laplacian():
    from xinvert_amd import FiniteDiff
    lat = np.linspace(-90, 90, 1800)
    lon = np.arange(3600) * 0.1
    rng = np.random.default_rng(7)
    dims = ('time', 'lat', 'lon')
    crd = {'time': np.arange(8.0), 'lat': lat, 'lon': lon}
    u = Field(rng.standard_normal((8, 1800, 3600)), dims, crd)
    fd = FiniteDiff({'T': 'time', 'Y': 'lat', 'X': 'lon'}, BCs={'Y': 'reflect', 'X': 'periodic'})
    md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill)
    assert same(fd.Laplacian(u, ['X', 'Y']), md.Laplacian(u, ['X', 'Y']))
    v = Field(rng.standard_normal((8, 1800, 3600)), dims, crd)
    assert same(fd.curl(u, v), md.curl(u, v))


def test_dev_call_over_2_to_the_31_elements():
    import torch
    from xinvert_amd import FiniteDiff
    from xinvert_amd.finitediffs import DeviceField
    lat = np.linspace(-90, 90, 181)
    lon = np.arange(360) * 1.0
    member = 181 * 360
    nb = (2 ** 31) // member + 1
    assert nb * member > 2 ** 31
    dims = ('t', 'lat', 'lon')
    crd = {'t': np.arange(nb, dtype=np.float64), 'lat': lat, 'lon': lon}
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.randn((nb, 181, 360), dtype=torch.float64, device=dev, generator=g)
    fd = FiniteDiff({'T': 't', 'Y': 'lat', 'X': 'lon'}, BCs={'Y': ('fixed', 'extend'), 'X': 'periodic'}, fill=1.0)
    md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill)
    out = fd.Laplacian(DeviceField(x, dims, crd), ['Y', 'X']).values
    torch.cuda.synchronize()
    for m in (0, nb - 1):
        xm = Field(x[m:m + 1].cpu().numpy(), dims, {'t': crd['t'][m:m + 1], 'lat': lat, 'lon': lon})
        assert same(out[m:m + 1].cpu().numpy(), md.Laplacian(xm, ['Y', 'X'])), m
    del x, out
    torch.cuda.empty_cache()
