"""Manufactured solutions for every application of xinvert_amd/apps.py: the table and the helper.

What pins the coefficient builders `apps._coeffs_*` and the grid metrics `apps._cal_params*` from outside: an analytic S,
the CONTINUOUS operator of the app's form applied to it with the coefficient FUNCTIONS the app defines (stated here as
sympy expressions, written as mathematics from the reference's equations and coefficient definitions), the resulting
forcing handed to the front end, and the discrete residual of S (or the error of the discrete solution) shrinking by 4
each time the grid spacing halves.  A first-order mistake gives 2, a wrong term 1.

Coordinates.  x, y, z are METRIC coordinates along the last, second-last and third-last core dim.  A dim measured in
degrees maps to metres as coordinate * pi / 180 * Rearth -- both dims on 'lat-lon' (the two horizontal ones in 3-D), the
second dim on 'z-lat' / 'z-lon', the only dim on 'lat', none on 'cartesian': so y = a phi and x = a lambda, with NO cos(phi)
in x (the builders carry it in the coefficients).  That is what _cal_params1D/2D/3D must compute.

Continuous operators (include/xinv.h, DESIGN.md 1, the point expressions xinv_res_* / xinv_upd_* of xinv_device.h):
    std1d   d/dx(A Sx) + B S                                                       = F
    std2d   d/dy(A Sy + B Sx) + d/dx(B Sy + C Sx)                                  = F
    std2dt  d/dy(A Sy + B Sx) + d/dx(C Sy + D Sx) + E S                            = F
    gen2d   A Syy + B Sxy + C Sxx + D Sy + E Sx + F S                              = G
    bih2d   A Syyyy + B Sxxyy + C Sxxxx + D Syy + E Sxy + F Sxx + G Sy + H Sx + I S = J
    std3d   d/dz(A Sz) + d/dy(B Sy) + d/dx(C Sx)                                   = F
    gen3d   A Szz + B Syy + C Sxx + D Sz + E Sy + F Sx + G S                       = H

Staggering.  In the flux forms the leading coefficient of each direction lives between grid points: A[j] between rows j-1
and j, C[i] (D[i] in std2dt) between columns i-1 and i (STAGGER below).  A builder that evaluates its function there
('half': cosH, _half_shift) is second order as it stands.  A builder that samples the function ON the grid point and lets
the kernel use it at the half point ('grid') is first order against the app's docstring -- that is the reference's
behaviour, not a bug: the manufactured forcing then uses the shifted function A(y + h/2), and the discrete operator is
still second order against what the reference computes.

Boundaries.  'fixed' and 'periodic' only.  The reference's 'extend' copies the neighbour's value into the boundary point:
a one-sided first-order statement of a zero normal derivative, first order by construction, so no second-order check of
it exists.

    CASES[(app, coords)] or [(app, coords, variant)] -> Case;  problem(case, n, mask) -> everything a run needs.
"""
import numpy as np
import sympy as sp

from xinvert_amd import apps, forms
from xinvert_amd.field import Field

X, Y, Z = sp.symbols('x y z', real=True)
HX, HY, HZ = sp.symbols('h_x h_y h_z', real=True)
_AX = (X, Y, Z)                                   # by distance from the last core dim
_H = {X: HX, Y: HY, Z: HZ}
UNDEF = -9.99e8
PI = sp.pi
d = sp.diff

# the coefficient of each flux form that lives on half points, and the direction it is staggered in
STAGGER = {'std1d': {'A': X}, 'std2d': {'A': Y, 'C': X}, 'std2dt': {'A': Y, 'D': X}, 'std3d': {'A': Z, 'B': Y, 'C': X},
           'gen2d': {}, 'gen3d': {}, 'bih2d': {}}
RANK = {k: forms.FORMS[k].rank for k in forms.FORMS}
# apps that have no residual entry: their check is the error of a discrete solve
NO_RESIDUAL = {'stommelmunk': ('_coeffs_StommelMunk', 'inv_general2D_bih'),
               'geoadjustment': ('_coeffs_GeoAdjustment', 'inv_standard1D'),
               'refstateswm': ('_coeffs_RefStateSWM', 'inv_standard1D')}
KIND_OF = {f.inv: f.kind for f in forms.FORMS.values()}


def terms(kind, S, c):
    """The continuous operator of a form on S, term by term: {letter: expression}; their sum is the right-hand side."""
    if kind == 'std1d':
        return {'A': d(c['A'] * d(S, X), X), 'B': c['B'] * S}
    if kind == 'std2d':
        return {'A': d(c['A'] * d(S, Y), Y), 'B': d(c['B'] * d(S, X), Y) + d(c['B'] * d(S, Y), X), 'C': d(c['C'] * d(S, X), X)}
    if kind == 'std2dt':
        return {'A': d(c['A'] * d(S, Y), Y), 'B': d(c['B'] * d(S, X), Y), 'C': d(c['C'] * d(S, Y), X),
                'D': d(c['D'] * d(S, X), X), 'E': c['E'] * S}
    if kind == 'gen2d':
        return {'A': c['A'] * d(S, Y, 2), 'B': c['B'] * d(S, X, Y), 'C': c['C'] * d(S, X, 2), 'D': c['D'] * d(S, Y),
                'E': c['E'] * d(S, X), 'F': c['F'] * S}
    if kind == 'bih2d':
        return {'A': c['A'] * d(S, Y, 4), 'B': c['B'] * d(S, X, 2, Y, 2), 'C': c['C'] * d(S, X, 4), 'D': c['D'] * d(S, Y, 2),
                'E': c['E'] * d(S, X, Y), 'F': c['F'] * d(S, X, 2), 'G': c['G'] * d(S, Y), 'H': c['H'] * d(S, X), 'I': c['I'] * S}
    if kind == 'std3d':
        return {'A': d(c['A'] * d(S, Z), Z), 'B': d(c['B'] * d(S, Y), Y), 'C': d(c['C'] * d(S, X), X)}
    if kind == 'gen3d':
        return {'A': c['A'] * d(S, Z, 2), 'B': c['B'] * d(S, Y, 2), 'C': c['C'] * d(S, X, 2), 'D': c['D'] * d(S, Z),
                'E': c['E'] * d(S, Y), 'F': c['F'] * d(S, X), 'G': c['G'] * S}
    raise KeyError(kind)


def degree_dims(coords, rank):
    """Which core dims (by position) are in degrees -- the statement of _cal_params*."""
    c = coords.lower()
    if c == 'lat-lon':
        return (0, 1) if rank == 2 else (1, 2)
    if c in ('z-lat', 'z-lon'):
        return (1,)
    if c == 'lat':
        return (0,)
    if c == 'cartesian':
        return ()
    raise KeyError(coords)


class Case:
    """One app in one coordinate branch.

    axes     per core dim (lo, hi, 'closed' | 'open') in the user's units: 'closed' holds both ends and (multiple of n) + 1
             points; 'open' holds lo + (hi - lo) * k / N (a periodic dim, or an even count whose spacing still halves)
    shape    n -> the grid's shape
    coef     {letter: (expression, 'half' | 'grid')}; a letter left out is identically zero
    S        the manufactured solution
    user     G -> the user-level forcing as an expression, G being the form's right-hand side L(S)
    rhs      for apps whose right-hand side the builder dictates: the expression L(S) must equal (checked numerically)
    fields   G -> {mParams key: (expression, 'full' | 'vec0' | 'col0')}: array-valued model parameters sampled on the grid
    """

    def __init__(self, app, coords, dims, axes, BCs, mParams, coef, S, user, shape, rhs=None, fields=None, note=''):
        self.app, self.coords, self.dims, self.axes, self.BCs = app, coords, tuple(dims), axes, list(BCs)
        self.mParams, self.coef, self.S, self.user, self.shape, self.rhs = mParams, coef, S, user, shape, rhs
        self.fields = fields or (lambda G: {})
        self.note = note
        name = app.lower()
        self.builder, inv = (apps._RESIDUAL[name][0], apps._RESIDUAL[name][1]) if name in apps._RESIDUAL else NO_RESIDUAL[name]
        self.inv = inv
        self.kind = KIND_OF[inv]
        self.valid = _VALID[name]
        self.rank = RANK[self.kind]
        self.a = float(mParams.get('Rearth', apps.default_mParams['Rearth']))
        self._fn = None

    # ---- symbolic side
    def effective(self):
        """The coefficient functions the discrete operator sees: 'grid'-flagged staggered ones shifted by half a cell."""
        out = {}
        for L in forms.FORMS[self.kind].arrays[:-1]:
            e, flag = self.coef.get(L, (sp.Integer(0), 'half'))
            e = sp.sympify(e)
            ax = STAGGER[self.kind].get(L)
            if ax is not None and flag == 'grid':
                e = e.subs(ax, ax + _H[ax] / 2)
            out[L] = e
        return out

    def grid_flagged(self):
        return [L for L, (e, flag) in self.coef.items() if flag == 'grid' and L in STAGGER[self.kind]
                and sp.sympify(e).has(STAGGER[self.kind][L])]

    def functions(self):
        if self._fn is None:
            t = {k: v for k, v in terms(self.kind, self.S, self.effective()).items() if v != 0}
            G = sum(t.values())
            args = [X, Y, Z, HX, HY, HZ]
            lam = lambda e: sp.lambdify(args, sp.sympify(e), 'numpy')
            self._fn = dict(terms={k: lam(v) for k, v in t.items()}, G=lam(G), S=lam(self.S), user=lam(self.user(G)),
                            rhs=None if self.rhs is None else lam(self.rhs),
                            fields={k: (lam(e), how) for k, (e, how) in self.fields(G).items()})
        return self._fn

    # ---- numeric side
    def coordinates(self, n):
        out = []
        for (lo, hi, how), N in zip(self.axes, self.shape(n)):
            out.append(np.linspace(lo, hi, N) if how == 'closed' else lo + (hi - lo) * np.arange(N) / N)
        return out

    def metric(self, cs):
        deg = degree_dims(self.coords, self.rank)
        return [np.asarray(c, dtype=np.float64) * (np.pi / 180.0 * self.a if k in deg else 1.0) for k, c in enumerate(cs)]


_VALID = {k.lower(): v[2] for k, v in apps._RESIDUAL.items()}
_VALID.update(stommelmunk=['A4', 'beta', 'R', 'D', 'rho0', 'g', 'Omega', 'Rearth'], geoadjustment=['g', 'Rearth', 'Omega'],
              refstateswm=['M0', 'C0', 'g', 'Rearth', 'Omega'])


def block(shape):
    """The undefined block of the masked variants: interior, a few points wide in every direction."""
    return tuple(slice(N // 4 + 1, N // 4 + 1 + max(2, N // 6)) for N in shape)


def problem(case, n, mask=None):
    """Everything a run on grid n needs -> dict(F, icbc, S, mParams, iParams, terms {letter: max|term|}, maxG, rhs_err,
    live_expected, shape).  mask: None, 'nan' or 'value' (an undefined block in the forcing)."""
    fn = case.functions()
    shape = case.shape(n)
    cs = case.coordinates(n)
    ms = case.metric(cs)
    h = {ax: 0.0 for ax in _AX}
    grids = {ax: np.zeros((1,) * case.rank) for ax in _AX}
    for k, m in enumerate(ms):
        ax = _AX[case.rank - 1 - k]
        sh = [1] * case.rank
        sh[k] = -1
        grids[ax] = m.reshape(sh)
        h[ax] = float(m[1] - m[0])
    args = (grids[X], grids[Y], grids[Z], h[X], h[Y], h[Z])
    ev = lambda f: np.array(np.broadcast_to(np.asarray(f(*args), dtype=np.float64), shape))
    S = ev(fn['S'])
    G = ev(fn['G'])
    Fu = ev(fn['user'])
    tmax = {k: float(np.abs(ev(f)).max()) for k, f in fn['terms'].items()}
    rhs_err = 0.0 if fn['rhs'] is None else float(np.abs(ev(fn['rhs']) - G).max() / np.abs(G).max())
    mP = dict(case.mParams)
    for k, (f, how) in fn['fields'].items():
        v = ev(f)
        if how == 'vec0':
            v = v[(slice(None),) + (0,) * (case.rank - 1)]
        elif how == 'col0':
            v = v[(slice(None),) + (slice(0, 1),) * (case.rank - 1)]
        mP[k] = np.ascontiguousarray(v)
    undef = -32767.0 if mask == 'value' else np.nan
    inner = np.ones(shape, dtype=bool)
    for k, BC in enumerate(case.BCs):
        if BC != 'periodic':
            sl = [slice(None)] * case.rank
            for e in (0, -1):
                sl[k] = e
                inner[tuple(sl)] = False
    if case.kind == 'bih2d':                       # the radius-2 stencil keeps two rings; the second ring is handed over
        ring = np.zeros(shape, dtype=bool)         # as undefined forcing, so that icbc supplies its value too
        for k, BC in enumerate(case.BCs):
            if BC != 'periodic':
                sl = [slice(None)] * case.rank
                for e in (1, -2):
                    sl[k] = e
                    ring[tuple(sl)] = True
        Fu[ring] = undef
        inner &= ~ring
    if mask is not None:
        Fu[block(shape)] = undef
        inner[block(shape)] = False
    coords = dict(zip(case.dims, cs))
    F = Field(Fu, case.dims, coords)
    icbc = Field(S.copy(), case.dims, coords)
    iP = {'BCs': list(case.BCs), 'undef': undef, 'printInfo': False}
    return dict(F=F, icbc=icbc, S=S, G=G, mParams=mP, iParams=iP, terms=tmax, maxG=float(np.abs(G).max()), rhs_err=rhs_err,
                live=inner, live_expected=int(inner.sum()), shape=shape, h=h, metric=ms)


def front_state(case, p):
    """What apps.residual / apps._template build before the kernels run -> (coeffs, maskF, initS, iParams merged)."""
    iP = apps._update(apps.default_iParams, p['iParams'])
    mP = apps._update(apps.default_mParams, p['mParams'], case.valid)
    maskF, initS, coeffs = getattr(apps, case.builder)(p['F'], list(case.dims), case.coords, mP, iP, p['icbc'])
    cd = [maskF[dm] for dm in case.dims]
    if case.rank == 1:
        ps = apps._cal_params1D(cd[0], case.coords, Rearth=mP['Rearth'], name=case.dims[0])
    elif case.rank == 2:
        ps = apps._cal_params2D(cd[0], cd[1], case.coords, Rearth=mP['Rearth'])
    else:
        ps = apps._cal_params3D(cd[0], cd[1], cd[2], case.coords, Rearth=mP['Rearth'])
    return coeffs, maskF, initS, apps._update(ps, iP)


def model_norms(case, p):
    """[n_live, mean|R|, max|R|, max|F|] of the manufactured S by tests/resid_model.py on the builder's own output."""
    import resid_model
    coeffs, maskF, initS, iP = front_state(case, p)
    kind = case.kind
    sc = {s: float(iP[forms.IPARAM.get(s, s)]) for s in forms.FORMS[kind].scalars
          if not s.startswith('BC') and s not in ('undef', 'optArg', 'xc', 'yc', 'zc')}
    cs = []
    for k, c in enumerate(coeffs):
        v = np.broadcast_to(np.asarray(c.values if hasattr(c, 'values') else c, dtype=np.float64), maskF.shape)
        null = k == 1 and forms.FORMS[kind].null_B and all(s == 0 for s in v.strides) and v.flat[0] == 0.0
        cs.append(None if null else np.array(v))
    cs.append(np.asarray(maskF.values, dtype=np.float64))
    state = apps._solver_state(p['S'], maskF.values, initS.values)
    R, live = resid_model.residual(kind, state, cs, sc, iP['BCs'][-1] == 'periodic', UNDEF)
    return resid_model.norms(R, cs[-1], live)


def oracle_problem(case, p):
    """The positional problem dict of tests/util.py (run_oracle / run_hip_*) out of the front end's state."""
    coeffs, maskF, initS, iP = front_state(case, p)
    q = forms.from_iparams(case.kind, iP, UNDEF)
    full = lambda c: np.ascontiguousarray(np.broadcast_to(np.asarray(c.values if hasattr(c, 'values') else c,
                                                                     dtype=np.float64), maskF.shape))
    q['coefs'] = [full(c) for c in coeffs] + [np.asarray(maskF.values, dtype=np.float64)]
    q['S0'] = np.array(initS.values, dtype=np.float64)
    return q, iP


# ====================================================================================================== the table
A_E = apps.default_mParams['Rearth']
OM = apps.default_mParams['Omega']
GR = apps.default_mParams['g']
R2D = 180 / PI

_n1 = lambda n: (n + 1, 2 * n)                     # odd rows, even columns
_n2 = lambda n: (2 * n, n + 1)                     # even rows, odd columns
_n3 = lambda n: (n // 2 + 1, n + 1, 2 * n)
_LL = lambda lo, hi: [(lo, hi, 'closed'), (0.0, 360.0, 'open')]
_LLF = lambda lo, hi: [(lo, hi, 'closed'), (0.0, 180.0, 'open')]
_PER = ['fixed', 'periodic']
_FIX = ['fixed', 'fixed']


def _sll(a, m1=2, l1=3, m2=1, l2=2):
    """Two harmonics on the sphere, 2 pi a periodic in x, non-zero on the latitude boundaries."""
    return sp.sin(m1 * X / a + sp.Rational(2, 5)) * sp.cos(l1 * Y / a) + sp.Rational(3, 5) * sp.cos(m2 * X / a) * sp.sin(l2 * Y / a + sp.Rational(3, 10))


def _sxy(Lx, Ly, x=X, y=Y):
    """Two harmonics on a box, periodic over Lx, non-zero on every boundary."""
    return sp.sin(2 * PI * x / Lx + sp.Rational(2, 5)) * sp.cos(sp.Rational(3, 2) * PI * y / Ly + sp.Rational(1, 5)) + \
        sp.Rational(3, 5) * sp.cos(2 * PI * x / Lx) * sp.sin(PI * y / Ly + sp.Rational(3, 10))


def _gm(coords, a, eps, Phi, f0, beta, test=False, arons=False):
    """The Gill-Matsuno family: c1 = eps / (eps^2 + f^2), c2 = f / (eps^2 + f^2)."""
    if coords == 'lat-lon':
        phi = Y / a
        f = 2 * OM * sp.sin(phi)
        cos = sp.cos(phi)
    else:
        f = f0 + beta * Y
        cos = sp.Integer(1)
        phi = None
    c1, c2 = eps / (eps ** 2 + f ** 2), f / (eps ** 2 + f ** 2)
    if test:                                          # flux form, multiplied through by cos(phi)
        return {'A': (c1 * Phi * cos, 'half'), 'B': (-c2 * Phi, 'half'), 'C': (c2 * Phi, 'half'), 'D': (c1 * Phi / cos, 'half'),
                'E': (-eps * cos, 'half')}, cos
    tan = sp.tan(phi) / a if phi is not None else 0
    co = {'A': (c1 * Phi, 'half'), 'C': (c1 * Phi / cos ** 2, 'half'), 'D': (Phi * (d(c1, Y) + c1 * tan), 'half'),
          'E': (-Phi * d(c2, Y) / cos, 'half')}
    if not arons:
        co['F'] = (sp.Float(-eps), 'half')
    return co, cos


def _build():
    C = {}

    def add(case, variant=None):
        C[(case.app, case.coords) + ((variant,) if variant else ())] = case

    a = A_E
    phi = Y / a
    cos, sin = sp.cos(phi), sp.sin(phi)
    fs = 2 * OM * sin                                # Coriolis parameter on the sphere
    Lb = 1.0e6                                       # the cartesian box
    box = [(0.0, Lb, 'closed'), (0.0, Lb, 'open')]
    boxc = [(0.0, Lb, 'open'), (0.0, Lb, 'closed')]
    Sb = _sxy(Lb, Lb)

    # ---------------------------------------------------------------- Poisson: the Laplacian in four branches
    add(Case('poisson', 'lat-lon', ('lat', 'lon'), _LL(-60, 60), _PER, {}, {'A': (cos, 'half'), 'C': (1 / cos, 'half')},
             _sll(a), lambda G: G / cos, _n1))
    a1 = 6.0e3                                       # a small planet puts the latitude span next to a 10 km column
    add(Case('poisson', 'z-lat', ('lev', 'lat'), [(0.0, 8.0e3, 'open'), (-50.0, 50.0, 'closed')], _FIX, {'Rearth': a1},
             {'A': (1, 'half'), 'C': (1, 'half')}, _sxy(1.0e4, 8.0e3), lambda G: G / sp.cos(X / a1), _n2))
    add(Case('poisson', 'z-lon', ('lev', 'lon'), [(0.0, 8.0e3, 'closed'), (0.0, 360.0, 'open')], _PER, {'Rearth': a1},
             {'A': (1, 'half'), 'C': (1, 'half')}, _sxy(2 * PI * a1, 8.0e3), lambda G: G, _n1))
    add(Case('poisson', 'cartesian', ('y', 'x'), boxc, _FIX, {}, {'A': (1, 'half'), 'C': (1, 'half')}, Sb, lambda G: G, _n2))

    # ---------------------------------------------------------------- Gill-Matsuno family
    gmP = {'epsilon': 5e-5, 'Phi': 1e5}
    for app, kw, mp in (('gillmatsuno', {}, gmP), ('gillmatsuno_test', {'test': True}, gmP),
                        ('stommelarons', {'arons': True}, {'epsilon': 5e-5})):
        Phi = mp.get('Phi', 1.0)
        co, cs_ = _gm('lat-lon', a, 5e-5, Phi, 0, 0, **kw)
        test = bool(kw.get('test'))                 # (cross terms: fixed x -- the kernels' west column)
        add(Case(app, 'lat-lon', ('lat', 'lon'), _LLF(-60, 60) if test else _LL(-60, 60), _FIX if test else _PER, dict(mp), co,
                 _sll(a), (lambda G, cs_=cs_, t=test: G / cs_ if t else G), _n1))
        Phic = Phi * 1e-3 if 'Phi' in mp else 1.0
        mpc = dict(mp, f0=3e-5, beta=2e-10)
        if 'Phi' in mp:
            mpc['Phi'] = Phic
        co, _ = _gm('cartesian', a, 5e-5, Phic, 3e-5, 2e-10, **kw)
        add(Case(app, 'cartesian', ('y', 'x'), box, _FIX if test else _PER, mpc, co, Sb * (1 + Y / (2 * Lb)), lambda G: G, _n1))

    # ---------------------------------------------------------------- Stommel
    R, D, rho0 = 5e-3, 100.0, 1027.0
    add(Case('stommel', 'lat-lon', ('lat', 'lon'), _LL(-60, 60), _PER, {'R': R, 'D': D},
             {'A': (-R / D, 'half'), 'C': (-R / D / cos ** 2, 'half'), 'E': (-2 * OM / a, 'half')}, _sll(a),
             lambda G: -G * D * rho0, _n1, note='the reference drops the metric terms of the spherical Laplacian and uses 2 Omega / a for beta at every latitude'))
    Rc, beta = 3e-4, 2e-11
    add(Case('stommel', 'cartesian', ('y', 'x'), boxc, _FIX, {'R': Rc, 'D': D, 'beta': beta},
             {'A': (-Rc / D, 'half'), 'C': (-Rc / D, 'half'), 'E': (-beta, 'half')}, Sb, lambda G: -G * D * rho0, _n2))
    Rf = Rc * (1 + sp.Rational(3, 10) * sp.sin(2 * PI * X / Lb) * sp.cos(PI * Y / Lb))
    add(Case('stommel', 'cartesian', ('y', 'x'), boxc, _FIX, {'D': D, 'beta': beta},
             {'A': (-Rf / D, 'half'), 'C': (-Rf / D, 'half'), 'E': (-beta, 'half')}, Sb, lambda G: -G * D * rho0, _n2,
             fields=lambda G: {'R': (Rf, 'full')}), 'Rfield')
    add(Case('stommel_test', 'lat-lon', ('lat', 'lon'), _LLF(-60, 60), _FIX, {'R': R, 'D': D},
             {'A': (-R / D * cos, 'half'), 'B': (-fs, 'half'), 'C': (fs, 'half'), 'D': (-R / D / cos, 'half')}, _sll(a),
             lambda G: -G * D * rho0 / cos, _n1))
    fd = apps.default_mParams['f0'] + beta * Y       # (invert_Stommel_test does not accept 'f0': the builder reads the default)
    add(Case('stommel_test', 'cartesian', ('y', 'x'), boxc, _FIX, {'R': Rc, 'D': D, 'beta': beta},
             {'A': (-Rc / D, 'half'), 'B': (-fd, 'half'), 'C': (fd, 'half'), 'D': (-Rc / D, 'half')}, Sb,
             lambda G: -G * D * rho0, _n2))

    # ---------------------------------------------------------------- Stommel-Munk (biharmonic)
    A4 = 5e8
    Rm = 5e-3
    add(Case('stommelmunk', 'lat-lon', ('lat', 'lon'), _LL(-60, 60), _PER, {'A4': A4, 'R': Rm, 'D': D},
             {'A': (A4, 'half'), 'C': (A4 / cos ** 2, 'half'), 'D': (-Rm / D, 'half'), 'F': (-Rm / D / cos ** 2, 'half'),
              'H': (-2 * OM / a, 'half')}, _sll(a), lambda G: -G * D * rho0, lambda n: (n + 1, 3 * n),   # (periodic one-pass kernel: xc % 3 == 0)
             note='as Stommel: no metric terms; the biharmonic coefficient of x is A4 / cos^2, not A4 / cos^4'))
    A4c = 8e4
    add(Case('stommelmunk', 'cartesian', ('y', 'x'), [(0.0, Lb, 'closed'), (0.0, Lb, 'closed')], _FIX,
             {'A4': A4c, 'R': Rc, 'D': D, 'beta': beta},
             {'A': (A4c, 'half'), 'C': (A4c, 'half'), 'D': (-Rc / D, 'half'), 'F': (-Rc / D, 'half'), 'H': (-beta, 'half')}, Sb,
             lambda G: -G * D * rho0, lambda n: (n + 1, 2 * n + 1)))

    # ---------------------------------------------------------------- Bretherton-Haidvogel and Fofonoff (std2dt)
    f0 = 1e-4
    fc = f0 + beta * Y
    lam = 5e-15
    add(Case('brethertonhaidvogel', 'lat-lon', ('lat', 'lon'), _LL(10, 70), _PER, {'lambda': lam, 'D': D},
             {'A': (cos, 'half'), 'D': (1 / cos, 'half'), 'E': (-lam * D * cos, 'half')}, _sll(a),
             lambda G: -G * D / (fs * cos), _n1))
    lamc = 1e-12
    add(Case('brethertonhaidvogel', 'cartesian', ('y', 'x'), boxc, _FIX, {'lambda': lamc, 'D': D, 'f0': f0, 'beta': beta},
             {'A': (1, 'half'), 'D': (1, 'half'), 'E': (-lamc * D, 'half')}, Sb, lambda G: -G * D / fc, _n2))
    # Fofonoff: the builder dictates the right-hand side c1 - f, so S is a particular solution plus solutions of the
    # homogeneous equation.  Sphere: c0 = -6 / a^2 makes the degree-2 spherical harmonics homogeneous.
    c0, c1 = -6 / a ** 2, 3e-5
    Sf = -c1 / c0 + 2 * OM * sin / (2 / a ** 2 + c0) + 2e9 * (sin * cos * sp.cos(X / a + sp.Rational(2, 5)) + sp.Rational(3, 5) * cos ** 2 * sp.sin(2 * X / a)
                                                             + sp.Rational(1, 2) * (3 * sin ** 2 - 1))
    add(Case('fofonoff', 'lat-lon', ('lat', 'lon'), _LL(-60, 60), _PER, {'c0': c0, 'c1': c1},
             {'A': (cos, 'half'), 'D': (1 / cos, 'half'), 'E': (-c0 * cos, 'half')}, Sf, lambda G: 1 + 0 * X, _n1,
             rhs=(c1 - fs) * cos))
    # box: c0 > 0 (a definite operator, so the sweeps converge); sin(l x) cosh(k y) with k^2 = l^2 + c0 is homogeneous
    c0c, c1c = 2e-12, 5e-5
    l1, l2 = np.pi / Lb, 0.5 * np.pi / Lb
    k1, k2 = float(np.sqrt(l1 ** 2 + c0c)), float(np.sqrt(l2 ** 2 + c0c))
    yc_ = Y - Lb / 2
    Sfc = -(c1c - f0 - beta * Y) / c0c + 2e7 * (sp.sin(l1 * X + sp.Rational(2, 5)) * sp.cosh(k1 * yc_) / np.cosh(k1 * Lb / 2)
                                                + sp.Rational(3, 5) * sp.cos(l2 * X) * sp.sinh(k2 * yc_) / np.sinh(k2 * Lb / 2))
    add(Case('fofonoff', 'cartesian', ('y', 'x'), box, _FIX, {'c0': c0c, 'c1': c1c, 'f0': f0, 'beta': beta},
             {'A': (1, 'half'), 'D': (1, 'half'), 'E': (-c0c, 'half')}, Sfc, lambda G: 1 + 0 * X, _n1, rhs=c1c - f0 - beta * Y))   # (rows closed: cosh grows towards the edge)

    # ---------------------------------------------------------------- geostrophic (|f| >= 2e-5 everywhere: no inflation)
    add(Case('geostrophic', 'lat-lon', ('lat', 'lon'), _LL(15, 65), _PER, {}, {'A': (fs * cos, 'half'), 'C': (fs / cos, 'half')},
             _sll(a), lambda G: G / cos, _n1))
    add(Case('geostrophic', 'cartesian', ('y', 'x'), boxc, _FIX, {'f0': 3e-5, 'beta': 1e-10},
             {'A': (3e-5 + 1e-10 * Y, 'half'), 'C': (3e-5 + 1e-10 * Y, 'half')}, Sb, lambda G: G, _n2))

    # ---------------------------------------------------------------- vertical planes: y is the level, x = a * latitude
    a0 = 1.0                                         # Rearth = 1: x is the latitude in radians
    zl = [(0.0, 1.0, 'open'), (20.0, 70.0, 'closed')]
    Sz = _sxy(1.0, 1.0)
    N2 = 1e-4 * (1 + Y / 2)                          # a stratification profile over the level
    add(Case('pv2d', 'z-lat', ('lev', 'lat'), zl, _FIX, {'Rearth': a0, 'f0': 1e-2}, {'A': (1e-4 / N2, 'grid'), 'C': (1, 'half')},
             Sz, lambda G: G, _n2, fields=lambda G: {'N2': (N2, 'col0')},
             note='both branches use the constant f0 where the docstring has f(lat)'))
    add(Case('pv2d', 'cartesian', ('z', 'y'), [(0.0, 1.0, 'closed'), (0.0, 1.0, 'open')], _FIX, {'f0': 1e-2},
             {'A': (1e-4 / N2, 'grid'), 'C': (1, 'half')}, Sz, lambda G: G, _n1, fields=lambda G: {'N2': (N2, 'col0')}))
    Ae = 1 + sp.Rational(3, 10) * sp.sin(2 * Y + X)
    Be = sp.Rational(3, 10) * sp.cos(X - Y)
    Ce = sp.Rational(3, 2) + sp.Rational(2, 5) * sp.cos(2 * X) * sp.sin(Y + 1)
    eco = {'A': (Ae, 'grid'), 'B': (Be, 'half'), 'C': (Ce, 'grid')}
    efl = lambda G: {'A': (Ae, 'full'), 'B': (Be, 'full'), 'C': (Ce, 'full')}
    add(Case('eliassen', 'z-lat', ('lev', 'lat'), zl, _FIX, {'Rearth': a0}, eco, Sz, lambda G: G, _n2, fields=efl))
    add(Case('eliassen', 'cartesian', ('z', 'y'), [(0.0, 1.0, 'closed'), (0.0, 1.0, 'open')], _FIX, {}, eco, Sz, lambda G: G,
             _n1, fields=efl))
    # RefState: C = Gamma g / (Q x1) holds the forcing itself, so Gamma is manufactured from the C wanted
    cw = sp.Rational(3, 10) * (1 + sp.Rational(1, 5) * sp.sin(2 * X + Y))
    Sr = 4 * Y ** 2 + sp.Rational(3, 10) * _sxy(1.0, 1.0)
    add(Case('refstate', 'z-lat', ('lev', 'lat'), zl, _FIX, {'Rearth': a0}, {'A': (sp.sin(X / a0), 'grid'), 'C': (cw, 'grid')}, Sr,
             lambda G: G, _n2, fields=lambda G: {'Gamma': (cw * G * (X / a0 * R2D) / GR, 'full')},
             note='C divides by the latitude in degrees'))
    ang0 = apps.default_mParams['ang0']              # (the entry point accepts 'Ang0' but the builder reads the default 'ang0')
    rr = [(0.0, 50.0, 'closed'), (50.0, 100.0, 'open')]
    cr = sp.Rational(3, 10) * (1 + sp.Rational(1, 5) * sp.sin((2 * X + Y) / 50))
    Srr = 4 * (Y / 50) ** 2 + sp.Rational(3, 10) * _sxy(50.0, 50.0)
    add(Case('refstate', 'cartesian', ('z', 'r'), rr, _FIX, {}, {'A': (2 * ang0 / X ** 3, 'grid'), 'C': (cr, 'grid')}, Srr,
             lambda G: G, _n1, fields=lambda G: {'Gamma': (cr * G * X / GR, 'full')}))

    # ---------------------------------------------------------------- 3-D
    lev = (1.0e5, 1.0e4, 'closed')                   # pressure, descending: a negative level spacing
    n2p = 2e-4 * (1 + (Z - 1e4) / 1.8e5)
    S3 = _sll(a) * sp.cos(PI * (Z - 1e4) / 9e4 + sp.Rational(1, 5)) + sp.Rational(1, 2) * sp.sin(X / a) * sp.cos(2 * Y / a) * sp.sin(2 * PI * Z / 9e4)
    add(Case('omega', 'lat-lon', ('lev', 'lat', 'lon'), [lev, (20.0, 70.0, 'closed'), (0.0, 360.0, 'open')],
             ['fixed', 'fixed', 'periodic'], {}, {'A': (fs ** 2 * cos, 'half'), 'B': (n2p * cos, 'half'), 'C': (n2p / cos, 'half')}, S3,
             lambda G: G / cos, _n3, fields=lambda G: {'N2': (n2p, 'vec0')}))
    L3 = 4.0e6
    S3c = _sxy(L3, L3) * sp.cos(PI * (Z - 1e4) / 9e4 + sp.Rational(1, 5)) + sp.Rational(1, 2) * sp.sin(2 * PI * X / L3) * sp.sin(2 * PI * Z / 9e4 + sp.Rational(1, 2))
    f3 = 5e-5 + 5e-11 * Y
    box3 = [lev, (0.0, L3, 'closed'), (0.0, L3, 'open')]
    add(Case('omega', 'cartesian', ('lev', 'y', 'x'), box3, ['fixed', 'fixed', 'fixed'], {'N2': 1e-5, 'f0': 5e-5, 'beta': 5e-11},
             {'A': (f3 ** 2, 'half'), 'B': (1e-5, 'half'), 'C': (1e-5, 'half')}, S3c, lambda G: G, _n3))
    eps3, k3 = 5e-5, 1e-8
    dep = (0.0, -4000.0, 'closed')
    n2o = 1e-5 * (1 - Z / 3000)
    c3 = k3 / n2o
    c1s, c2s = eps3 / (eps3 ** 2 + fs ** 2), fs / (eps3 ** 2 + fs ** 2)
    So = _sll(a) * sp.cos(PI * Z / 4000 + sp.Rational(1, 5)) + sp.Rational(1, 2) * sp.sin(X / a) * sp.cos(2 * Y / a) * sp.sin(2 * PI * Z / 4000)
    add(Case('3docean', 'lat-lon', ('lev', 'lat', 'lon'), [dep, (15.0, 65.0, 'closed'), (0.0, 360.0, 'open')],
             ['fixed', 'fixed', 'periodic'], {'epsilon': eps3, 'k': k3},
             {'A': (c3, 'half'), 'B': (c1s, 'half'), 'C': (c1s / cos ** 2, 'half'), 'D': (d(c3, Z), 'half'),
              'E': (d(c1s, Y) - c1s * sp.tan(phi) / a, 'half'), 'F': (-d(c2s, Y) / cos, 'half')}, So, lambda G: G, _n3,
             fields=lambda G: {'N2': (n2o, 'vec0')},
             note='the metric term of E is -c1 tan(phi) / a here and +c1 tan(phi) / a in Gill-Matsuno'))
    c1c_, c2c_ = eps3 / (eps3 ** 2 + f3 ** 2), f3 / (eps3 ** 2 + f3 ** 2)
    Soc = _sxy(L3, L3) * sp.cos(PI * Z / 4000 + sp.Rational(1, 5)) + sp.Rational(1, 2) * sp.sin(2 * PI * X / L3) * sp.sin(2 * PI * Z / 4000 + sp.Rational(1, 2))
    add(Case('3docean', 'cartesian', ('lev', 'y', 'x'), [dep, (0.0, L3, 'closed'), (0.0, L3, 'open')], ['fixed', 'fixed', 'fixed'],
             {'epsilon': eps3, 'k': k3 * 10, 'f0': 5e-5, 'beta': 5e-11},
             {'A': (10 * c3, 'half'), 'B': (c1c_, 'half'), 'C': (c1c_, 'half'), 'D': (10 * d(c3, Z), 'half'), 'E': (d(c1c_, Y), 'half'),
              'F': (-d(c2c_, Y), 'half')}, Soc, lambda G: G, _n3, fields=lambda G: {'N2': (n2o, 'vec0')}))

    # ---------------------------------------------------------------- 1-D (x is the only dim: a * latitude)
    ag = 6.0e5                                       # a small planet: the flux term weighs in beside f cos / g
    ph1 = X / ag
    f1 = 2 * OM * sp.sin(ph1)
    Ag = sp.cos(ph1) / f1
    Sg = 1000 + 20 * (sp.sin(5 * ph1) + sp.Rational(1, 2) * sp.cos(3 * ph1 + sp.Rational(1, 5)))
    Fg = -f1 * sp.cos(ph1) / GR                      # the right-hand side the builder dictates
    Bg = (Fg - d(Ag * d(Sg, X), X)) / Sg             # ... so B, and with it h0 = -f cos / (g B), follows from S
    add(Case('geoadjustment', 'lat', ('lat',), [(20.0, 70.0, 'closed')], ['fixed'], {'Rearth': ag}, {'A': (Ag, 'half'), 'B': (Bg, 'half')},
             Sg, lambda G: -f1 * sp.cos(ph1) / GR / Bg, lambda n: (4 * n + 1,), rhs=Fg))
    C0 = 1.0e8
    M0 = 5.0e13 * (1 + sp.Rational(1, 5) * sp.sin(4 * ph1))
    asin_, acos_ = ag * sp.sin(ph1), ag * sp.cos(ph1)
    Fs = -(asin_ * C0 ** 2 / (2 * PI * GR * acos_ ** 3)) + 2 * PI * OM ** 2 * asin_ * acos_ / GR - d(d(M0, X) / sp.cos(ph1), X)
    Ss = 2.0e14 + 1.0e13 * (sp.sin(5 * ph1) + sp.Rational(1, 2) * sp.cos(3 * ph1 + sp.Rational(1, 5)))
    Bs = (Fs - d(d(Ss, X) / sp.cos(ph1), X)) / Ss
    add(Case('refstateswm', 'lat', ('lat',), [(20.0, 70.0, 'closed')], ['fixed'], {'Rearth': ag, 'C0': C0},
             {'A': (1 / sp.cos(ph1), 'half'), 'B': (Bs, 'half')}, Ss, lambda G: -Bs * PI * GR * acos_ ** 3 / (C0 * asin_),
             lambda n: (4 * n + 1,), rhs=Fs, fields=lambda G: {'M0': (M0, 'vec0')}))
    return C


CASES = _build()
RESIDUAL_CASES = {k: c for k, c in CASES.items() if c.app in apps._RESIDUAL}
SOLVE_CASES = {k: c for k, c in CASES.items() if c.app in NO_RESIDUAL}
# the coordinate branches each builder accepts (the `elif` chains of apps._coeffs_*)
BRANCHES = {'poisson': ('lat-lon', 'z-lat', 'z-lon', 'cartesian'), 'pv2d': ('z-lat', 'cartesian'), 'eliassen': ('z-lat', 'cartesian'),
            'refstate': ('z-lat', 'cartesian'), 'geoadjustment': ('lat',), 'refstateswm': ('lat',)}
# one masked variant per form: (table key, how the undefined block is written)
MASKED = {'std2d': (('poisson', 'lat-lon'), 'nan'), 'gen2d': (('stommel', 'cartesian'), 'value'),
          'std2dt': (('brethertonhaidvogel', 'cartesian'), 'nan'), 'std3d': (('omega', 'lat-lon'), 'value'),
          'gen3d': (('3docean', 'cartesian'), 'nan')}
# ... and of the biharmonic form, which has no residual: the block is an inner boundary of the solve.  (The 1-D form has
# none: both 1-D builders, like the reference's, write a right-hand side without the forcing's mask -- `zero - f cos / g`
# with zero = maskF - maskF -- so an undefined point of their input is not an undefined point of the solve.)
MASKED_SOLVE = {'bih2d': (('stommelmunk', 'cartesian'), 'value')}
GRIDS = (16, 32, 64)
FIRST, LAST, WEIGHT = 3.0, 3.5, 0.05              # e(n)/e(2n) at the first and the last refinement; a term's least weight


def check_weights(case, p):
    """Every term of L(S) weighs at least 5 % of max|G| on this grid (a term below that could change sign unnoticed), and
    a dictated right-hand side is met."""
    for k, v in p['terms'].items():
        assert v >= WEIGHT * p['maxG'], (case.app, case.coords, k, v / p['maxG'])
    assert p['rhs_err'] <= 1e-9, (case.app, case.coords, p['rhs_err'])
