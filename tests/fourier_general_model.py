"""The direct Fourier solve of the 2-D general form for periodic x, restated in numpy ("General form"): the
arithmetic of k_fourier_cfactor, k_fourier_csubst and k_fourier_gcheck of xinvert_amd/csrc/xinv_cfourier.h, operation by
operation in float64 (complex arithmetic written out in real operations, as the kernels have it); the transform and the
lambda table are those of tests/fourier_model.py.

    sigma(n)                   -> [K] sin(2 pi k / n), rounded once from long double; 0 at k = 0 and, for even n, at n / 2
    factor(c, sc, lam, sig)    -> (lo, up [nb, yc], ir, ii, gr, gi [nb, yc, K]): inv_j and gamma_j of every wavenumber
    solve(S0, c, G, sc, undef) -> (S, flags [nbatch, 3]); raises when a point the solve reads is undef
c = (A, C, D, E, Fc), one value per row: [yc] (shared) or [nbatch, yc]; sc = (delx, delxSqr, ratio, ratioSqr).  All leave
their inputs alone.
"""
import numpy as np

import fourier_model as M


def problem(yc, xc, nb, shared, seed):
    """Random, dominant coefficients: A, C in [0.5, 2]; |D ratio delx / 2| <= 0.9 A ratioSqr; E in [-3, 3] (|Im di|
    comparable to |Re di|); Fc in [-1, 0]; non-zero boundary rows.  -> dict(S0, G [nb, yc, xc], c = [A, C, D, E, Fc] as
    [yc] (shared) or [nb, yc], sc = (delx, delxSqr, ratio, ratioSqr), ...)."""
    rng = np.random.default_rng(seed)
    delx, dely = 1.1, 1.3
    ratio = delx / dely
    sc = (delx, delx * delx, ratio, ratio * ratio)
    A, C = rng.uniform(0.5, 2.0, (nb, yc)), rng.uniform(0.5, 2.0, (nb, yc))
    D = rng.uniform(-0.9, 0.9, (nb, yc)) * A * sc[3] / (ratio * delx / 2)
    E, Fc = rng.uniform(-3.0, 3.0, (nb, yc)), rng.uniform(-1.0, 0.0, (nb, yc))
    c = [A, C, D, E, Fc]
    if shared:
        c = [x[0].copy() for x in c]
    G = rng.standard_normal((nb, yc, xc))
    S0 = rng.standard_normal((nb, yc, xc)) * np.abs(G).max() * sc[1]
    return dict(S0=S0, G=G, c=c, sc=sc, nb=nb, yc=yc, xc=xc)


def gill_matsuno(ny, nx, members=1, seed=None):
    """xinvert_amd.synthetic.gill_matsuno in the same shape: coefficients shared, one value per row (rows 0 and yc-1, the
    poles, are not read); -> also `full`, the problem dict of tests/util.py for member 0."""
    from xinvert_amd import synthetic
    p = synthetic.gill_matsuno(ny, nx, members) if seed is None else synthetic.gill_matsuno(ny, nx, members, seed)
    A, B, C, D, E, Fc, G = p['coefs']
    assert not np.any(np.asarray(B)[1:-1] != 0)
    c = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (ny, nx))[:, 0]) for x in (A, C, D, E, Fc)]
    G = np.ascontiguousarray(G, dtype=np.float64).reshape(members, ny, nx)
    S0 = np.ascontiguousarray(p['S0'], dtype=np.float64).reshape(members, ny, nx)
    return dict(S0=S0, G=G, c=c, sc=(p['delx'], p['delxSqr'], p['ratio'], p['ratioSqr']), nb=members, yc=ny, xc=nx,
                full=synthetic.member(p, 0))


def sigma(n):
    ld = np.longdouble
    pi = ld('3.14159265358979323846264338327950288')
    k = np.arange(n // 2 + 1, dtype=ld)
    s = np.sin(ld(2) * pi * k / ld(n)).astype(np.float64)
    s[0] = 0.0
    if n % 2 == 0:
        s[n // 2] = 0.0
    return s


def rows(c, nb, yc):
    return [np.broadcast_to(np.asarray(x, dtype=np.float64), (nb, yc)) for x in c]


def undef_count(S0, c, G, undef):
    """[nbatch]: how many of the points the solve reads hold `undef` (k_fourier_gcheck)."""
    nb, yc = S0.shape[:2]
    cnt = (G[:, 1:-1] == undef).sum(axis=(1, 2)) + (S0[:, 0] == undef).sum(axis=1) + (S0[:, -1] == undef).sum(axis=1)
    for x in rows(c, nb, yc):
        cnt = cnt + (x[:, 1:-1] == undef).sum(axis=1)
    return cnt


def factor(c, sc, lam, sig):
    """k_fourier_cfactor: c as [nb, yc] each.  Rows 0 and yc-1 stay zero."""
    A, C, D, E, Fc = c
    delx, dx2, ratio, rs = sc
    nb, yc = A.shape
    K = lam.size
    hd = delx * 0.5
    lo, up = np.zeros((nb, yc)), np.zeros((nb, yc))
    ir, ii, gr, gi = (np.zeros((nb, yc, K)) for _ in range(4))
    pgr, pgi = np.zeros((nb, K)), np.zeros((nb, K))
    with np.errstate(all='ignore'):
        for j in range(1, yc - 1):
            ars = A[:, j] * rs
            dh = (D[:, j] * ratio) * hd
            l, u = ars - dh, ars + dh
            dr = (-(2.0 * ars[:, None] + C[:, j, None] * lam)) + (Fc[:, j] * dx2)[:, None]
            di = (E[:, j] * delx)[:, None] * sig
            if j == 1:
                er, ei = dr, di
            else:
                er, ei = dr - l[:, None] * pgr, di - l[:, None] * pgi
            q = 1.0 / (er * er + ei * ei)
            ir[:, j], ii[:, j] = er * q, -(ei * q)
            pgr, pgi = u[:, None] * ir[:, j], u[:, None] * ii[:, j]
            gr[:, j], gi[:, j] = pgr, pgi
            lo[:, j], up[:, j] = l, u
    return lo, up, ir, ii, gr, gi


def solve(S0, c, G, sc, undef=-9.99e8):
    """-> (S, flags) as xinv_fourier_general_2d_f64_dev returns them; S0, G [nbatch, yc, xc] or [yc, xc]."""
    one = np.ndim(S0) == 2
    S0 = np.array(S0, dtype=np.float64, copy=True).reshape((-1,) + np.shape(S0)[-2:])
    G = np.asarray(G, dtype=np.float64).reshape(S0.shape)
    nb, yc, xc = S0.shape
    if yc < 3 or xc < 3:
        raise ValueError('every core dimension needs at least 3 points')
    M.factor(xc)
    c = rows(c, nb, yc)
    bad = undef_count(S0, c, G, undef)
    if bad.any():
        raise ValueError('member %d holds undef at %d of the points the solve reads' % (int(np.argmax(bad > 0)), bad[bad > 0][0]))
    _, lam = M.tables(xc)
    lo, up, ir, ii, gr, gi = factor(c, sc, lam, sigma(xc))
    spec = np.zeros((nb, yc, xc // 2 + 1), dtype=np.complex128)
    spec[:, 1:-1] = M.rfft_rows(G[:, 1:-1], sc[1])
    spec[:, [0, yc - 1]] = M.rfft_rows(S0[:, [0, yc - 1]])
    with np.errstate(all='ignore'):
        pr, pi = spec[:, 0].real.copy(), spec[:, 0].imag.copy()
        rho_r, rho_i = np.zeros(spec.shape), np.zeros(spec.shape)
        for j in range(1, yc - 1):
            tr, ti = spec[:, j].real.copy(), spec[:, j].imag.copy()
            if j == yc - 2:
                u = up[:, j, None]
                tr = tr - u * spec[:, yc - 1].real
                ti = ti - u * spec[:, yc - 1].imag
            l = lo[:, j, None]
            tr = tr - l * pr
            ti = ti - l * pi
            pr, pi = tr * ir[:, j] - ti * ii[:, j], tr * ii[:, j] + ti * ir[:, j]
            rho_r[:, j], rho_i[:, j] = pr, pi
        for j in range(yc - 3, 0, -1):
            xr = rho_r[:, j] - (gr[:, j] * pr - gi[:, j] * pi)
            xi = rho_i[:, j] - (gr[:, j] * pi + gi[:, j] * pr)
            pr, pi = xr, xi
            rho_r[:, j], rho_i[:, j] = pr, pi
        X = rho_r[:, 1:-1] + 1j * rho_i[:, 1:-1]
        S0[:, 1:-1] = M.irfft_rows(X, xc)
    fl = np.zeros((nb, 3))
    fl[:, 0] = (~(np.isfinite(rho_r[:, 1:-1]) & np.isfinite(rho_i[:, 1:-1]))).any(axis=(1, 2))
    return (S0[0], fl[0]) if one else (S0, fl)
