"""The direct Fourier solve of the 2-D standard form for periodic x, restated in numpy: the arithmetic of
k_rowdft, k_fourier_tri and k_fourier_check of xinvert_amd/csrc/xinv_fourier.h, operation by operation in float64 (plain
numpy arithmetic evaluates every binary operation in the order written, without contraction).

    factor(n)                  -> the Stockham passes' radices (4s first, then 2, 3, 5); raises for any other prime factor
    tables(n)                  -> (W [n] complex = exp(-2 pi i t / n), lam [K] = 4 sin^2(pi k / n)), rounded once from long double
    rfft_rows(x), irfft_rows(X, n)   the packed-pair transform: rows 2p and 2p + 1 of the last-but-one axis are one complex transform
    system(A, C, ratioSqr, lam)      -> lo [yc], up [yc], di [yc, K] of the tridiagonal systems (rows 1 .. yc-2 are used)
    solve(S0, A, C, F, delxSqr, ratioSqr, undef) -> (S, flags [nbatch, 3]); raises when a point the solve reads is undef
A and C are one value per row: [yc] (shared) or [nbatch, yc].  All leave their inputs alone.
"""
import numpy as np

MAX_N = 4096                     # XINV_DFT_MAX_N: a ping-pong pair of n complex doubles within 128 KiB of LDS


def factor(n):
    n = int(n)
    if n < 2:
        raise ValueError('a row needs at least 2 points, got %d' % n)
    out, r = [], n
    for q in (4, 2, 3, 5):
        while r % q == 0:
            out.append(q)
            r //= q
    if r != 1:
        f = next((p for p in range(7, int(r ** 0.5) + 1, 2) if r % p == 0), r)
        raise ValueError('the row length %d has the prime factor %d (the transform takes products of 2, 3 and 5)' % (n, f))
    if n > MAX_N:
        raise ValueError("the row length %d is beyond the transform's LDS budget (at most %d points)" % (n, MAX_N))
    return out


def tables(n):
    ld = np.longdouble
    pi = ld('3.14159265358979323846264338327950288')
    t = np.arange(n, dtype=ld)
    ang = ld(2) * pi * t / ld(n)
    W = np.cos(ang).astype(np.float64) + 1j * (-np.sin(ang)).astype(np.float64)
    s = np.sin(pi * np.arange(n // 2 + 1, dtype=ld) / ld(n))
    return W, (ld(4) * s * s).astype(np.float64)


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


S3 = 0.86602540378443864676
C1, C2 = 0.30901699437494742410, -0.80901699437494742410
S1, S2 = 0.95105651629515357212, 0.58778525229247312917


def _mnj(r, i):                                          # times -i
    return i, -r


def _pass(zr, zi, W, R, ns):
    """One Stockham pass of radix R over the last axis (k_rowdft's xinv_dft_pass)."""
    n = zr.shape[-1]
    nb = n // R
    j = np.arange(nb)
    k = j % ns
    j0 = (j // ns) * ns * R + k
    tstep = n // (ns * R)
    v = []
    for r in range(R):
        vr, vi = zr[..., j + r * nb], zi[..., j + r * nb]
        if ns > 1 and r > 0:
            w = W[r * k * tstep]
            vr, vi = _cmul(vr, vi, w.real, w.imag)
        v.append((vr, vi))
    add = lambda a, b: (a[0] + b[0], a[1] + b[1])
    sub = lambda a, b: (a[0] - b[0], a[1] - b[1])
    scl = lambda a, s: (a[0] * s, a[1] * s)
    mnj = lambda a: _mnj(*a)
    if R == 2:
        o = [add(v[0], v[1]), sub(v[0], v[1])]
    elif R == 4:
        a, b, c, d = add(v[0], v[2]), sub(v[0], v[2]), add(v[1], v[3]), mnj(sub(v[1], v[3]))
        o = [add(a, c), add(b, d), sub(a, c), sub(b, d)]
    elif R == 3:
        t, d = add(v[1], v[2]), mnj(scl(sub(v[1], v[2]), S3))
        m = sub(v[0], scl(t, 0.5))
        o = [add(v[0], t), add(m, d), sub(m, d)]
    else:
        a1, b1, a2, b2 = add(v[1], v[4]), sub(v[1], v[4]), add(v[2], v[3]), sub(v[2], v[3])
        m1 = add(v[0], add(scl(a1, C1), scl(a2, C2)))
        m2 = add(v[0], add(scl(a1, C2), scl(a2, C1)))
        d1 = mnj(add(scl(b1, S1), scl(b2, S2)))
        d2 = mnj(sub(scl(b1, S2), scl(b2, S1)))
        o = [add(v[0], add(a1, a2)), add(m1, d1), add(m2, d2), sub(m2, d2), sub(m1, d1)]
    outr, outi = np.empty_like(zr), np.empty_like(zi)
    for r in range(R):
        outr[..., j0 + r * ns], outi[..., j0 + r * ns] = o[r]
    return outr, outi


def _dft(zr, zi, n):
    W, _ = tables(n)
    ns = 1
    for R in factor(n):
        zr, zi = _pass(zr, zi, W, R, ns)
        ns *= R
    return zr, zi


def _pairs(x):
    """[G, rows, w] -> ([G * pairs, w], [G * pairs, w]): the rows of even and of odd index of every group; a missing last
    partner reads 0."""
    G, rows, w = x.shape
    if rows % 2:
        x = np.concatenate([x, np.zeros((G, 1, w), dtype=x.dtype)], axis=1)
    return x[:, 0::2].reshape(-1, w), x[:, 1::2].reshape(-1, w)


def _unpairs(e, o, G, rows):
    out = np.empty((G, 2 * (e.shape[0] // G), e.shape[-1]), dtype=e.dtype)
    out[:, 0::2], out[:, 1::2] = e.reshape(G, -1, e.shape[-1]), o.reshape(G, -1, o.shape[-1])
    return out[:, :rows]


def _groups(x):
    """[..., rows, w] (or one row [w]) -> [G, rows, w]: rows 2p and 2p + 1 of ONE group (member) share a transform."""
    return x.reshape((-1,) + x.shape[-2:]) if x.ndim >= 2 else x.reshape(1, 1, -1)


def rfft_rows(x, scale=1.0):
    """Real [..., rows, n] -> half spectrum [..., rows, n // 2 + 1] complex."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    K = n // 2 + 1
    g = _groups(x)
    x0, x1 = _pairs(g * scale)
    with np.errstate(all='ignore'):
        zr, zi = _dft(x0.copy(), x1.copy(), n)
        k = np.arange(K)
        nk = np.where(k == 0, 0, n - k)
        wr, wi = zr[:, nk], zi[:, nk]
        zr, zi = zr[:, :K], zi[:, :K]
        X0 = (zr + wr) * 0.5 + 1j * ((zi - wi) * 0.5)
        X1 = (zi + wi) * 0.5 + 1j * ((wr - zr) * 0.5)
    return _unpairs(X0, X1, g.shape[0], g.shape[1]).reshape(x.shape[:-1] + (K,))


def irfft_rows(X, n):
    """Half spectrum [..., rows, n // 2 + 1] complex -> real [..., rows, n] (numpy.fft.irfft(X, n): Im X[0] and Im X[n/2]
    are ignored)."""
    X = np.asarray(X, dtype=np.complex128)
    K = n // 2 + 1
    assert X.shape[-1] == K
    g = _groups(X)
    P, Q = _pairs(g)
    i = np.arange(n)
    up = i >= K
    k = np.where(up, n - i, i)
    edge = (k == 0) | (2 * k == n)
    sgn = np.where(up, -1.0, 1.0)
    pr, pi = P.real[:, k], np.where(edge, 0.0, P.imag[:, k]) * sgn
    qr, qi = Q.real[:, k], np.where(edge, 0.0, Q.imag[:, k]) * sgn
    with np.errstate(all='ignore'):
        zr, zi = _dft(pr - qi, -(pi + qr), n)
        x0, x1 = zr / float(n), -zi / float(n)
    return _unpairs(x0, x1, g.shape[0], g.shape[1]).reshape(X.shape[:-1] + (n,))


def system(A, C, ratioSqr, lam):
    """Rows j = 1 .. yc-2 of the tridiagonal systems: lo_j, up_j [..., yc], di_jk [..., yc, K] (rows 0, yc-1: zeros)."""
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    lo, up = np.zeros_like(A), np.zeros_like(A)
    di = np.zeros(A.shape + (lam.size,))
    lo[..., 1:-1] = A[..., 1:-1] * ratioSqr
    up[..., 1:-1] = A[..., 2:] * ratioSqr
    di[..., 1:-1, :] = -(((A[..., 2:] + A[..., 1:-1]) * ratioSqr)[..., None] + C[..., 1:-1, None] * lam)
    return lo, up, di


def undef_count(S0, A, C, F, undef):
    """[nbatch]: how many of the points the solve reads hold `undef` (k_fourier_check)."""
    S0, F = np.asarray(S0), np.asarray(F)
    nb = S0.shape[0]
    A, C = np.broadcast_to(A, (nb, S0.shape[1])), np.broadcast_to(C, (nb, S0.shape[1]))
    return ((F[:, 1:-1] == undef).sum(axis=(1, 2)) + (S0[:, 0] == undef).sum(axis=1) + (S0[:, -1] == undef).sum(axis=1) +
            (A[:, 1:] == undef).sum(axis=1) + (C[:, 1:-1] == undef).sum(axis=1))


def solve(S0, A, C, F, delxSqr, ratioSqr, undef=-9.99e8):
    """-> (S, flags) as xinv_fourier_standard_2d_f64_dev returns them; S0, F [nbatch, yc, xc] or [yc, xc]."""
    one = np.ndim(S0) == 2
    S0 = np.array(S0, dtype=np.float64, copy=True).reshape((-1,) + np.shape(S0)[-2:])
    F = np.asarray(F, dtype=np.float64).reshape(S0.shape)
    nb, yc, xc = S0.shape
    if yc < 3 or xc < 3:
        raise ValueError('every core dimension needs at least 3 points')
    factor(xc)
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), (nb, yc))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (nb, yc))
    bad = undef_count(S0, A, C, F, undef)
    if bad.any():
        raise ValueError('member %d holds undef at %d of the points the solve reads' % (int(np.argmax(bad > 0)), bad[bad > 0][0]))
    _, lam = tables(xc)
    lo, up, di = system(A, C, ratioSqr, lam)
    spec = np.zeros((nb, yc, xc // 2 + 1), dtype=np.complex128)
    spec[:, 1:-1] = rfft_rows(F[:, 1:-1], delxSqr)
    spec[:, [0, yc - 1]] = rfft_rows(S0[:, [0, yc - 1]])
    with np.errstate(all='ignore'):
        gam = np.zeros((nb, yc, lam.size))
        pr, pi = spec[:, 0].real.copy(), spec[:, 0].imag.copy()
        gp = np.zeros((nb, lam.size))
        for j in range(1, yc - 1):
            l, u = lo[:, j, None], up[:, j, None]
            rr, ri = spec[:, j].real.copy(), spec[:, j].imag.copy()
            if j == yc - 2:
                rr = rr - u * spec[:, yc - 1].real
                ri = ri - u * spec[:, yc - 1].imag
            inv = 1.0 / (di[:, j] if j == 1 else di[:, j] - l * gp)
            pr = (rr - l * pr) * inv
            pi = (ri - l * pi) * inv
            gp = u * inv
            gam[:, j] = gp
            spec[:, j] = pr + 1j * pi
        for j in range(yc - 3, 0, -1):
            pr = spec[:, j].real - gam[:, j] * pr
            pi = spec[:, j].imag - gam[:, j] * pi
            spec[:, j] = pr + 1j * pi
        S0[:, 1:-1] = irfft_rows(spec[:, 1:-1], xc)
    fl = np.zeros((nb, 3))
    fl[:, 0] = (~np.isfinite(spec[:, 1:-1])).any(axis=(1, 2))
    return (S0[0], fl[0]) if one else (S0, fl)
