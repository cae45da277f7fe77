"""Test-side restatements of the tridiagonal direct solver (reference numbas.trace / traceCyclic, numbas.py:1589-1685)
and of the system the direct path of the 1-D standard form assembles (XINV_PATH_DIRECT1D, include/xinv.h).

trace, traceCyclic   the reference's recurrence, expression by expression and in its loop order, in float64 -- vectorised
                     over any leading (batch) axes, which changes no bit: every system sees the same IEEE operations in
                     the same order.  The golden cases (tests/golden/tridiag_cases.npz, written by the reference itself)
                     pin them bit for bit; the HIP kernel k_tridiag is compared with them bit for bit.
assemble             S0, A, B, F -> lower, diagonal, upper, right-hand side, a0, cn and which members close cyclically.
direct_solve         assemble + trace / traceCyclic -> (S, flags [nbatch, 3]) as the direct path returns them.
All leave their inputs alone.
"""
import numpy as np

BCS = ['fixed', 'extend', 'periodic']


def _bc(BCx):
    return BCx if isinstance(BCx, str) else BCS[int(BCx)]


def _t(v):
    """[..., n] -> [n, ...] float64 (the march indexes the first axis)."""
    return np.moveaxis(np.asarray(v, dtype=np.float64), -1, 0)


def trace(a, b, c, d):
    """numbas.py:1610-1636; a, c [..., N-1], b, d [..., N] (leading axes broadcast)."""
    a, b, c, d = _t(a), _t(b), _t(c), _t(d)
    N = b.shape[0]
    if a.shape[0] != N - 1 or d.shape[0] != N or c.shape[0] != N - 1:
        raise Exception('lengths of given arrays are not satisfied')
    lead = np.broadcast_shapes(a.shape[1:], b.shape[1:], c.shape[1:], d.shape[1:])
    buf0 = np.zeros((N,) + lead)
    buf1 = np.zeros((N - 1,) + lead)
    res = np.zeros((N,) + lead)
    with np.errstate(all='ignore'):
        buf1[0] = c[0] / b[0]
        buf0[0] = b[0]
        for i in range(1, N - 1):
            buf0[i] = b[i] - a[i - 1] * buf1[i - 1]
            buf1[i] = c[i] / buf0[i]
        buf0[N - 1] = b[N - 1] - a[N - 2] * buf1[N - 2]
        res[0] = d[0] / buf0[0]
        for i in range(1, N):
            res[i] = (d[i] - a[i - 1] * res[i - 1]) / buf0[i]
        for i in range(N - 2, -1, -1):
            res[i] -= buf1[i] * res[i + 1]
    return np.ascontiguousarray(np.moveaxis(res, 0, -1))


def traceCyclic(a, b, c, d, a0, cn):
    """numbas.py:1664-1685; a0, cn scalars or one value per system."""
    b_ = np.asarray(b, dtype=np.float64)
    d_ = np.asarray(d, dtype=np.float64)
    a0, cn = np.asarray(a0, dtype=np.float64), np.asarray(cn, dtype=np.float64)
    N = b_.shape[-1]
    lead = np.broadcast_shapes(np.shape(a)[:-1], b_.shape[:-1], np.shape(c)[:-1], d_.shape[:-1], a0.shape, cn.shape)
    buf4 = np.zeros(lead + (N,))
    buf4[..., N - 1], buf4[..., 0] = cn, 0
    buf1 = np.broadcast_to(trace(a, b, c, buf4), lead + (N,))
    buf4[..., N - 1], buf4[..., 0] = 0, a0
    buf2 = np.broadcast_to(trace(a, b, c, buf4), lead + (N,))
    buf3 = np.broadcast_to(trace(a, b, c, d), lead + (N,))
    res = np.zeros(lead + (N,))
    with np.errstate(all='ignore'):
        res[..., N - 1] = ((1.0 + buf1[..., 0]) / buf1[..., N - 1] * buf3[..., N - 1] - buf3[..., 0]) / \
                          ((1.0 + buf1[..., 0]) * (1.0 + buf2[..., N - 1]) / buf1[..., N - 1] - buf2[..., 0])
        res[..., 0] = (buf3[..., 0] - buf2[..., 0] * res[..., N - 1]) / (1 + buf1[..., 0])
        r0, rn = res[..., 0:1], res[..., N - 1:N]
        res[..., 1:N - 1] = buf3[..., 1:N - 1] - buf1[..., 1:N - 1] * r0 - buf2[..., 1:N - 1] * rn
    return res


def assemble(S0, A, B, F, BCx, delxSqr, undef):
    """The system of the direct path: dict(lo, di, up, rh [nbatch, xc], a0, cn, cyc [nbatch]).  Row i reads
    lo[i] x[i-1] + di[i] x[i] + up[i] x[i+1] = rh[i]; lo[0] and up[xc-1] are the periodic corners."""
    BCx = _bc(BCx)
    S0 = np.atleast_2d(np.asarray(S0, dtype=np.float64))
    nb, xc = S0.shape
    A, B, F = (np.broadcast_to(np.asarray(v, dtype=np.float64), (nb, xc)) for v in (A, B, F))
    per = BCx == 'periodic'
    idx = np.arange(xc)
    Ap = A[:, (idx + 1) % xc]
    inner = ((idx >= 1) & (idx <= xc - 2)) | per
    live = inner[None, :] & (F != undef) & (A != undef) & (Ap != undef) & (B != undef)
    with np.errstate(all='ignore'):
        lo = np.where(live, A / delxSqr, 0.0)
        up = np.where(live, Ap / delxSqr, 0.0)
        di = np.where(live, B - (Ap + A) / delxSqr, 1.0)
        rh = np.where(live, F, S0)
        cyc = np.zeros(nb, bool)
        if BCx == 'extend':
            e0, en = S0[:, 1] != undef, S0[:, xc - 2] != undef
            di[e0, 0], up[e0, 0], rh[e0, 0] = 1.0, -1.0, 0.0
            lo[en, xc - 1], di[en, xc - 1], rh[en, xc - 1] = -1.0, 1.0, 0.0
        if per:
            live0, liven = live[:, 0], live[:, xc - 1]
            cyc = live0 & liven
            w0, wn = live0 & ~liven, liven & ~live0        # the other end is an identity row: its value is known
            rh[w0, 0] = F[w0, 0] - lo[w0, 0] * S0[w0, xc - 1]
            rh[wn, xc - 1] = F[wn, xc - 1] - up[wn, xc - 1] * S0[wn, 0]
    return dict(lo=lo, di=di, up=up, rh=rh, a0=lo[:, 0].copy(), cn=up[:, xc - 1].copy(), cyc=cyc)


def direct_solve(S0, A, B, F, BCx, delxSqr, undef):
    """-> (S [nbatch, xc] (or [xc] for a 1-D S0), flags [nbatch, 3] (or [3])) of XINV_PATH_DIRECT1D."""
    one = np.ndim(S0) == 1
    s = assemble(S0, A, B, F, BCx, delxSqr, undef)
    x = trace(s['lo'][:, 1:], s['di'], s['up'][:, :-1], s['rh'])
    if s['cyc'].any():
        xcy = traceCyclic(s['lo'][:, 1:], s['di'], s['up'][:, :-1], s['rh'], s['a0'], s['cn'])
        x = np.where(s['cyc'][:, None], xcy, x)
    fl = np.zeros((x.shape[0], 3))
    fl[:, 0] = (~np.isfinite(x)).any(axis=1)
    return (x[0], fl[0]) if one else (x, fl)
