"""The residual R = L(S) - F of the five second-order forms, restated in numpy: what k_resid2d / k_resid3d
must give bit for bit.  Plain float64 numpy arithmetic evaluates every binary operation in the order written, without
contraction, so the expressions below -- the reference's `temp`, operand by operand (numbas.py:312-399, 1095-1183,
530-620, 117-196, 820-981), divided by delxSqr -- are also the rounding.

    residual(kind, S, coefs, sc, per, undef) -> R        one member; coefs: the form's arrays, forcing last; B may be None
    norms(kind, R, coefs, undef, live) -> [n_live, mean|R|, max|R|, max|F|]
"""
import numpy as np

KINDS = ('std2d', 'gen2d', 'std2dt', 'std3d', 'gen3d')


def _sh(a, dj, di):
    """a[j + dj, i + di] on the interior rows, every column, x wrapped (rows: a 2-D array's axis 0)."""
    return np.roll(a, -di, axis=-1)[..., 1 + dj:a.shape[-2] - 1 + dj, :]


def _res2d(kind, S, c, sc, west_col):
    """(temp / delxSqr, cond) on rows 1 .. yc-2, all columns (x wrapped).  west_col: a bool row, True at i == 0."""
    u = sc['undef']
    sC, sP, sM, sW, sE = _sh(S, 0, 0), _sh(S, 1, 0), _sh(S, -1, 0), _sh(S, 0, -1), _sh(S, 0, 1)
    sPE, sPW, sME, sMW = _sh(S, 1, 1), _sh(S, 1, -1), _sh(S, -1, 1), _sh(S, -1, -1)
    sM_q = np.where(west_col, sM, sME)                       # the i == 0 irregularity (numbas.py:327-328): S[j-1, 0]
    rS, rQ, dS = sc.get('ratioSqr'), sc.get('ratioQtr'), sc['delxSqr']
    if kind == 'std2d':
        A, B, C, F = c
        aP, a0, cE, c0, f = _sh(A, 1, 0), _sh(A, 0, 0), _sh(C, 0, 1), _sh(C, 0, 0), _sh(F, 0, 0)
        if B is None:
            cond = (f != u) & (aP != u) & (a0 != u) & (cE != u) & (c0 != u)
            temp = ((aP * (sP - sC) - a0 * (sC - sM)) * rS + (cE * (sE - sC) - c0 * (sC - sW))) - f * dS
        else:
            bE, bW, bPc, bM = _sh(B, 0, 1), _sh(B, 0, -1), _sh(B, 1, 0), _sh(B, -1, 0)
            bPu = np.where(west_col, _sh(B, 1, 1), bPc)      # ... and B[j+1, 1]
            cond = (f != u) & (aP != u) & (a0 != u) & (bE != u) & (bW != u) & (bPc != u) & (bM != u) & (cE != u) & (c0 != u)
            temp = ((aP * (sP - sC) - a0 * (sC - sM)) * rS + (bPu * (sPE - sPW) - bM * (sM_q - sMW)) * rQ +
                    (bE * (sPE - sME) - bW * (sPW - sMW)) * rQ + (cE * (sE - sC) - c0 * (sC - sW))) - f * dS
    elif kind == 'std2dt':
        A, B, C, D, E, F = c
        aP, a0, f, e = _sh(A, 1, 0), _sh(A, 0, 0), _sh(F, 0, 0), _sh(E, 0, 0)
        bPc, bM = _sh(B, 1, 0), _sh(B, -1, 0)
        bPu = np.where(west_col, _sh(B, 1, 1), bPc)
        cE, cW, dE, d0 = _sh(C, 0, 1), _sh(C, 0, -1), _sh(D, 0, 1), _sh(D, 0, 0)
        cond = (f != u) & (aP != u) & (a0 != u) & (bPc != u) & (bM != u) & (cE != u) & (cW != u) & (dE != u) & (d0 != u) & (e != u)
        temp = ((aP * (sP - sC) - a0 * (sC - sM)) * rS + (bPu * (sPE - sPW) - bM * (sM_q - sMW)) * rQ +
                (cE * (sPE - sME) - cW * (sPW - sMW)) * rQ + (dE * (sE - sC) - d0 * (sC - sW))) + (e * sC - f) * dS
    else:
        A, B, C, D, E, F, G = [None if a is None else _sh(a, 0, 0) for a in c]
        r, dx = sc['ratio'], sc['delx']
        if B is None:
            cond = (G != u) & (A != u) & (C != u) & (D != u) & (E != u) & (F != u)
            temp = (A * ((sP - sC) - (sC - sM)) * rS + C * ((sE - sC) - (sC - sW)) +
                    (D * (sP - sM) * r + E * (sE - sW)) * dx / 2.0 + (F * sC - G) * dS)
        else:
            cond = (G != u) & (A != u) & (B != u) & (C != u) & (D != u) & (E != u) & (F != u)
            temp = (A * ((sP - sC) - (sC - sM)) * rS + B * ((sPE - sME) - (sPW - sMW)) * rQ +
                    C * ((sE - sC) - (sC - sW)) + (D * (sP - sM) * r + E * (sE - sW)) * dx / 2.0 + (F * sC - G) * dS)
    return temp / dS, cond


def _s3(a, dk, dj, di):
    return np.roll(a, -di, axis=2)[1 + dk:a.shape[0] - 1 + dk, 1 + dj:a.shape[1] - 1 + dj, :]


def _res3d(kind, S, c, sc, west_col):
    u = sc['undef']
    sC, sKP, sKM = _s3(S, 0, 0, 0), _s3(S, 1, 0, 0), _s3(S, -1, 0, 0)
    sJP, sJM, sE, sW = _s3(S, 0, 1, 0), _s3(S, 0, -1, 0), _s3(S, 0, 0, 1), _s3(S, 0, 0, -1)
    r2S, r1S, dS = sc['ratio2Sqr'], sc['ratio1Sqr'], sc['delxSqr']
    if kind == 'std3d':
        A, B, C, F = c
        aP, a0, bP, b0 = _s3(A, 1, 0, 0), _s3(A, 0, 0, 0), _s3(B, 0, 1, 0), _s3(B, 0, 0, 0)
        cE, c0, f = _s3(C, 0, 0, 1), _s3(C, 0, 0, 0), _s3(F, 0, 0, 0)
        cond = (f != u) & (aP != u) & (a0 != u) & (bP != u) & (b0 != u) & (cE != u) & (c0 != u)
        temp = ((aP * (sKP - sC) - a0 * (sC - sKM)) * r2S + (bP * (sJP - sC) - b0 * (sC - sJM)) * r1S +
                (cE * (sE - sC) - c0 * (sC - sW))) - f * dS
    else:
        A, B, C, D, E, F, G, H = [_s3(a, 0, 0, 0) for a in c]
        r2, r1, dx = sc['ratio2'], sc['ratio1'], sc['delx']
        # the west-periodic branch tests G twice and never H (numbas.py:849-852)
        cond = (west_col | (H != u)) & (G != u) & (A != u) & (B != u) & (C != u) & (D != u) & (E != u) & (F != u)
        temp = (A * ((sKP - sC) - (sC - sKM)) * r2S + B * ((sJP - sC) - (sC - sJM)) * r1S +
                C * ((sE - sC) - (sC - sW)) + (D * (sKP - sKM) * r2 + E * (sJP - sJM) * r1 + F * (sE - sW)) * dx / 2.0 +
                (G * sC - H) * dS)
    return temp / dS, cond


def residual(kind, S, coefs, sc, per, undef):
    """-> (R, live): R shaped like S, `undef` where the reference updates nothing; live: the updated points."""
    S = np.asarray(S, dtype=np.float64)
    sc = dict(sc, undef=undef)
    xc = S.shape[-1]
    west = np.arange(xc) == 0
    with np.errstate(all='ignore'):
        val, cond = (_res3d if kind in ('std3d', 'gen3d') else _res2d)(kind, S, list(coefs), sc, west)
    if not per:
        cond = cond & ((np.arange(xc) >= 1) & (np.arange(xc) <= xc - 2))
    R = np.full(S.shape, undef, dtype=np.float64)
    live = np.zeros(S.shape, dtype=bool)
    inner = (slice(1, -1),) * (S.ndim - 1) + (slice(None),)
    R[inner] = np.where(cond, val, undef)
    live[inner] = cond
    return R, live


def norms(R, forcing, live):
    """[n_live, mean|R|, max|R|, max|F|] over the live points; a NaN among them makes the mean and its maximum NaN; no live
    point: mean NaN, maxima 0."""
    n = int(live.sum())
    if n == 0:
        return np.array([0.0, np.nan, 0.0, 0.0])
    ar, af = np.abs(R[live]), np.abs(np.asarray(forcing, dtype=np.float64)[live])
    mx = lambda v: np.nan if np.isnan(v).any() else v.max()
    return np.array([float(n), ar.sum() / n, mx(ar), mx(af)])
