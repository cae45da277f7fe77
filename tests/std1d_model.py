"""Test-side restatements of the 1-D standard-form SOR (reference numbas.invert_standard_1D, numbas.py:633-742).

lex_solve  the reference's own lexicographic sweep, point by point in Python floats: the golden cases
           (tests/golden/std1d_cases.npz, written by the reference itself) pin it bit for bit.
rb_solve   the same arithmetic in the order the HIP kernel k_std1d documents (xinvert_amd/csrc/xinv_std1d.h):
           red-black on i & 1, colour 0 first, periodic odd xc's point xc-1 as its own colour right after colour 0,
           and the norm summed per lane chunk, over the lanes by the xor butterfly, over the wavefronts in order.
Both return (S, flags) and leave the inputs alone.
"""
import math

import numpy as np

BC_CODES = {'fixed': 0, 'extend': 1, 'periodic': 2}
MAX_XC = 8192          # XINV_STD1D_MAX_XC
WAVE_XC = 512          # XINV_STD1D_WAVE_XC


def shape(xc):
    """(points per lane, wavefronts) of a member of xc points (xinv_std1d_shape)."""
    if xc <= WAVE_XC:
        p = 2
        while 64 * p < xc:
            p *= 2
        return p, 1
    if xc <= MAX_XC:
        return 8, (xc + 511) // 512
    raise ValueError('xc > %d' % MAX_XC)


def _bc(BCx):
    return BCx if isinstance(BCx, str) else {v: k for k, v in BC_CODES.items()}[int(BCx)]


def lex_solve(S, A, B, F, BCx, delxSqr, optArg, undef, mxLoop, tolerance, flags=None):
    """numbas.py:680-742 restated in Python floats (lexicographic)."""
    BCx = _bc(BCx)
    S = [float(v) for v in np.asarray(S, dtype=np.float64)]
    A = [float(v) for v in A]
    B = [float(v) for v in B]
    F = [float(v) for v in F]
    xc = len(S)
    fl = [0.0, 1.0, 0.0] if flags is None else [float(v) for v in flags]
    loop = 0
    normPrev = np.finfo(np.float64).max

    def upd(i, im, ip, ia):
        # ia: index of "A[i+1]"
        if F[i] != undef and A[i] != undef and A[ia] != undef and B[i] != undef:
            t = (A[ia] * (S[ip] - S[i]) - A[i] * (S[i] - S[im])) / delxSqr + (B[i] * S[i] - F[i])
            t *= optArg / ((A[ia] + A[i]) / delxSqr - B[i])
            S[i] += t

    while True:
        if BCx == 'extend':
            if S[1] != undef:
                S[0] = S[1]
            if S[-2] != undef:
                S[-1] = S[-2]
        if BCx == 'periodic':
            upd(0, xc - 1, 1, 1)
        for i in range(1, xc - 1):
            upd(i, i - 1, i + 1, i + 1)
        if BCx == 'periodic':
            upd(xc - 1, xc - 2, 0, 0)
        norm, count = 0.0, 0
        for v in S:
            if v != undef:
                norm += abs(v)
                count += 1
        norm = norm / count if count else math.nan
        if math.isnan(norm) or norm > 1e100:
            fl[0] = 1.0
            break
        fl[1] = abs(norm - normPrev) / normPrev
        fl[2] = loop
        if fl[1] < tolerance or loop >= mxLoop or norm == 0:
            break
        normPrev = norm
        loop += 1
    return np.array(S), np.array(fl)


def kernel_norm(S, undef):
    """mean |S| over S != undef in k_std1d's order: lane chunks in index order, xor butterfly, waves in order."""
    xc = len(S)
    ppl, nw = shape(xc)
    v = np.zeros(nw * 64 * ppl)
    ok = S != undef
    v[:xc] = np.where(ok, np.abs(S), 0.0)
    v = v.reshape(nw * 64, ppl)
    s = np.zeros(nw * 64)
    for k in range(ppl):
        s = s + v[:, k]
    s = s.reshape(nw, 64)
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ d]
    tot = s[0, 0]
    for w in range(1, nw):
        tot = tot + s[w, 0]
    cnt = int(ok.sum())
    return tot / cnt if cnt else math.nan


def rb_solve(S, A, B, F, BCx, delxSqr, optArg, undef, mxLoop, tolerance, flags=None):
    """The kernel's red-black ordering and norm order with the reference's point arithmetic."""
    BCx = _bc(BCx)
    S = np.array(S, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    xc = len(S)
    per, ext = BCx == 'periodic', BCx == 'extend'
    seam = per and xc % 2 == 1
    fl = np.array([0.0, 1.0, 0.0]) if flags is None else np.array(flags, dtype=np.float64)
    idx = np.arange(xc)
    Ap = A[(idx + 1) % xc]
    with np.errstate(all='ignore'):
        fac = optArg / ((Ap + A) / delxSqr - B)
    upd = (idx >= 1) & (idx <= xc - 2)
    if per:
        upd |= (idx == 0) | (idx == xc - 1)
    pred = upd & (F != undef) & (A != undef) & (Ap != undef) & (B != undef)
    c0 = pred & (idx % 2 == 0)
    if seam:
        c0[xc - 1] = False
    cS = np.zeros(xc, bool)
    if seam:
        cS[xc - 1] = pred[xc - 1]
    c1 = pred & (idx % 2 == 1)
    im, ip = (idx - 1) % xc, (idx + 1) % xc

    def colour(c):
        i = idx[c]
        if len(i) == 0:
            return
        Si, Sm, Sp = S[i], S[im[i]], S[ip[i]]
        t = (Ap[i] * (Sp - Si) - A[i] * (Si - Sm)) / delxSqr + (B[i] * Si - F[i])
        t = t * fac[i]
        S[i] = Si + t

    loop = 0
    normPrev = np.finfo(np.float64).max
    with np.errstate(all='ignore'):
        while True:
            if ext:
                if S[1] != undef:
                    S[0] = S[1]
                if S[-2] != undef:
                    S[-1] = S[-2]
            colour(c0)
            colour(cS)
            colour(c1)
            norm = kernel_norm(S, undef)
            if math.isnan(norm) or norm > 1e100:
                fl[0] = 1.0
                break
            fl[1] = abs(norm - normPrev) / normPrev
            fl[2] = loop
            if fl[1] < tolerance or loop >= mxLoop or norm == 0:
                break
            normPrev = norm
            loop += 1
    return S, fl
