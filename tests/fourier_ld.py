"""A long-double truth for the direct Fourier solve of the 2-D standard form for periodic x, without a GPU
and without tests/fourier_model.py: only the equation in the header of xinvert_amd/csrc/xinv_fourier.h is shared.

    dft_longdouble(x)          -> (re, im) of the half spectrum of real rows by the O(n^2) sum
    err_ld(X, truth)           -> relative L2 distance of a complex128 spectrum from that sum
    ld_solve(S0, A, C, F, delxSqr, ratioSqr) -> S     the full xc x xc DFT matrix, one Thomas recurrence per wavenumber
    ld_backward(S, A, C, F, delxSqr, ratioSqr) -> [nbatch]   max|R| / max|F| of the five-point equation, evaluated directly
Everything is numpy.longdouble (64 significant bits on x86-64: eps 2^-63); S0, F are [nbatch, yc, xc] or [yc, xc], A and C
one value per row, [yc] or [nbatch, yc].  Inputs are left alone.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).eps <= 2.0 ** -63, 'numpy.longdouble is no wider than float64 here: the long-double truth needs a wider type'

PI = LD('3.14159265358979323846264338327950288')


# ------------------------------------------------------------------ the row transform
_WLD = {}


def dft_longdouble(x):
    """The half spectrum of real rows [rows, n] by the O(n^2) sum in long double, exp(-2 pi i t / n) tabulated once per n."""
    n = x.shape[-1]
    if n not in _WLD:
        ang = LD(2) * LD('3.14159265358979323846264338327950288') * np.arange(n, dtype=LD) / LD(n)
        _WLD[n] = (np.cos(ang), -np.sin(ang))
    wr, wi = _WLD[n]
    xl = x.astype(LD)
    K = n // 2 + 1
    out_r, out_i = np.empty((x.shape[0], K), dtype=LD), np.empty((x.shape[0], K), dtype=LD)
    i = np.arange(n)
    for k0 in range(0, K, 64):                             # (in blocks of wavenumbers: the table index is (i k) mod n)
        k = np.arange(k0, min(K, k0 + 64))
        t = (i[None, :] * k[:, None]) % n
        out_r[:, k] = xl @ wr[t].T
        out_i[:, k] = xl @ wi[t].T
    return out_r, out_i


def err_ld(X, truth):
    tr, ti = truth
    dr, di = X.real.astype(LD) - tr, X.imag.astype(LD) - ti
    return float(np.sqrt((dr * dr + di * di).sum()) / np.sqrt((tr * tr + ti * ti).sum()))


# ------------------------------------------------------------------ the solve
_MAT = {}


def _dft_matrix(xc):
    """[xc, xc] complex long double: exp(-2 pi i (i k mod xc) / xc), from a table of xc values."""
    if xc not in _MAT:
        ang = LD(2) * PI * np.arange(xc, dtype=LD) / LD(xc)
        w = np.empty(xc, dtype=CLD)
        w.real, w.imag = np.cos(ang), -np.sin(ang)
        i = np.arange(xc)
        _MAT[xc] = w[(i[:, None] * i[None, :]) % xc]
    return _MAT[xc]


def _batched(S0, A, C, F):
    S = np.asarray(S0)
    one = S.ndim == 2
    S = S.astype(LD).reshape((-1,) + S.shape[-2:])
    F = np.asarray(F).astype(LD).reshape(S.shape)
    nb, yc, _ = S.shape
    A = np.broadcast_to(np.asarray(A).astype(LD), (nb, yc))
    C = np.broadcast_to(np.asarray(C).astype(LD), (nb, yc))
    return one, S, A, C, F


def ld_solve(S0, A, C, F, delxSqr, ratioSqr):
    """Rows 1 .. yc-2 of  lo_j X[j-1] + di_jk X[j] + up_j X[j+1] = DFT(F[j] delxSqr)[k]  for every wavenumber k = 0 .. xc-1,
    lo_j = A[j] ratioSqr, up_j = A[j+1] ratioSqr, di_jk = -((A[j+1] + A[j]) ratioSqr + C[j] lambda_k), rows 0 and yc-1 of S0
    known and moved to the right-hand sides; back through the conjugate matrix divided by xc."""
    one, S, A, C, F = _batched(S0, A, C, F)
    nb, yc, xc = S.shape
    rs, dx2 = LD(ratioSqr), LD(delxSqr)
    W = _dft_matrix(xc)
    s = np.sin(PI * np.arange(xc, dtype=LD) / LD(xc))
    lam = LD(4) * s * s                                                      # [xc]
    rhs = (F * dx2).astype(CLD) @ W                                          # [nb, yc, xc]; rows 0 and yc-1 are not used
    bottom, top = S[:, 0].astype(CLD) @ W, S[:, yc - 1].astype(CLD) @ W
    sub = A[:, :-1] * rs                                                     # sub[:, j]: the coefficient of X[j-1] in row j
    sup = np.concatenate([A[:, 1:] * rs, np.zeros((nb, 1), dtype=LD)], axis=1)   # sup[:, j]: that of X[j+1]
    dia = -((sup + A * rs)[:, :, None] + C[:, :, None] * lam)                # [nb, yc, xc]
    rhs[:, 1] = rhs[:, 1] - sub[:, 1, None] * bottom
    rhs[:, yc - 2] = rhs[:, yc - 2] - sup[:, yc - 2, None] * top
    cp = np.zeros((nb, yc, xc), dtype=LD)
    dp = np.zeros((nb, yc, xc), dtype=CLD)
    cp[:, 1] = sup[:, 1, None] / dia[:, 1]
    dp[:, 1] = rhs[:, 1] / dia[:, 1]
    for j in range(2, yc - 1):
        den = dia[:, j] - sub[:, j, None] * cp[:, j - 1]
        cp[:, j] = sup[:, j, None] / den
        dp[:, j] = (rhs[:, j] - sub[:, j, None] * dp[:, j - 1]) / den
    X = np.zeros((nb, yc, xc), dtype=CLD)
    X[:, yc - 2] = dp[:, yc - 2]
    for j in range(yc - 3, 0, -1):
        X[:, j] = dp[:, j] - cp[:, j] * X[:, j + 1]
    out = S.copy()
    out[:, 1:-1] = ((X[:, 1:-1] @ np.conj(W)) / LD(xc)).real
    return out[0] if one else out


def ld_backward(S, A, C, F, delxSqr, ratioSqr):
    """[nbatch] max|R| / max|F| over rows 1 .. yc-2, R = (A[j] rs S[j-1] + A[j+1] rs S[j+1] - (A[j+1] + A[j]) rs S[j]
    + C[j] (S[j, i-1] - 2 S[j, i] + S[j, i+1])) / delxSqr - F[j], the columns wrapping along x."""
    _, S, A, C, F = _batched(S, A, C, F)
    rs, dx2 = LD(ratioSqr), LD(delxSqr)
    mid, lo, up = S[:, 1:-1], S[:, :-2], S[:, 2:]
    a_lo, a_up, c = (A[:, 1:-1] * rs)[:, :, None], (A[:, 2:] * rs)[:, :, None], C[:, 1:-1, None]
    along_x = np.roll(mid, 1, axis=2) - LD(2) * mid + np.roll(mid, -1, axis=2)
    R = (a_lo * lo + a_up * up - (a_up + a_lo) * mid + c * along_x) / dx2 - F[:, 1:-1]
    return np.abs(R).max(axis=(1, 2)) / np.abs(F[:, 1:-1]).max(axis=(1, 2))
