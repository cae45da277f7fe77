// xinv_cfourier_host.h -- the solve of the 2-D general form (xinv_cfourier.h) on device arrays: the steps of a one-shot solve
// of xinv_fourier_host.h around the general form's own kernels.  The call, its checks, the transforms, the workspace and
// the host-pointer staging are those of xinv_fourier_host.h.  Included by xinv_hip.hip only, after it.
#pragma once
#include "xinv_cfourier.h"

// The workspace holds, behind the spectrum, the factors [nset][2][yc][K] complex, then lo and up [nset][2][yc]
static int cfourier_run_dev(const FourierCall &c, double *flags, hipStream_t st)
{
    FourierRun r;
    const int64_t nb = c.nbatch, yc = c.yc, xc = c.xc, K = xc / 2 + 1, plane = yc * K;
    int64_t nset = 1;
    for (int q = 1; q <= 5; q++)
        if (c.stride(q) != 0) nset = nb;
    int rc = fourier_open(r, c, (size_t)nset * (size_t)plane * 4 + (size_t)nset * 2 * (size_t)yc, st);
    if (rc) return rc;
    double *fac = r.rest, *lu = fac + (size_t)nset * plane * 4;
    CFourierCheckArgs k;
    memset(&k, 0, sizeof k);
    k.S = c.S(); k.G = c.forcing(); k.sS = c.stride(0); k.sG = c.stride(6);
    for (int q = 0; q < 5; q++) { k.c[q] = c.coef(q); k.sc[q] = c.stride(1 + q); }
    k.yc = yc; k.xc = xc; k.undef = c.undef; k.bad = r.bad;
    xinv_launch_fourier_gcheck(k, nb, st);
    if ((rc = fourier_checked(r, nb, "G, A, C, D, E, F", st))) return rc;

    CFourierFactorArgs f;                                // the factors of every wavenumber's system, per coefficient set
    memset(&f, 0, sizeof f);
    f.fac = fac; f.lu = lu;
    f.A = k.c[0]; f.C = k.c[1]; f.D = k.c[2]; f.E = k.c[3]; f.Fc = k.c[4];
    f.sA = k.sc[0]; f.sC = k.sc[1]; f.sD = k.sc[2]; f.sE = k.sc[3]; f.sFc = k.sc[4];
    f.lam = r.tab + 2 * xc; f.sig = r.tab + 2 * xc + K;
    f.yc = yc; f.K = K;
    f.delx = c.delx; f.delxSqr = c.delxSqr; f.ratio = c.ratio; f.ratioSqr = c.ratioSqr;
    xinv_launch_fourier_cfactor(f, nset, st);
    HIPCHK(hipGetLastError());
    FourierDfts d = fourier_dfts(r.dft, r.spec, c.S(), c.forcing(), k.sS, k.sG, nb, yc, xc, c.delxSqr, nullptr);
    if ((rc = fourier_forward(d, st))) return rc;
    CFourierSubstArgs t;                                 // one complex tridiagonal system per wavenumber and member
    memset(&t, 0, sizeof t);
    t.spec = r.spec; t.fac = fac; t.lu = lu;
    t.sfac = nset > 1 ? 4 * plane : 0; t.slu = nset > 1 ? 2 * yc : 0;
    t.yc = yc; t.K = K; t.ovf = r.ovf;
    xinv_launch_fourier_csubst(t, nb, st);
    HIPCHK(hipGetLastError());
    if ((rc = fourier_rowdft(d.inv, true, st))) return rc;
    return fourier_close(r, nb, 5, flags, st);
}
