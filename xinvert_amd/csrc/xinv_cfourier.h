// xinv_cfourier.h -- the direct Fourier solve of the 2-D GENERAL form for periodic x (include/xinv_fourier.h,
// xinv_fourier_general_2d_f64_*):
//   A d2S/dy2 + C d2S/dx2 + D dS/dy + E dS/dx + Fc S = G,   B == 0,   A, C, D, E, Fc functions of y alone,
//   BCy fixed, BCx periodic, no mask.
// With coefficients constant along x the fixed point of the sweep (numbas.py:1092-1184 with B == 0) commutes with the cyclic
// shift along x, so the transform of xinv_fourier.h (k_rowdft, reused as it is) turns it into one COMPLEX tridiagonal
// system in y per zonal wavenumber k -- E dS/dx makes the diagonal complex, D dS/dy makes lo and up differ:
//   lo_j X[j-1] + di_jk X[j] + up_j X[j+1] = DFT(G[j,:] * delxSqr)[k],      j = 1 .. yc-2
//   lo_j = A[j] ratioSqr - D[j] ratio (delx / 2),      up_j = A[j] ratioSqr + D[j] ratio (delx / 2)
//   Re di_jk = -(2 A[j] ratioSqr + C[j] lambda_k) + Fc[j] delxSqr,      lambda_k = 4 sin^2(pi k / xc)
//   Im di_jk = E[j] delx sigma_k,                                          sigma_k = sin(2 pi k / xc)
// with the known rows X[0] = DFT(S[0,:]) and X[yc-1] = DFT(S[yc-1,:]) moved to the right-hand sides of rows 1 and yc-2.
// Every coefficient is read at row j only.  lambda and sigma are host-built tables (sigma_0 and, for even xc, sigma_{xc/2}
// are exactly 0: the symbol is real where the half spectrum is).
//
// Three kernels; every call takes the same path, factor then substitute, so the bits do not depend on whether the
// coefficients are shared.
//   k_fourier_cfactor   one wavenumber per lane and coefficient set: the Thomas march without pivoting and without the
//                       right-hand sides, storing inv_j = 1 / (di_jk - lo_j gamma_{j-1}) and gamma_j = up_j inv_j, both
//                       complex; one real division per row (the reciprocal of re^2 + im^2, then two multiplications:
//                       the squares must neither overflow nor underflow, 1e-154 < |di - lo gamma| < 1e154).  Lane 0 of
//                       a set also stores lo_j and up_j, so the substitution works with the same bits of them.
//   k_fourier_csubst    one lane per wavenumber and member: forward rho_j = (r_j - lo_j rho_{j-1}) inv_j, backward
//                       x_j = rho_j - gamma_j x_{j+1}, complex, no division, in place on the spectrum; the rows are
//                       loaded a batch ahead of the chain.  A non-finite solution sets the member's word.
//   k_fourier_gcheck    counts `undef` among the points the solve reads; runs before anything is written.
// Rules of DESIGN 4.9: 64-bit indexing, solver data and tables through vector loads only, no floating-point atomics,
// complex arithmetic written out in real operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define XINV_CFAC_WG 64                  /* k_fourier_cfactor: one wavefront per workgroup, one wavenumber per lane */
#define XINV_CSUB_WG 64                  /* k_fourier_csubst: as k_fourier_cfactor */
#define XINV_CSUB_AHEAD 8                /* ... rows loaded ahead of the dependent chain */
#define XINV_GCHK_WG 256

// The factors of one coefficient set: two planes [yc][K] complex (re, im interleaved), inv then gamma; lo and up beside
// them as [nset][2][yc].
struct CFourierFactorArgs {
    double *fac;                         // [nset][2][yc][K] complex; rows 0 and yc-1 are not written
    double *lu;                          // [nset][2][yc]: lo, up; rows 0 and yc-1 are not written
    const double *A, *C, *D, *E, *Fc;    // one value per row, [nset or 1][yc]
    const double *lam, *sig;             // [K] each
    int64_t sA, sC, sD, sE, sFc;         // set strides (0 = shared)
    int64_t yc, K, set0;
    double delx, delxSqr, ratio, ratioSqr;
};

struct CFourierSubstArgs {
    double *spec;                        // [nbatch][yc][K] complex: rows 1 .. yc-2 right-hand sides -> solution; rows 0, yc-1 known
    const double *fac, *lu;              // CFourierFactorArgs::fac, ::lu
    int64_t sfac, slu;                   // member strides of fac and lu (0 = one shared set)
    int64_t yc, K, member0;
    int *ovf;                            // [nbatch]
};

struct CFourierCheckArgs {
    const double *S, *G;                 // [nbatch][yc][xc]
    const double *c[5];                  // A, C, D, E, Fc: one value per row
    int64_t sS, sG, sc[5];
    int64_t yc, xc, member0;
    double undef;
    int *bad;                            // [nbatch]: how many of the points the solve reads hold `undef`
};

#ifdef XINV_CFOURIER_KERNELS

// grid: (ceil(K / 64), coefficient sets of the chunk)
__global__ void __launch_bounds__(XINV_CFAC_WG) k_fourier_cfactor(CFourierFactorArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * XINV_CFAC_WG + threadIdx.x, s = a.set0 + blockIdx.y;
    if (k >= a.K) return;
    const int64_t yc = a.yc, K = a.K;
    double *iv = a.fac + s * 4 * yc * K + 2 * k, *gm = iv + 2 * yc * K;
    double *lop = a.lu + s * 2 * yc, *upp = lop + yc;
    const double *A = a.A + s * a.sA, *C = a.C + s * a.sC, *D = a.D + s * a.sD, *E = a.E + s * a.sE, *Fc = a.Fc + s * a.sFc;
    const double lam = a.lam[k], sig = a.sig[k];
    const double rs = a.ratioSqr, ratio = a.ratio, dx = a.delx, dx2 = a.delxSqr, hd = a.delx * 0.5;
    double gr = 0.0, gi = 0.0;
    for (int64_t j = 1; j <= yc - 2; j++) {
        const double ars = A[j] * rs, dh = (D[j] * ratio) * hd;
        const double lo = ars - dh, up = ars + dh;
        const double dr = -(2.0 * ars + C[j] * lam) + Fc[j] * dx2, di = (E[j] * dx) * sig;
        const double er = j == 1 ? dr : dr - lo * gr, ei = j == 1 ? di : di - lo * gi;
        const double q = 1.0 / (er * er + ei * ei);
        const double ir = er * q, ii = -(ei * q);
        gr = up * ir;
        gi = up * ii;
        iv[2 * j * K] = ir;
        iv[2 * j * K + 1] = ii;
        gm[2 * j * K] = gr;
        gm[2 * j * K + 1] = gi;
        if (k == 0) { lop[j] = lo; upp[j] = up; }
    }
}

// grid: (ceil(K / 64), members of the chunk).  The loads of a batch of rows do not depend on the chain: they are issued a
// batch ahead of it (unconditionally -- past the march's end they read its last row again, unused), and nothing in the
// load phase uses a loaded value.
__global__ void __launch_bounds__(XINV_CSUB_WG) k_fourier_csubst(CFourierSubstArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * XINV_CSUB_WG + threadIdx.x, m = a.member0 + blockIdx.y;
    const int64_t yc = a.yc, K = a.K, K2 = 2 * a.K;
    if (k >= K) return;
    constexpr int U = XINV_CSUB_AHEAD;
    double *sp = a.spec + m * yc * K2 + 2 * k;
    const double *iv = a.fac + m * a.sfac + 2 * k, *gm = iv + yc * K2;
    const double *lop = a.lu + m * a.slu, *upp = lop + yc;

    // forward: rows ascending; the known row 0 enters through lo_1, row yc-1 through up on row yc-2
    const int64_t jl = yc - 2;
    const double lastr = sp[(yc - 1) * K2], lasti = sp[(yc - 1) * K2 + 1], upl = upp[jl];
    double pr = sp[0], pi = sp[1];
    double rr[U], ri[U], fr[U], fi[U], la[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t j = 1 + u <= jl ? 1 + u : jl;
        rr[u] = sp[j * K2]; ri[u] = sp[j * K2 + 1]; fr[u] = iv[j * K2]; fi[u] = iv[j * K2 + 1]; la[u] = lop[j];
    }
    for (int64_t j0 = 1; j0 <= jl; j0 += U) {
        double nr[U], ni[U], gr[U], gi[U], ln[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + U + u <= jl ? j0 + U + u : jl;
            nr[u] = sp[j * K2]; ni[u] = sp[j * K2 + 1]; gr[u] = iv[j * K2]; gi[u] = iv[j * K2 + 1]; ln[u] = lop[j];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + u;
            if (j <= jl) {
                double tr = rr[u], ti = ri[u];
                if (j == jl) { tr = tr - upl * lastr; ti = ti - upl * lasti; }
                tr = tr - la[u] * pr;
                ti = ti - la[u] * pi;
                pr = tr * fr[u] - ti * fi[u];
                pi = tr * fi[u] + ti * fr[u];
                sp[j * K2] = pr;
                sp[j * K2 + 1] = pi;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { rr[u] = nr[u]; ri[u] = ni[u]; fr[u] = gr[u]; fi[u] = gi[u]; la[u] = ln[u]; }
    }
    // backward: row yc-2 stands
    int bad = !(isfinite(pr) && isfinite(pi));
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t j = jl - 1 - u >= 1 ? jl - 1 - u : 1;
        rr[u] = sp[j * K2]; ri[u] = sp[j * K2 + 1]; fr[u] = gm[j * K2]; fi[u] = gm[j * K2 + 1];
    }
    for (int64_t j0 = jl - 1; j0 >= 1; j0 -= U) {
        double nr[U], ni[U], gr[U], gi[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 - U - u >= 1 ? j0 - U - u : 1;
            nr[u] = sp[j * K2]; ni[u] = sp[j * K2 + 1]; gr[u] = gm[j * K2]; gi[u] = gm[j * K2 + 1];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 - u;
            if (j >= 1) {
                const double xr = rr[u] - (fr[u] * pr - fi[u] * pi), xi = ri[u] - (fr[u] * pi + fi[u] * pr);
                pr = xr;
                pi = xi;
                sp[j * K2] = pr;
                sp[j * K2 + 1] = pi;
                bad |= !(isfinite(pr) && isfinite(pi));
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { rr[u] = nr[u]; ri[u] = ni[u]; fr[u] = gr[u]; fi[u] = gi[u]; }
    }
    if (bad) atomicOr(a.ovf + m, 1);
}

// grid: (yc, members of the chunk): row j of G (1 .. yc-2) and of S (0, yc-1); thread 0 also tests A, C, D, E, Fc at an interior j
__global__ void __launch_bounds__(XINV_GCHK_WG) k_fourier_gcheck(CFourierCheckArgs a)
{
    const int64_t j = blockIdx.x, m = a.member0 + blockIdx.y, yc = a.yc, xc = a.xc;
    const double u = a.undef;
    const bool edge = j == 0 || j == yc - 1;
    const double *row = (edge ? a.S + m * a.sS : a.G + m * a.sG) + j * xc;
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < xc; i += XINV_GCHK_WG) cnt += row[i] == u;
    if (threadIdx.x == 0 && !edge) {
#pragma unroll
        for (int q = 0; q < 5; q++) cnt += a.c[q][m * a.sc[q] + j] == u;
    }
    if (cnt) atomicAdd(a.bad + m, cnt);
}

#endif /* XINV_CFOURIER_KERNELS */

// xinv_tu_cfourier.hip
__attribute__((visibility("hidden"))) void xinv_launch_fourier_cfactor(CFourierFactorArgs a, int64_t nset, hipStream_t st);
__attribute__((visibility("hidden"))) void xinv_launch_fourier_csubst(CFourierSubstArgs a, int64_t nbatch, hipStream_t st);
__attribute__((visibility("hidden"))) void xinv_launch_fourier_gcheck(CFourierCheckArgs a, int64_t nbatch, hipStream_t st);
