// xinv_fourier.h -- the direct Fourier solve of the 2-D standard form for periodic x (include/xinv_fourier.h):
//   d/dy(A dS/dy) + d/dx(C dS/dx) = F,   B == 0,   A and C functions of y alone,   BCy fixed, BCx periodic, no mask.
// With coefficients constant along x the discrete operator (numbas.py:351-369 with B == 0) commutes with the cyclic shift
// along x, so a discrete Fourier transform along x turns it into one REAL tridiagonal system in y per zonal wavenumber k:
//   lo_j X[j-1] + di_jk X[j] + up_j X[j+1] = DFT(F[j,:] * delxSqr)[k],      j = 1 .. yc-2
//   lo_j = A[j] ratioSqr,  up_j = A[j+1] ratioSqr,  di_jk = -((A[j+1] + A[j]) ratioSqr + C[j] lambda_k),
//   lambda_k = 4 sin^2(pi k / xc)   (tabulated on the host: 2 - 2 cos loses half the digits at small k)
// with the known rows X[0] = DFT(S[0,:]) and X[yc-1] = DFT(S[yc-1,:]) moved to the right-hand sides of rows 1 and yc-2.
// The matrix is real: the real and imaginary parts of a wavenumber are two right-hand sides of one system.
//
// Three kernels.
//   k_rowdft<INVERSE>   mixed-radix Stockham transform (radices 4, 2, 3, 5) of real rows, TWO rows per workgroup packed into
//                       one complex transform z = x0 + i x1 of length n (rows of one member: what is large or non-finite in
//                       one row reaches its partner's rounding, never another member).  The pair stays in LDS from load to
//                       store (a ping-pong pair of n complex values: 32 n bytes, 115 KB at n = 3600 -- one workgroup per
//                       CU), twiddles come from a host-built table W[t] = exp(-2 pi i t / n) through vector loads.  Forward: real [n] -> half spectrum
//                       [K = n/2 + 1] complex (re, im interleaved), X0 = (Z[k] + conj Z[n-k]) / 2, X1 = (Z[k] - conj Z[n-k]) / 2i.
//                       Inverse: the reverse (Z rebuilt from the Hermitian halves; the imaginary parts of X[0] and X[n/2] are
//                       ignored as numpy.fft.irfft ignores them), by conj(DFT(conj Z)) / n -- one set of passes serves both.
//   k_fourier_tri       one wavenumber per lane, marching j: the Thomas recurrence without pivoting (|di| >= |lo| + |up| for
//                       positive A, C), both right-hand sides in the lane, loads and stores coalesced along k, one division
//                       per row.  The forward factors up_j / beta_j sit in the workspace; the right-hand sides are replaced in
//                       place by the forward result and then by the solution.  A non-finite solution sets the member's word.
//   k_fourier_check     counts `undef` among the points the solve reads; runs before anything is written.
// Two more for a plan (xinv_fourier_plan_*: one operator, many forcings), which keeps what depends on A, C, ratioSqr and xc alone:
//   k_fourier_factor    one wavenumber per lane and coefficient set, once per plan: k_fourier_tri's march without the
//                       right-hand sides, storing inv_j = 1 / beta_j and gamma_j = up_j inv_j -- the same expressions, the same bits.
//   k_fourier_subst     one lane per (wavenumber, real or imaginary part): the two parts are independent real recurrences
//                       with the same factors, so a member offers 2K lanes.  Forward rho_j = (r_j - lo_j rho_{j-1}) inv_j,
//                       backward x_j = rho_j - gamma_j x_{j+1}: no division; rows are loaded a batch ahead of the chain.
// and k_rowdft takes a per-member skip word (the plan's undef counts): a member that holds `undef` keeps its S.
// Rules of DESIGN 4.9: 64-bit indexing, solver data and tables through vector loads only, no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/xinv.h"

#define XINV_DFT_WG 256                  /* threads of a k_rowdft workgroup */
#define XINV_DFT_MAX_N 4096              /* LDS budget: 2 x n complex doubles = 32 n bytes <= 128 KiB of the CU's 160 */
#define XINV_DFT_MAX_PASS 12             /* 4096 = 4^6; 3^7 = 2187: seven passes at the most */
#define XINV_FTRI_WG 64                  /* k_fourier_tri: one wavefront per workgroup, one wavenumber per lane */
#define XINV_FCHK_WG 256
#define XINV_FFAC_WG 64                  /* k_fourier_factor: as k_fourier_tri */
#define XINV_FSUB_WG 64                  /* k_fourier_subst: one wavefront per workgroup, 2K lanes per member */
#define XINV_FSUB_AHEAD 8                /* ... rows loaded ahead of the dependent chain */

// Which rows a k_rowdft launch transforms and where they go: nrows / rpm members of rpm rows each, a workgroup per pair of
// rows (2p, 2p + 1) of ONE member (an odd rpm leaves the last row alone).  Row q of member m: real side at real +
// m * r_member + r_first + q * r_step, spectrum side at spec + m * s_member + s_first + q * s_step (all in doubles).  Forward reads `real` (times `scale`) and writes `spec`; inverse the reverse.
struct RowDftArgs {
    double *real;
    double *spec;
    const double *tw;                    // [n] complex: exp(-2 pi i t / n)
    int64_t nrows, rpm;
    int64_t r_member, r_first, r_step;
    int64_t s_member, s_first, s_step;
    double scale;                        // forward: applied to the real input (delxSqr; 1: exact)
    int n, npass;
    int radix[XINV_DFT_MAX_PASS];
    const int *skip;                     // null, or [members]: a workgroup whose member's word is not 0 does nothing
};

struct FourierTriArgs {
    double *spec;                        // [nbatch][yc][K] complex: rows 1 .. yc-2 right-hand sides -> solution; rows 0, yc-1 known
    double *gam;                         // workspace [nbatch][yc][K]: up_j / beta_j
    const double *A, *C;                 // one value per row, [nbatch or 1][yc]
    const double *lam;                   // [K]
    int64_t sA, sC;                      // member strides (0 = shared)
    int64_t yc, K, member0;
    double ratioSqr;
    int *ovf;                            // [nbatch]
};

// The factors of a plan: per coefficient set (one member's A, C, or the one shared pair) two planes [yc][K], inv then gamma.
struct FourierFactorArgs {
    double *fac;                         // [nset][2][yc][K]; rows 0 and yc-1 are not written
    const double *A, *C;                 // one value per row, [nset or 1][yc]
    const double *lam;                   // [K]
    int64_t sA, sC;                      // set strides (0 = shared)
    int64_t yc, K, set0;
    double ratioSqr;
};

struct FourierSubstArgs {
    double *spec;                        // [nbatch][yc][2K] doubles: as FourierTriArgs::spec
    const double *fac;                   // FourierFactorArgs::fac
    const double *A;                     // the plan's copy, [nbatch or 1][yc]: lo_j = A[j] ratioSqr
    int64_t sA, sfac;                    // member strides of A and of fac (0 = shared)
    int64_t yc, K, member0;
    double ratioSqr;
    int *ovf;                            // [nbatch]
};

struct FourierCheckArgs {
    const double *S, *A, *C, *F;
    int64_t sS, sA, sC, sF;
    int64_t yc, xc, member0;
    double undef;
    int *bad;                            // [nbatch]: how many of the points the solve reads hold `undef`
};

#ifdef XINV_FOURIER_KERNELS

struct xinv_c2 { double x, y; };

__device__ __forceinline__ xinv_c2 c_add(xinv_c2 a, xinv_c2 b) { return { a.x + b.x, a.y + b.y }; }
__device__ __forceinline__ xinv_c2 c_sub(xinv_c2 a, xinv_c2 b) { return { a.x - b.x, a.y - b.y }; }
__device__ __forceinline__ xinv_c2 c_mul(xinv_c2 a, xinv_c2 b) { return { a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x }; }
__device__ __forceinline__ xinv_c2 c_mnj(xinv_c2 a) { return { a.y, -a.x }; }          // a * (-i)
__device__ __forceinline__ xinv_c2 c_scl(xinv_c2 a, double s) { return { a.x * s, a.y * s }; }

// One Stockham pass of radix R over n points: butterfly j of n / R, with ns = the product of the earlier radices, reads
// in[j + r n/R], multiplies by W^(r k n / (ns R)), k = j % ns, and writes out[(j / ns) ns R + k + r ns].
template <int R>
__device__ __forceinline__ void xinv_dft_pass(const xinv_c2 *in, xinv_c2 *out, const double *tw, int n, int ns, int tid)
{
    const int nb = n / R, tstep = n / (ns * R);
    for (int j = tid; j < nb; j += XINV_DFT_WG) {
        const int k = j % ns, j0 = (j / ns) * ns * R + k;
        xinv_c2 v[R];
#pragma unroll
        for (int r = 0; r < R; r++) v[r] = in[j + r * nb];
        if (ns > 1) {
#pragma unroll
            for (int r = 1; r < R; r++) {
                const int64_t t = (int64_t)r * k * tstep;
                const xinv_c2 w = { tw[2 * t], tw[2 * t + 1] };
                v[r] = c_mul(v[r], w);
            }
        }
        if constexpr (R == 2) {
            out[j0] = c_add(v[0], v[1]);
            out[j0 + ns] = c_sub(v[0], v[1]);
        } else if constexpr (R == 4) {
            const xinv_c2 a = c_add(v[0], v[2]), b = c_sub(v[0], v[2]), c = c_add(v[1], v[3]), d = c_mnj(c_sub(v[1], v[3]));
            out[j0] = c_add(a, c);
            out[j0 + ns] = c_add(b, d);
            out[j0 + 2 * ns] = c_sub(a, c);
            out[j0 + 3 * ns] = c_sub(b, d);
        } else if constexpr (R == 3) {
            const double s3 = 0.86602540378443864676;                      // sin(2 pi / 3)
            const xinv_c2 t = c_add(v[1], v[2]), d = c_mnj(c_scl(c_sub(v[1], v[2]), s3));
            const xinv_c2 m = c_sub(v[0], c_scl(t, 0.5));
            out[j0] = c_add(v[0], t);
            out[j0 + ns] = c_add(m, d);
            out[j0 + 2 * ns] = c_sub(m, d);
        } else {
            const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;      // cos(2 pi / 5), cos(4 pi / 5)
            const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;       // sin(2 pi / 5), sin(4 pi / 5)
            const xinv_c2 a1 = c_add(v[1], v[4]), b1 = c_sub(v[1], v[4]), a2 = c_add(v[2], v[3]), b2 = c_sub(v[2], v[3]);
            const xinv_c2 m1 = c_add(v[0], c_add(c_scl(a1, c1), c_scl(a2, c2)));
            const xinv_c2 m2 = c_add(v[0], c_add(c_scl(a1, c2), c_scl(a2, c1)));
            const xinv_c2 d1 = c_mnj(c_add(c_scl(b1, s1), c_scl(b2, s2)));
            const xinv_c2 d2 = c_mnj(c_sub(c_scl(b1, s2), c_scl(b2, s1)));
            out[j0] = c_add(v[0], c_add(a1, a2));
            out[j0 + ns] = c_add(m1, d1);
            out[j0 + 2 * ns] = c_add(m2, d2);
            out[j0 + 3 * ns] = c_sub(m2, d2);
            out[j0 + 4 * ns] = c_sub(m1, d1);
        }
    }
}

template <bool INVERSE>
__global__ void __launch_bounds__(XINV_DFT_WG) k_rowdft(RowDftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xinv_dft_lds[];
    const int n = a.n, K = n / 2 + 1, tid = threadIdx.x;
    // a pair never straddles two members: a non-finite row spoils its partner, and must not leave its member
    const int64_t ppm = (a.rpm + 1) / 2, m0 = (int64_t)blockIdx.x / ppm, q0 = 2 * ((int64_t)blockIdx.x % ppm);
    // (the word was written by a kernel queued before this one: read through the coherent L2, never the scalar cache;
    // uniform over the workgroup, and before LDS or a barrier is touched)
    if (a.skip && __hip_atomic_load(a.skip + m0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    xinv_c2 *buf0 = (xinv_c2 *)xinv_dft_lds, *buf1 = buf0 + n;
    const bool two = q0 + 1 < a.rpm;
    double *x0 = a.real + m0 * a.r_member + a.r_first + q0 * a.r_step, *x1 = x0 + (two ? a.r_step : 0);
    double *X0 = a.spec + m0 * a.s_member + a.s_first + q0 * a.s_step, *X1 = X0 + (two ? a.s_step : 0);

    if constexpr (!INVERSE) {
        const double sc = a.scale;
        for (int i = tid; i < n; i += XINV_DFT_WG) buf0[i] = { x0[i] * sc, two ? x1[i] * sc : 0.0 };
    } else {
        // conj(Z), Z[k] = X0[k] + i X1[k] with X[n-k] = conj X[k]; the imaginary parts of X[0] and X[n/2] play no part
        for (int i = tid; i < n; i += XINV_DFT_WG) {
            const bool up = i >= K;
            const int k = up ? n - i : i;
            xinv_c2 p = { X0[2 * (int64_t)k], X0[2 * (int64_t)k + 1] };
            xinv_c2 q = { 0.0, 0.0 };
            if (two) q = { X1[2 * (int64_t)k], X1[2 * (int64_t)k + 1] };
            if (k == 0 || 2 * k == n) { p.y = 0.0; q.y = 0.0; }
            if (up) { p.y = -p.y; q.y = -q.y; }
            buf0[i] = { p.x - q.y, -(p.y + q.x) };
        }
    }
    __syncthreads();

    xinv_c2 *in = buf0, *out = buf1;
    int ns = 1;
    for (int p = 0; p < a.npass; p++) {
        const int R = a.radix[p];
        if (R == 4) xinv_dft_pass<4>(in, out, a.tw, n, ns, tid);
        else if (R == 2) xinv_dft_pass<2>(in, out, a.tw, n, ns, tid);
        else if (R == 3) xinv_dft_pass<3>(in, out, a.tw, n, ns, tid);
        else xinv_dft_pass<5>(in, out, a.tw, n, ns, tid);
        ns *= R;
        __syncthreads();
        xinv_c2 *t = in; in = out; out = t;
    }

    if constexpr (!INVERSE) {
        for (int k = tid; k < K; k += XINV_DFT_WG) {
            const xinv_c2 z = in[k], w = in[k == 0 ? 0 : n - k];
            X0[2 * (int64_t)k] = (z.x + w.x) * 0.5;
            X0[2 * (int64_t)k + 1] = (z.y - w.y) * 0.5;
            if (two) {
                X1[2 * (int64_t)k] = (z.y + w.y) * 0.5;
                X1[2 * (int64_t)k + 1] = (w.x - z.x) * 0.5;
            }
        }
    } else {
        const double dn = (double)n;
        for (int i = tid; i < n; i += XINV_DFT_WG) {
            const xinv_c2 z = in[i];                                   // conj of the inverse transform, unscaled
            x0[i] = z.x / dn;
            if (two) x1[i] = -z.y / dn;
        }
    }
}

// grid: (ceil(K / 64), members of the chunk)
__global__ void __launch_bounds__(XINV_FTRI_WG) k_fourier_tri(FourierTriArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * XINV_FTRI_WG + threadIdx.x, m = a.member0 + blockIdx.y;
    if (k >= a.K) return;
    const int64_t yc = a.yc, K = a.K;
    double *sp = a.spec + m * yc * K * 2 + 2 * k, *gm = a.gam + m * yc * K + k;
    const double *A = a.A + m * a.sA, *C = a.C + m * a.sC;
    const double lam = a.lam[k], rs = a.ratioSqr;

    // forward: rows ascending; the known row 0 goes to the right-hand side of row 1, row yc-1 to that of row yc-2
    double gp = 0.0, pr = sp[0], pi = sp[1];
    double Aj = A[1];
    for (int64_t j = 1; j <= yc - 2; j++) {
        const double Ap = A[j + 1], Cj = C[j];
        const double lo = Aj * rs, up = Ap * rs, di = -((Ap + Aj) * rs + Cj * lam);
        double rr = sp[2 * j * K], ri = sp[2 * j * K + 1];
        if (j == yc - 2) {
            rr = rr - up * sp[2 * (yc - 1) * K];
            ri = ri - up * sp[2 * (yc - 1) * K + 1];
        }
        const double inv = 1.0 / (j == 1 ? di : di - lo * gp);
        pr = (rr - lo * pr) * inv;
        pi = (ri - lo * pi) * inv;
        gp = up * inv;
        gm[j * K] = gp;
        sp[2 * j * K] = pr;
        sp[2 * j * K + 1] = pi;
        Aj = Ap;
    }
    // backward: row yc-2 stands
    int bad = !(isfinite(pr) && isfinite(pi));
    for (int64_t j = yc - 3; j >= 1; j--) {
        const double g = gm[j * K];
        pr = sp[2 * j * K] - g * pr;
        pi = sp[2 * j * K + 1] - g * pi;
        sp[2 * j * K] = pr;
        sp[2 * j * K + 1] = pi;
        bad |= !(isfinite(pr) && isfinite(pi));
    }
    if (bad) atomicOr(a.ovf + m, 1);
}

// grid: (ceil(K / 64), coefficient sets of the chunk).  The expressions of k_fourier_tri, operation by operation.
__global__ void __launch_bounds__(XINV_FFAC_WG) k_fourier_factor(FourierFactorArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * XINV_FFAC_WG + threadIdx.x, s = a.set0 + blockIdx.y;
    if (k >= a.K) return;
    const int64_t yc = a.yc, K = a.K;
    double *iv = a.fac + s * 2 * yc * K + k, *gm = iv + yc * K;
    const double *A = a.A + s * a.sA, *C = a.C + s * a.sC;
    const double lam = a.lam[k], rs = a.ratioSqr;
    double gp = 0.0, Aj = A[1];
    for (int64_t j = 1; j <= yc - 2; j++) {
        const double Ap = A[j + 1], Cj = C[j];
        const double lo = Aj * rs, up = Ap * rs, di = -((Ap + Aj) * rs + Cj * lam);
        const double inv = 1.0 / (j == 1 ? di : di - lo * gp);
        gp = up * inv;
        iv[j * K] = inv;
        gm[j * K] = gp;
        Aj = Ap;
    }
}

// grid: (ceil(2K / 64), members of the chunk).  Lane q marches the double at spec[(m yc + j) 2K + q] with the factors of
// wavenumber q >> 1.  The loads of a batch of rows do not depend on the chain: they are issued a batch ahead of it.
__global__ void __launch_bounds__(XINV_FSUB_WG) k_fourier_subst(FourierSubstArgs a)
{
    const int64_t q = (int64_t)blockIdx.x * XINV_FSUB_WG + threadIdx.x, m = a.member0 + blockIdx.y;
    const int64_t yc = a.yc, K = a.K, K2 = 2 * a.K;
    if (q >= K2) return;
    constexpr int U = XINV_FSUB_AHEAD;
    double *sp = a.spec + m * yc * K2 + q;
    const double *iv = a.fac + m * a.sfac + (q >> 1), *gm = iv + yc * K;
    const double *A = a.A + m * a.sA;
    const double rs = a.ratioSqr;

    // forward: rows ascending; the known row 0 enters through lo_1, row yc-1 through up on row yc-2
    const int64_t jl = yc - 2;
    const double last = sp[(yc - 1) * K2], upl = A[yc - 1] * rs;
    double p = sp[0];
    // (a batch's loads are unconditional -- past the march's end they read its last row again, unused -- and nothing in
    // the load phase uses a loaded value: no wait until the chain needs the row)
    double r[U], f[U], la[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t j = 1 + u <= jl ? 1 + u : jl;
        r[u] = sp[j * K2]; f[u] = iv[j * K]; la[u] = A[j];
    }
    for (int64_t j0 = 1; j0 <= jl; j0 += U) {
        double rn[U], fn[U], ln[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + U + u <= jl ? j0 + U + u : jl;
            rn[u] = sp[j * K2]; fn[u] = iv[j * K]; ln[u] = A[j];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + u;
            if (j <= jl) {
                double rr = r[u];
                if (j == jl) rr = rr - upl * last;
                const double lo = la[u] * rs;
                p = (rr - lo * p) * f[u];
                sp[j * K2] = p;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { r[u] = rn[u]; f[u] = fn[u]; la[u] = ln[u]; }
    }
    // backward: row yc-2 stands
    int bad = !isfinite(p);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t j = jl - 1 - u >= 1 ? jl - 1 - u : 1;
        r[u] = sp[j * K2]; f[u] = gm[j * K];
    }
    for (int64_t j0 = jl - 1; j0 >= 1; j0 -= U) {
        double rn[U], fn[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 - U - u >= 1 ? j0 - U - u : 1;
            rn[u] = sp[j * K2]; fn[u] = gm[j * K];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 - u;
            if (j >= 1) {
                p = r[u] - f[u] * p;
                sp[j * K2] = p;
                bad |= !isfinite(p);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { r[u] = rn[u]; f[u] = fn[u]; }
    }
    if (bad) atomicOr(a.ovf + m, 1);
}

// grid: (yc, members of the chunk): row j of F (1 .. yc-2) and of S (0, yc-1); thread 0 also tests A[j] (1 .. yc-1), C[j] (1 .. yc-2)
__global__ void __launch_bounds__(XINV_FCHK_WG) k_fourier_check(FourierCheckArgs a)
{
    const int64_t j = blockIdx.x, m = a.member0 + blockIdx.y, yc = a.yc, xc = a.xc;
    const double u = a.undef;
    const bool edge = j == 0 || j == yc - 1;
    const double *row = (edge ? a.S + m * a.sS : a.F + m * a.sF) + j * xc;
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < xc; i += XINV_FCHK_WG) cnt += row[i] == u;
    if (threadIdx.x == 0) {
        if (j >= 1) cnt += a.A[m * a.sA + j] == u;
        if (!edge) cnt += a.C[m * a.sC + j] == u;
    }
    if (cnt) atomicAdd(a.bad + m, cnt);
}

#endif /* XINV_FOURIER_KERNELS */

// The launch loop of every kernel of this family (and of xinv_cfourier.h) that takes a member, or a coefficient set, per
// blockIdx.y: one launch per chunk, with the chunk's first member in the arguments' `first` field (member0 / set0).
#define FOURIER_MEMBER_CHUNK 32768       /* members per launch (grid.y <= 65535) */
template <class Args>
static inline void xinv_launch_chunks(void (*kernel)(Args), Args a, int64_t Args::*first, int64_t members, unsigned gx,
                                      unsigned wg, hipStream_t st)
{
    for (int64_t m0 = 0; m0 < members; m0 += FOURIER_MEMBER_CHUNK) {
        const int64_t nm = members - m0 < FOURIER_MEMBER_CHUNK ? members - m0 : FOURIER_MEMBER_CHUNK;
        a.*first = m0;
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)nm), dim3(wg), 0, st, a);
    }
}

// xinv_tu_fourier.hip
__attribute__((visibility("hidden"))) int xinv_launch_rowdft(const RowDftArgs &a, bool inverse, hipStream_t st);
__attribute__((visibility("hidden"))) void xinv_launch_fourier_tri(FourierTriArgs a, int64_t nbatch, hipStream_t st);
__attribute__((visibility("hidden"))) void xinv_launch_fourier_check(FourierCheckArgs a, int64_t nbatch, hipStream_t st);
__attribute__((visibility("hidden"))) void xinv_launch_fourier_factor(FourierFactorArgs a, int64_t nset, hipStream_t st);
__attribute__((visibility("hidden"))) void xinv_launch_fourier_subst(FourierSubstArgs a, int64_t nbatch, hipStream_t st);
