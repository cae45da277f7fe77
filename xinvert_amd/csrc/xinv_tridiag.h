// xinv_tridiag.h -- k_tridiag: the reference's tridiagonal direct solver, numbas.trace / numbas.traceCyclic
// (numbas.py:1589-1685), one system per lane, and on top of it the direct solve of the 1-D standard form
//   d/dx(A dS/dx) + B S = F
// (XINV_PATH_DIRECT1D: the fixed point the SOR sweeps of numbas.py:683-725 converge to).
//
// Arithmetic.  The reference's recurrence, expression by expression, in its loop order, without contraction:
//   buf0[0] = b[0];  buf1[0] = c[0] / b[0];  buf0[i] = b[i] - a[i-1] * buf1[i-1];  buf1[i] = c[i] / buf0[i]
//   res[0] = d[0] / buf0[0];  res[i] = (d[i] - a[i-1] * res[i-1]) / buf0[i]                (forward, i ascending)
//   res[i] -= buf1[i] * res[i+1]                                                           (backward, i = N-2 .. 0)
// traceCyclic is three such solves over the same a, b, c -- right-hand sides (0, .., 0, cn), (a0, 0, .., 0) and d: they
// share buf0 / buf1 and run side by side in one forward and one backward pass -- plus the closing formulas of
// numbas.py:1678-1683.  No cyclic reduction, no scan: a lane is the reference's loop, so the result is its bits.
//
// Layout.  The caller's [nbatch][n], x fastest, one base pointer and one batch stride per array (0 = shared).  A
// workgroup is one wavefront and owns XINV_TRI_SYS = 64 consecutive systems.  Lane-per-system access to that layout is
// strided, so the systems move between HBM and LDS in chunks of 64 systems x XINV_TRI_T points: the loader maps the
// wavefront onto (system, point) = (idx / T, idx % T) -- every system's T points are one contiguous 128-byte piece --
// and writes four tiles [64][T + 1] (the odd row stride keeps the 64 lanes of a march step on distinct banks).  Each
// lane then marches its own row; the results replace the inputs of the same row in place (a row's inputs are in
// registers before its outputs are written) and leave with the same coalesced mapping.  The forward pass keeps buf1
// (and, cyclic, the two auxiliary solves) in a workspace the library owns and the forward result in x; the backward
// pass walks the chunks in reverse; the cyclic closing pass is elementwise.
//
// The 1-D standard form (FUSED).  The tiles hold S0, A (T + 1 points: row i reads A[i+1]), B, F and the row of the
// system is assembled in registers when the lane reaches it; no a, b, c, d array exists.  Rows default to identity
// (x[i] = S0[i]).  Live rows -- i in 1 .. xc-2, and 0 and xc-1 when periodic, with the reference's predicate F[i], A[i],
// A[i+1], B[i] != undef --: lower A[i] / delxSqr, upper A[i+1] / delxSqr, diagonal B[i] - (A[i+1] + A[i]) / delxSqr,
// right-hand side F[i].  'extend': row 0 is x[0] - x[1] = 0 when S0[1] != undef, row xc-1 is x[xc-1] - x[xc-2] = 0 when
// S0[xc-2] != undef.  'periodic': a0 = row 0's lower, cn = row xc-1's upper; the cyclic closing applies to the members
// whose two end rows are live; where an end row is an identity row, the other end's wrap term times that known value
// moves to the right-hand side and the plain solve stands.  A non-finite result sets the member's overflow word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/xinv.h"

#define XINV_TRI_SYS 64                 /* systems per workgroup: one per lane of its one wavefront */
#define XINV_TRI_T 16                   /* points per chunk: 16 doubles = one 128-byte line per system */
#define XINV_TRI_LD (XINV_TRI_T + 1)    /* tile row stride in doubles (odd) */

struct TridiagArgs {
    double *x;                          // [nbatch][n] the solution (FUSED: S, the first guess on entry)
    const double *p[4];                 // a, b, c, d (FUSED: A, B, F, unused)
    int64_t sx, sp[4];                  // batch strides in elements (0 = one copy shared by every system)
    const double *a0, *cn;              // cyclic corners, one value per system (not FUSED)
    int64_t sa0, scn;
    double *wg, *wu, *wv;               // workspace [nbatch][n]: buf1; cyclic: the two auxiliary solves
    int *ovf;                           // FUSED: [nbatch], 1 = the member's result holds a non-finite value
    int64_t nbatch, n;
    double delxSqr, undef;              // FUSED
    int ext;                            // FUSED: 'extend'
};

// 64 systems x `ncol` points starting at point `first` of every system, HBM -> tile; points outside [lo, hi) and
// systems past the batch read as 0.
__device__ __forceinline__ void xinv_tri_load(double *tile, const double *base, int64_t stride, int64_t m0, int64_t nbatch,
                                              int64_t first, int64_t lo, int64_t hi, int lane)
{
#pragma unroll
    for (int k = 0; k < XINV_TRI_T; k++) {
        const int idx = k * 64 + lane, r = idx / XINV_TRI_T, col = idx % XINV_TRI_T;
        const int64_t i = first + col, m = m0 + r;
        tile[r * XINV_TRI_LD + col] = (m < nbatch && i >= lo && i < hi) ? base[m * stride + i] : 0.0;
    }
}

// tile -> HBM, points [first, first + T) of every system that lie below `hi`
__device__ __forceinline__ void xinv_tri_store(const double *tile, double *base, int64_t stride, int64_t m0, int64_t nbatch,
                                               int64_t first, int64_t hi, int lane)
{
#pragma unroll
    for (int k = 0; k < XINV_TRI_T; k++) {
        const int idx = k * 64 + lane, r = idx / XINV_TRI_T, col = idx % XINV_TRI_T;
        const int64_t i = first + col, m = m0 + r;
        if (m < nbatch && i < hi) base[m * stride + i] = tile[r * XINV_TRI_LD + col];
    }
}

template <bool FUSED, bool CYC>
__global__ void __launch_bounds__(XINV_TRI_SYS) k_tridiag(TridiagArgs a)
{
    // FUSED: A | B | F | S0; otherwise a[i-1] | b | c | d.  After a row's step: u | buf1 | v | res (u, v: cyclic).
    __shared__ double t0[XINV_TRI_SYS * XINV_TRI_LD], t1[XINV_TRI_SYS * XINV_TRI_LD], t2[XINV_TRI_SYS * XINV_TRI_LD],
        t3[XINV_TRI_SYS * XINV_TRI_LD];
    __shared__ double l_r0[XINV_TRI_SYS], l_rn[XINV_TRI_SYS];
    __shared__ int l_cyc[XINV_TRI_SYS], l_ovf[XINV_TRI_SYS];
    const int lane = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * XINV_TRI_SYS, nb = a.nbatch, n = a.n;
    const int64_t m = m0 + lane < nb ? m0 + lane : nb - 1;       // (a tail lane marches the last system and stores nothing)
    const int64_t nchunk = (n + XINV_TRI_T - 1) / XINV_TRI_T;
    const double dsq = a.delxSqr, undef = a.undef;
    double *row0 = t0 + lane * XINV_TRI_LD, *row1 = t1 + lane * XINV_TRI_LD, *row2 = t2 + lane * XINV_TRI_LD,
           *row3 = t3 + lane * XINV_TRI_LD;

    // what a lane knows of its system before the march: the cyclic corners, or the end rows of the 1-D form
    double a0 = 0.0, cn = 0.0, sFirst = 0.0, sLast = 0.0;
    bool cyc = CYC, ext0 = false, extN = false, wrap0 = false, wrapN = false;
    if constexpr (FUSED) {
        const double *Sg = a.x + m * a.sx;
        if (a.ext) {
            ext0 = Sg[1] != undef;
            extN = Sg[n - 2] != undef;
        }
        if constexpr (CYC) {
            const double *Ag = a.p[0] + m * a.sp[0], *Bg = a.p[1] + m * a.sp[1], *Fg = a.p[2] + m * a.sp[2];
            const double A0 = Ag[0];
            const bool live0 = Fg[0] != undef && A0 != undef && Ag[1] != undef && Bg[0] != undef;
            const bool liveN = Fg[n - 1] != undef && Ag[n - 1] != undef && A0 != undef && Bg[n - 1] != undef;
            cyc = live0 && liveN;
            wrap0 = live0 && !liveN;                            // x[n-1] = S0[n-1] is known: row 0's wrap term moves right
            wrapN = liveN && !live0;
            sFirst = Sg[0];
            sLast = Sg[n - 1];
        }
    } else if constexpr (CYC) {
        a0 = a.a0[m * a.sa0];
        cn = a.cn[m * a.scn];
    }
    l_ovf[lane] = 0;

    // ---- forward: chunks ascending
    double gp = 0.0, wp = 0.0, up = 0.0, vp = 0.0;              // buf1[i-1] and res[i-1] of the three solves
    for (int64_t ch = 0; ch < nchunk; ch++) {
        const int64_t f = ch * XINV_TRI_T;
        if constexpr (FUSED) {
            xinv_tri_load(t0, a.p[0], a.sp[0], m0, nb, f, 0, n, lane);
            xinv_tri_load(t1, a.p[1], a.sp[1], m0, nb, f, 0, n, lane);
            xinv_tri_load(t2, a.p[2], a.sp[2], m0, nb, f, 0, n, lane);
            xinv_tri_load(t3, a.x, a.sx, m0, nb, f, 0, n, lane);
            // A one past the chunk (periodic: A[n] is A[0])
            const int64_t ih = f + XINV_TRI_T;
            const double *Ag = a.p[0] + m * a.sp[0];
            row0[XINV_TRI_T] = ih < n ? Ag[ih] : ((CYC && ih == n) ? Ag[0] : 0.0);
        } else {
            xinv_tri_load(t0, a.p[0], a.sp[0], m0, nb, f - 1, 0, n - 1, lane);
            xinv_tri_load(t1, a.p[1], a.sp[1], m0, nb, f, 0, n, lane);
            xinv_tri_load(t2, a.p[2], a.sp[2], m0, nb, f, 0, n - 1, lane);
            xinv_tri_load(t3, a.p[3], a.sp[3], m0, nb, f, 0, n, lane);
        }
        __syncthreads();
        const int cols = (int)(n - f < XINV_TRI_T ? n - f : XINV_TRI_T);
        for (int j = 0; j < cols; j++) {
            const int64_t i = f + j;
            double lo, di, hi, rh;
            if constexpr (FUSED) {
                const double Ai = row0[j], Bi = row1[j], Fi = row2[j], s0 = row3[j];
                // (periodic, the chunk ends at n exactly: row n-1 reads A[0] from the halo; inside a chunk A[n] is A[0] too)
                double Aip = row0[j + 1];
                if (CYC && i == n - 1 && j + 1 < XINV_TRI_T) Aip = a.p[0][m * a.sp[0]];
                const bool inner = (i >= 1 && i <= n - 2) || CYC;
                lo = 0.0; di = 1.0; hi = 0.0; rh = s0;
                if (inner && Fi != undef && Ai != undef && Aip != undef && Bi != undef) {
                    lo = Ai / dsq;
                    hi = Aip / dsq;
                    di = Bi - (Aip + Ai) / dsq;
                    rh = Fi;
                    if (CYC && i == 0) { a0 = lo; if (wrap0) rh = Fi - lo * sLast; }
                    if (CYC && i == n - 1) { cn = hi; if (wrapN) rh = Fi - hi * sFirst; }
                }
                if (i == 0 && ext0) { di = 1.0; hi = -1.0; rh = 0.0; }
                if (i == n - 1 && extN) { lo = -1.0; di = 1.0; rh = 0.0; }
            } else {
                lo = row0[j]; di = row1[j]; hi = row2[j]; rh = row3[j];
            }
            const double buf0 = i == 0 ? di : di - lo * gp;
            gp = hi / buf0;
            wp = i == 0 ? rh / buf0 : (rh - lo * wp) / buf0;
            row1[j] = gp;
            row3[j] = wp;
            if constexpr (CYC) {
                const double ru = i == n - 1 ? cn : 0.0, rv = i == 0 ? a0 : 0.0;
                up = i == 0 ? ru / buf0 : (ru - lo * up) / buf0;
                vp = i == 0 ? rv / buf0 : (rv - lo * vp) / buf0;
                row0[j] = up;
                row2[j] = vp;
            }
        }
        __syncthreads();
        xinv_tri_store(t1, a.wg, n, m0, nb, f, n, lane);
        xinv_tri_store(t3, a.x, a.sx, m0, nb, f, n, lane);
        if constexpr (CYC) {
            xinv_tri_store(t0, a.wu, n, m0, nb, f, n, lane);
            xinv_tri_store(t2, a.wv, n, m0, nb, f, n, lane);
        }
        __syncthreads();
    }

    // ---- backward: chunks descending; res[n-1] stands
    const double wN = wp, uN = up, vN = vp;
    int bad = 0;
    for (int64_t ch = nchunk - 1; ch >= 0; ch--) {
        const int64_t f = ch * XINV_TRI_T;
        xinv_tri_load(t1, a.wg, n, m0, nb, f, 0, n, lane);
        xinv_tri_load(t3, a.x, a.sx, m0, nb, f, 0, n, lane);
        if constexpr (CYC) {
            xinv_tri_load(t0, a.wu, n, m0, nb, f, 0, n, lane);
            xinv_tri_load(t2, a.wv, n, m0, nb, f, 0, n, lane);
        }
        __syncthreads();
        const int cols = (int)(n - f < XINV_TRI_T ? n - f : XINV_TRI_T);
        for (int j = cols - 1; j >= 0; j--) {
            const int64_t i = f + j;
            if (i < n - 1) {
                const double g = row1[j];
                wp = row3[j] - g * wp;
                row3[j] = wp;
                if constexpr (CYC) {
                    up = row0[j] - g * up;
                    vp = row2[j] - g * vp;
                    row0[j] = up;
                    row2[j] = vp;
                }
            }
            if (!CYC && !isfinite(wp)) bad = 1;
        }
        __syncthreads();
        xinv_tri_store(t3, a.x, a.sx, m0, nb, f, n, lane);
        if constexpr (CYC) {
            xinv_tri_store(t0, a.wu, n, m0, nb, f, n, lane);
            xinv_tri_store(t2, a.wv, n, m0, nb, f, n, lane);
        }
        __syncthreads();
    }

    // ---- cyclic closing (numbas.py:1678-1683), elementwise over the chunks
    if constexpr (CYC) {
        const double w0 = wp, u0 = up, v0 = vp;
        const double rn = ((1.0 + u0) / uN * wN - w0) / ((1.0 + u0) * (1.0 + vN) / uN - v0);
        const double r0 = (w0 - v0 * rn) / (1 + u0);
        l_r0[lane] = r0;
        l_rn[lane] = rn;
        l_cyc[lane] = cyc;
        __syncthreads();
        for (int64_t ch = 0; ch < nchunk; ch++) {
            const int64_t f = ch * XINV_TRI_T;
#pragma unroll
            for (int k = 0; k < XINV_TRI_T; k++) {
                const int idx = k * 64 + lane, r = idx / XINV_TRI_T, col = idx % XINV_TRI_T;
                const int64_t i = f + col, mm = m0 + r;
                if (mm < nb && i < n) {
                    double v = a.x[mm * a.sx + i];
                    if (l_cyc[r]) {
                        const double R0 = l_r0[r], RN = l_rn[r];
                        v = i == 0 ? R0 : i == n - 1 ? RN : v - a.wu[mm * n + i] * R0 - a.wv[mm * n + i] * RN;
                        a.x[mm * a.sx + i] = v;
                    }
                    if (!isfinite(v)) l_ovf[r] = 1;
                }
            }
        }
        __syncthreads();
        bad = l_ovf[lane];
    }
    if (FUSED && m0 + lane < nb) a.ovf[m0 + lane] = bad;
}

// xinv_tu_tridiag.hip: the passes of one solve over every system
__attribute__((visibility("hidden"))) void xinv_launch_tridiag(const TridiagArgs &a, bool fused, bool cyclic, hipStream_t st);
