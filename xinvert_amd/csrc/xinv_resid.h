// xinv_resid.h -- k_resid2d / k_resid3d: the residual R = L(S) - F of the five second-order forms, and its norms.
//
// A pure function of S: nothing is swept, S and the coefficients are only read, no 'extend' pre-pass runs.  At every
// point the reference's kernels update (numbas.py:312-399 and its siblings: rows / planes 1 .. n-2, columns 1 .. xc-2, and
// columns 0 and xc-1 when x is periodic, where the reference's operand predicate holds) R is the reference's `temp`
// before the relaxation scaling, divided by delxSqr (xinv_res_* in xinv_device.h); everywhere else R is `undef`.
//
// Streaming.  2-D: a workgroup of XINV_RESID_WG lanes owns that many consecutive columns and marches XINV_RESID_ROWS
// rows of one member; 3-D: a workgroup of 64 x 4 lanes owns a 4-row x 64-column patch and marches XINV_RESID_PLANES
// planes.  The marching direction's three values of S live in a rotating register window (2-D: for the lane's column
// and its two x neighbours; 3-D: for the lane's point), so a value of S comes from HBM once per strip plus the one-row
// (one-plane) halo at either end.  x neighbours (and, 3-D, the y neighbours of the current plane) are plain vector loads
// of addresses the neighbouring lane loads in the same instruction: they are served by the vector L1 from the line that
// is being fetched anyway.  No lane shift and no LDS stage: the periodic wrap, odd xc and the strip edges are index
// arithmetic (im / ip), with no halo lanes and no unaligned strips.  A coefficient that the expression reads at two
// rows (A of the standard forms) is read per point; the second read is an L1 / L2 hit.  R is written once.
//
// Norms per member over the live points: [n_live, mean|R|, max|R|, max|F|] (F: the forcing array of the form).  Every
// workgroup reduces its lanes in a fixed tree in LDS and writes four doubles into its own slot; k_resid_final adds the
// slots of a member in slot order.  No floating-point atomics; the same launch gives the same bits.  A NaN residual
// at a live point makes mean|R| and max|R| NaN; a member without live points has mean|R| = NaN and both maxima 0.
//
// All indexing is 64-bit.  Loads of lanes past xc (or past yc in 3-D) are clamped to the last column (row): every
// address formed lies inside the member.
#pragma once
#include "xinv_device.h"

#define XINV_RESID_WG 256        /* 2-D: lanes (= columns) per workgroup */
#define XINV_RESID_ROWS 16       /* 2-D: rows a workgroup marches */
#define XINV_RESID_PLANES 8      /* 3-D: planes a workgroup marches */
#define XINV_RESID_TX 64         /* 3-D: patch columns */
#define XINV_RESID_TY 4          /* 3-D: patch rows */

enum { RESID_STD2D = 0, RESID_GEN2D = 1, RESID_STD2DT = 2, RESID_STD3D = 3, RESID_GEN3D = 4 };

struct ResidArgs {
    double *R;
    const double *S;
    const double *c[8];        // the form's arrays, the forcing last (c[1] may be NULL in the 5-point variants)
    int64_t sR, sS, sc[8];     // batch strides in elements (0 = shared; not R)
    int64_t zc, yc, xc;
    int per;                   // periodic x
    int nstrip;                // 3-D: plane strips per member (blockIdx.z = member * nstrip + strip)
    int64_t member0;           // first member of this launch
    XinvScal sc_;
    double *part;              // [nbatch][nslot][4] partial norms, or NULL: no norms wanted
    int64_t nslot;
};

// Launches for members [0, nbatch) in chunks (grid.z is limited to 65535), then, with a.part, the final reducer into
// `norms` (device, [nbatch][4]).  nine: B is an array (2-D standard / general forms).  Returns 1 for a shape whose grid
// does not fit, 0 otherwise.
__attribute__((visibility("hidden"))) int xinv_launch_resid(int form, bool nine, ResidArgs a, int64_t nbatch, double *norms,
                                                            hipStream_t st);
// slots per member for a shape (what `part` must hold: nbatch * slots * 4 doubles)
static inline int64_t xinv_resid_slots(bool threed, int64_t zc, int64_t yc, int64_t xc)
{
    if (!threed)
        return ((xc + XINV_RESID_WG - 1) / XINV_RESID_WG) * ((yc + XINV_RESID_ROWS - 1) / XINV_RESID_ROWS);
    return ((xc + XINV_RESID_TX - 1) / XINV_RESID_TX) * ((yc + XINV_RESID_TY - 1) / XINV_RESID_TY) *
           ((zc + XINV_RESID_PLANES - 1) / XINV_RESID_PLANES);
}

#ifdef XINV_RESID_KERNELS      /* the kernels: xinv_tu_resid.hip only (the host driver sees the launcher above) */
// max of two magnitudes that keeps a NaN whichever side it comes from (the order of a reduction must not matter)
__device__ __forceinline__ double xinv_resid_max(double a, double b)
{
    return (a != a || b != b) ? (double)NAN : (a > b ? a : b);
}

// {count, sum|R|, max|R|, max|F|} of the NT lanes of a workgroup, combined in a fixed tree; valid in thread 0
template <int NT>
__device__ __forceinline__ void xinv_resid_block_reduce(int t, double &n, double &s, double &mr, double &mf)
{
    __shared__ double ln[NT], ls[NT], lr[NT], lf[NT];
    ln[t] = n; ls[t] = s; lr[t] = mr; lf[t] = mf;
    __syncthreads();
#pragma unroll
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) {
            ln[t] += ln[t + h];
            ls[t] += ls[t + h];
            lr[t] = xinv_resid_max(lr[t], lr[t + h]);
            lf[t] = xinv_resid_max(lf[t], lf[t + h]);
        }
        __syncthreads();
    }
    n = ln[0]; s = ls[0]; mr = lr[0]; mf = lf[0];
}

// ------------------------------------------------------------------------------------------------ 2-D
// w[a][b]: rows j-1, j, j+1 (a = 0, 1, 2) x columns im, i, ip (b = 0, 1, 2).  r, rp, rm: element offsets of rows j, j+1,
// j-1.  Returns the reference's predicate; res = the residual, f = the forcing at the point.
template <int FORM, bool NINE> struct Resid2D;

template <bool NINE> struct Resid2D<RESID_STD2D, NINE> {
    static __device__ __forceinline__ bool point(const double *const (&c)[8], const double (&w)[3][3], int64_t r,
                                                 int64_t rp, int64_t rm, int64_t i, int64_t im, int64_t ip, bool west,
                                                 const XinvScal &sc, double &res, double &f)
    {
        const double *A = c[0], *B = c[1], *C = c[2], *F = c[3];
        f = F[r + i];
        if (NINE)
            return xinv_res_std2d_9(res, w[1][1], w[2][1], w[0][1], w[1][0], w[1][2], w[2][2], w[2][0], w[0][2], w[0][0],
                                    west ? w[0][1] : w[0][2],
                                    A[rp + i], A[r + i], B[r + ip], B[r + im], B[rp + i], B[rp + (west ? ip : i)],
                                    B[rm + i], C[r + ip], C[r + i], f, sc);
        return xinv_res_std2d_5(res, w[1][1], w[2][1], w[0][1], w[1][0], w[1][2], A[rp + i], A[r + i], C[r + ip],
                                C[r + i], f, sc);
    }
};

template <bool NINE> struct Resid2D<RESID_GEN2D, NINE> {
    static __device__ __forceinline__ bool point(const double *const (&c)[8], const double (&w)[3][3], int64_t r,
                                                 int64_t rp, int64_t rm, int64_t i, int64_t im, int64_t ip, bool west,
                                                 const XinvScal &sc, double &res, double &f)
    {
        const int64_t p = r + i;
        f = c[6][p];
        if (NINE)
            return xinv_res_gen2d_9(res, w[1][1], w[2][1], w[0][1], w[1][0], w[1][2], w[2][2], w[2][0], w[0][2], w[0][0],
                                    c[0][p], c[1][p], c[2][p], c[3][p], c[4][p], c[5][p], f, sc);
        return xinv_res_gen2d_5(res, w[1][1], w[2][1], w[0][1], w[1][0], w[1][2], c[0][p], c[2][p], c[3][p], c[4][p],
                                c[5][p], f, sc);
    }
};

template <bool NINE> struct Resid2D<RESID_STD2DT, NINE> {
    static __device__ __forceinline__ bool point(const double *const (&c)[8], const double (&w)[3][3], int64_t r,
                                                 int64_t rp, int64_t rm, int64_t i, int64_t im, int64_t ip, bool west,
                                                 const XinvScal &sc, double &res, double &f)
    {
        const double *A = c[0], *B = c[1], *C = c[2], *D = c[3], *E = c[4], *F = c[5];
        f = F[r + i];
        return xinv_res_std2dt_9(res, w[1][1], w[2][1], w[0][1], w[1][0], w[1][2], w[2][2], w[2][0], w[0][2], w[0][0],
                                 west ? w[0][1] : w[0][2],
                                 A[rp + i], A[r + i], B[rp + i], B[rp + (west ? ip : i)], B[rm + i],
                                 C[r + ip], C[r + im], D[r + ip], D[r + i], E[r + i], f, sc);
    }
};

// grid: x over blocks of XINV_RESID_WG columns, y over strips of XINV_RESID_ROWS rows (all rows 0 .. yc-1), z over members
template <int FORM, bool NINE>
__global__ __launch_bounds__(XINV_RESID_WG) void k_resid2d(ResidArgs a)
{
    const int t = threadIdx.x;
    const int64_t m = a.member0 + blockIdx.z;
    const int64_t xc = a.xc, yc = a.yc;
    const int64_t col = (int64_t)blockIdx.x * XINV_RESID_WG + t;
    const bool incol = col < xc;
    const int64_t i = incol ? col : xc - 1;
    const int64_t im = (i == 0) ? xc - 1 : i - 1;
    const int64_t ip = (i == xc - 1) ? 0 : i + 1;
    const bool colok = incol && (a.per || (i >= 1 && i <= xc - 2));
    const bool west = (i == 0);
    const int64_t j0 = (int64_t)blockIdx.y * XINV_RESID_ROWS;
    const int64_t j1 = (j0 + XINV_RESID_ROWS < yc) ? j0 + XINV_RESID_ROWS : yc;
    const double *S = a.S + m * a.sS;
    double *R = a.R + m * a.sR;
    const double *c[8];
#pragma unroll
    for (int q = 0; q < 8; q++) c[q] = a.c[q] ? a.c[q] + m * a.sc[q] : nullptr;
    const double u = a.sc_.undef;

    double w[3][3];
    {
        const int64_t ra = (j0 > 0 ? j0 - 1 : 0) * xc, rb = j0 * xc;
        w[1][0] = S[ra + im]; w[1][1] = S[ra + i]; w[1][2] = S[ra + ip];
        w[2][0] = S[rb + im]; w[2][1] = S[rb + i]; w[2][2] = S[rb + ip];
    }
    double n = 0.0, s = 0.0, mr = 0.0, mf = 0.0;
    for (int64_t j = j0; j < j1; j++) {
#pragma unroll
        for (int b = 0; b < 3; b++) { w[0][b] = w[1][b]; w[1][b] = w[2][b]; }
        const int64_t jn = (j + 1 < yc) ? j + 1 : yc - 1;
        w[2][0] = S[jn * xc + im]; w[2][1] = S[jn * xc + i]; w[2][2] = S[jn * xc + ip];
        double out = u;
        if (colok && j >= 1 && j <= yc - 2) {
            double res, f;
            const int64_t r = j * xc;
            if (Resid2D<FORM, NINE>::point(c, w, r, r + xc, r - xc, i, im, ip, west, a.sc_, res, f)) {
                out = res;
                const double ar = fabs(res);
                n += 1.0; s += ar;
                mr = xinv_resid_max(mr, ar);
                mf = xinv_resid_max(mf, fabs(f));
            }
        }
        if (incol) R[j * xc + i] = out;
    }
    if (!a.part) return;
    xinv_resid_block_reduce<XINV_RESID_WG>(t, n, s, mr, mf);
    if (t == 0) {
        double *o = a.part + (m * a.nslot + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
        o[0] = n; o[1] = s; o[2] = mr; o[3] = mf;
    }
}

// ------------------------------------------------------------------------------------------------ 3-D
// grid: x over blocks of 64 columns, y over blocks of 4 rows (all rows), z over (member, strip of XINV_RESID_PLANES planes)
template <int FORM>
__global__ __launch_bounds__(XINV_RESID_TX * XINV_RESID_TY) void k_resid3d(ResidArgs a)
{
    const int t = threadIdx.y * XINV_RESID_TX + threadIdx.x;
    const int64_t m = a.member0 + blockIdx.z / a.nstrip;
    const int64_t strip = blockIdx.z % a.nstrip;
    const int64_t xc = a.xc, yc = a.yc, zc = a.zc, P = yc * xc;
    const int64_t col = (int64_t)blockIdx.x * XINV_RESID_TX + threadIdx.x;
    const int64_t row = (int64_t)blockIdx.y * XINV_RESID_TY + threadIdx.y;
    const bool inside = col < xc && row < yc;
    const int64_t i = col < xc ? col : xc - 1;
    const int64_t j = row < yc ? row : yc - 1;
    const int64_t im = (i == 0) ? xc - 1 : i - 1;
    const int64_t ip = (i == xc - 1) ? 0 : i + 1;
    const int64_t jm = (j > 0) ? j - 1 : 0, jp = (j < yc - 1) ? j + 1 : yc - 1;
    const bool ptok = inside && j >= 1 && j <= yc - 2 && (a.per || (i >= 1 && i <= xc - 2));
    const int64_t k0 = strip * XINV_RESID_PLANES;
    const int64_t k1 = (k0 + XINV_RESID_PLANES < zc) ? k0 + XINV_RESID_PLANES : zc;
    const double *S = a.S + m * a.sS;
    double *R = a.R + m * a.sR;
    const double *c[8];
#pragma unroll
    for (int q = 0; q < 8; q++) c[q] = a.c[q] ? a.c[q] + m * a.sc[q] : nullptr;
    const double u = a.sc_.undef;
    const int64_t q0 = j * xc + i;                                   // the lane's point inside a plane

    double sM, sC = S[(k0 > 0 ? k0 - 1 : 0) * P + q0], sP = S[k0 * P + q0];
    double n = 0.0, s = 0.0, mr = 0.0, mf = 0.0;
    for (int64_t k = k0; k < k1; k++) {
        sM = sC; sC = sP;
        sP = S[((k + 1 < zc) ? k + 1 : zc - 1) * P + q0];
        double out = u;
        if (ptok && k >= 1 && k <= zc - 2) {
            const int64_t pl = k * P, r = pl + j * xc, p = r + i;
            const double sJP = S[pl + jp * xc + i], sJM = S[pl + jm * xc + i], sE = S[r + ip], sW = S[r + im];
            double res, f;
            bool cond;
            if (FORM == RESID_STD3D) {
                f = c[3][p];
                cond = xinv_res_std3d(res, sC, sP, sM, sJP, sJM, sE, sW, c[0][p + P], c[0][p], c[1][p + xc], c[1][p],
                                      c[2][r + ip], c[2][p], f, a.sc_);
            } else {
                f = c[7][p];
                cond = xinv_res_gen3d(res, sC, sP, sM, sJP, sJM, sE, sW, c[0][p], c[1][p], c[2][p], c[3][p], c[4][p],
                                      c[5][p], c[6][p], f, i != 0, a.sc_);
            }
            if (cond) {
                out = res;
                const double ar = fabs(res);
                n += 1.0; s += ar;
                mr = xinv_resid_max(mr, ar);
                mf = xinv_resid_max(mf, fabs(f));
            }
        }
        if (inside) R[k * P + q0] = out;
    }
    if (!a.part) return;
    xinv_resid_block_reduce<XINV_RESID_TX * XINV_RESID_TY>(t, n, s, mr, mf);
    if (t == 0) {
        double *o = a.part + (m * a.nslot + (strip * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4;
        o[0] = n; o[1] = s; o[2] = mr; o[3] = mf;
    }
}

// the slots of one member added in slot order (64 lanes: lane t takes slots t, t + 64, ...; then the same fixed tree)
// -> norms[m] = {n_live, mean|R|, max|R|, max|F|}
__global__ __launch_bounds__(64) void k_resid_final(const double *part, int64_t nslot, double *norms, int64_t member0)
{
    const int t = threadIdx.x;
    const int64_t m = member0 + blockIdx.x;
    const double *p = part + m * nslot * 4;
    double n = 0.0, s = 0.0, mr = 0.0, mf = 0.0;
    for (int64_t q = t; q < nslot; q += 64) {
        n += p[q * 4]; s += p[q * 4 + 1];
        mr = xinv_resid_max(mr, p[q * 4 + 2]);
        mf = xinv_resid_max(mf, p[q * 4 + 3]);
    }
    xinv_resid_block_reduce<64>(t, n, s, mr, mf);
    if (t == 0) {
        double *o = norms + m * 4;
        o[0] = n; o[1] = (n != 0.0) ? s / n : (double)NAN; o[2] = mr; o[3] = mf;
    }
}
#endif /* XINV_RESID_KERNELS */
