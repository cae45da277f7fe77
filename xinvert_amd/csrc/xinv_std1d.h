// xinv_std1d.h -- k_std1d: the 1-D standard form (reference numbas.invert_standard_1D, numbas.py:633-742),
//   d/dx(A dS/dx) + B S = F,
// solved register-resident: one member per wavefront (or per workgroup of up to 16 wavefronts), every sweep of a launch
// -- point updates, norm, stop rule -- inside the kernel.  1-D members never need a grid-wide barrier.
//
// Layout.  Lane l of wave w holds the contiguous chunk of points g = (64 w + l) * PPL + k, k = 0 .. PPL-1 (PPL even).
// Per point it keeps S, A[g], B[g], F[g], the relaxation factor optArg / ((A[g+1] + A[g]) / delxSqr - B[g]) (evaluated
// once per launch with the reference's expression: the bits of evaluating it every sweep) and the update predicate
// F, A[g], A[g+1], B != undef (bit k of a mask), plus A at the chunk's end + 1.  Shape, a function of xc alone:
//   xc <= 512: one wavefront, PPL = the smallest of 2, 4, 8 with 64 PPL >= xc (four members per workgroup);
//   xc  > 512: PPL = 8, W = ceil(xc / 512) wavefronts of one workgroup, chunk ends crossing between them through LDS;
//   xc  > XINV_STD1D_MAX_XC = 16 x 64 x 8 = 8192: XINV_ERR_ARG (an SOR sweep count is not practical there anyway).
// (PPL 16 would hold 1024 points in one wavefront, but its 81 doubles of state per lane spill past 256 VGPRs.)
//
// Ordering.  Red-black on g & 1, colour 0 first.  'extend' copies S[0] = S[1], S[xc-1] = S[xc-2] (each when its source
// is not undef) at the start of every sweep (numbas.py:685-689); 'fixed' and 'extend' update 1 .. xc-2, 'periodic' also
// 0 and xc-1 with the wrap (numbas.py:692-725).  Periodic with odd xc: point xc-1 is its own colour, run right after
// colour 0.  With PPL even, each half-sweep reads exactly one value across lanes: colour 0 the previous chunk's last
// point (DPP wave_shr:1), colour 1 the next chunk's first point (DPP wave_shl:1); wave ends cross through LDS.
//
// Norm (mean |S| over S != undef, numbas.py:1731-1747), every sweep, in a FIXED order: each lane sums |S| of its chunk
// in index order from 0.0; the 64 lane sums are combined by the butterfly s = s + s[l ^ d], d = 32, 16, 8, 4, 2, 1
// (every lane ends with the same bits); the wave totals are then added in wave order (((w0 + w1) + w2) + ...).  The
// order depends on xc only -- not on the batch, the launch shape, the budget or the device --, so flags[1] and the loop
// count are reproducible bit for bit (tests/std1d_model.py restates it).  count == 0 gives NaN: the overflow exit.
//
// Bounded launches.  A launch runs at most `budget` sweeps of every member that is not done, then stores S and the
// member's XinvCtl; the next launch resumes from them, so the result does not depend on the budget.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/xinv.h"
#include "xinv_device.h"

#define XINV_STD1D_MAX_XC 8192          /* 16 wavefronts x 64 lanes x PPL 8 */
#define XINV_STD1D_WAVE_XC 512          /* one wavefront up to here (PPL 8) */
#define XINV_STD1D_MEMBERS_PER_WG 4     /* single-wave members per workgroup */

struct Std1dArgs {
    double *S;
    const double *A, *B, *F;
    int64_t sS, sA, sB, sF;             // batch strides in elements (0 = one copy shared by every member)
    XinvCtl *ctl;                       // [nbatch]
    int64_t nbatch, xc;
    int BCx;
    int nwave;                          // wavefronts per member (multi-wave kernel)
    int budget;                         // sweeps per launch
    double delxSqr, optArg, undef;
    XinvStop stop;
};

// lane l receives lane l-1's value (lane 0 keeps its own); lane l receives lane l+1's value (lane 63 keeps its own)
__device__ __forceinline__ double xinv_wave_shr1(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double xinv_wave_shl1(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double xinv_readlane_d(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// S[k] for a wave-uniform runtime k, without indexing the register array.  The empty asm keeps each S[q] a register
// value: otherwise the select chain is folded into one load from a computed address, and the array is demoted to LDS.
template <int PPL>
__device__ __forceinline__ double xinv_pick(const double (&S)[PPL], int k)
{
    double r = S[0];
    asm volatile("" : "+v"(r));
#pragma unroll
    for (int q = 1; q < PPL; q++) {
        double t = S[q];
        asm volatile("" : "+v"(t));
        r = (q == k) ? t : r;
    }
    return r;
}

template <int PPL, bool MULTI>
__global__ void __launch_bounds__(MULTI ? 1024 : 64 * XINV_STD1D_MEMBERS_PER_WG) k_std1d(Std1dArgs a)
{
    __shared__ double l_last[16], l_first[16], l_sum[16], l_wrap[2];
    __shared__ long long l_cnt[16];
    const int lane = threadIdx.x & 63;
    const int w = MULTI ? (int)(threadIdx.x >> 6) : 0;
    const int W = MULTI ? a.nwave : 1;
    const int64_t m = MULTI ? (int64_t)blockIdx.x
                            : (int64_t)blockIdx.x * XINV_STD1D_MEMBERS_PER_WG + (threadIdx.x >> 6);
    if (m >= a.nbatch) return;                                  // (single-wave kernel: a tail wave; uniform per wave)
    XinvCtl *cp = a.ctl + m;
    if (xinv_ctl_done(cp)) return;                              // uniform per member
    double normPrev = cp->normPrev, flag1 = cp->flag1, flag2 = cp->flag2;
    long long loop = cp->loop, sweeps = cp->sweeps;
    int done = 0, overflow = cp->overflow, wrote = cp->wrote;

    const int64_t xc = a.xc;
    const double undef = a.undef, dsq = a.delxSqr, opt = a.optArg;
    const bool per = a.BCx == XINV_BC_PERIODIC, ext = a.BCx == XINV_BC_EXTEND;
    const bool seam = per && (xc & 1);                          // odd periodic: xc-1 is its own colour
    const int64_t g0 = ((int64_t)w * 64 + lane) * PPL;
    const int64_t gl = xc - 1;                                  // the last point and its owner
    const int lastLane = (int)((gl / PPL) & 63), lastWave = (int)(gl / PPL / 64), kl = (int)(gl % PPL);
    const bool ownFirst = w == 0 && lane == 0;
    const bool ownLast = w == lastWave && lane == lastLane;

    double *Sg = a.S + m * a.sS;
    const double *Ag = a.A + m * a.sA, *Bg = a.B + m * a.sB, *Fg = a.F + m * a.sF;
    double S[PPL], Am[PPL + 1], Bv[PPL], Fv[PPL], fac[PPL];
    unsigned pred = 0, valid = 0;
    // A[g] (A[xc] of the wrap is A[0]); written out per slot: a loop over PPL + 1 slots is left rolled and the array
    // demoted to memory
    auto loadA = [&](int64_t g) { return g < xc ? Ag[g] : ((per && g == xc) ? Ag[0] : 0.0); };
#pragma unroll
    for (int k = 0; k < PPL; k++) Am[k] = loadA(g0 + k);
    Am[PPL] = loadA(g0 + PPL);
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        const int64_t g = g0 + k;
        const bool in = g < xc;
        S[k] = in ? Sg[g] : 0.0;
        Bv[k] = in ? Bg[g] : 0.0;
        Fv[k] = in ? Fg[g] : 0.0;
        fac[k] = opt / ((Am[k + 1] + Am[k]) / dsq - Bv[k]);
        const bool upd = (g >= 1 && g <= xc - 2) || (per && (g == 0 || g == xc - 1));
        if (upd && Fv[k] != undef && Am[k] != undef && Am[k + 1] != undef && Bv[k] != undef) pred |= 1u << k;
        if (in) valid |= 1u << k;
    }
    // colour 0 without the seam point; the seam point alone
    unsigned pred0 = 0, pred1 = 0, predS = 0;
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        const unsigned b = pred & (1u << k);
        if (seam && ownLast && k == kl) predS |= b;
        else if ((k & 1) == 0) pred0 |= b;
        else pred1 |= b;
    }

#define XINV_STD1D_UPD(k, Sm, Sp)                                                                        \
    {                                                                                                    \
        double t_ = (Am[(k) + 1] * ((Sp) - S[k]) - Am[k] * (S[k] - (Sm))) / dsq + (Bv[k] * S[k] - Fv[k]); \
        t_ *= fac[k];                                                                                    \
        S[k] += t_;                                                                                      \
    }

    for (int it = 0; it < a.budget; it++) {
        // ---- the previous chunk's last point (odd: colour 0 does not change it) and, periodic, S[xc-1] for point 0
        double left = xinv_wave_shr1(S[PPL - 1]);
        double wrapL = 0.0;
        if constexpr (MULTI) {
            if (lane == 63) l_last[w] = S[PPL - 1];
            if (per && ownLast) l_wrap[0] = xinv_pick<PPL>(S, kl);
            __syncthreads();
            if (lane == 0 && w > 0) left = l_last[w - 1];
            if (per) wrapL = l_wrap[0];
        } else if (per) {
            wrapL = xinv_readlane_d(xinv_pick<PPL>(S, kl), lastLane);
        }
        if (ext) {                                              // numbas.py:685-689
            if (ownFirst && S[1] != undef) S[0] = S[1];
            if (ownLast) {
                const double v = kl == 0 ? left : xinv_pick<PPL>(S, kl - 1 < 0 ? 0 : kl - 1);
                if (v != undef) {
#pragma unroll
                    for (int k = 0; k < PPL; k++) S[k] = (k == kl) ? v : S[k];
                }
            }
        }
        // ---- colour 0
#pragma unroll
        for (int k = 0; k < PPL; k += 2) {
            if (pred0 & (1u << k)) {
                const double sm = k == 0 ? (ownFirst ? wrapL : left) : S[k - 1];
                XINV_STD1D_UPD(k, sm, S[k + 1])
            }
        }
        // ---- odd periodic: the seam point xc-1 (even), right after colour 0; its east neighbour is S[0]
        double wrapR = 0.0;
        if (per) {
            if constexpr (MULTI) {
                if (ownFirst) l_wrap[1] = S[0];
                __syncthreads();
                wrapR = l_wrap[1];
            } else {
                wrapR = xinv_readlane_d(S[0], 0);
            }
        }
        if (predS) {
#pragma unroll
            for (int k = 0; k < PPL; k += 2) {
                if (predS & (1u << k)) {
                    const double sm = k == 0 ? left : S[k - 1 < 0 ? 0 : k - 1];
                    XINV_STD1D_UPD(k, sm, wrapR)
                }
            }
        }
        // ---- the next chunk's first point (even: after colour 0 and the seam)
        double right = xinv_wave_shl1(S[0]);
        if constexpr (MULTI) {
            if (lane == 0) l_first[w] = S[0];
            __syncthreads();
            if (lane == 63 && w + 1 < W) right = l_first[w + 1];
        }
        // ---- colour 1 (periodic even xc: point xc-1 reads S[0] as its east neighbour)
#pragma unroll
        for (int k = 1; k < PPL; k += 2) {
            if (pred1 & (1u << k)) {
                double sp = k == PPL - 1 ? right : S[k + 1 < PPL ? k + 1 : k];
                if (per && ownLast && k == kl) sp = wrapR;
                XINV_STD1D_UPD(k, S[k - 1], sp)
            }
        }
        // ---- norm: lane sum in index order, butterfly over the lanes, waves in wave order
        double s = 0.0;
        int c = 0;
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            if ((valid & (1u << k)) && S[k] != undef) { s += fabs(S[k]); c++; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s = s + __shfl_xor(s, d);
            c = c + __shfl_xor(c, d);
        }
        long long cnt = c;
        if constexpr (MULTI) {
            if (lane == 0) { l_sum[w] = s; l_cnt[w] = cnt; }
            __syncthreads();
            s = l_sum[0];
            cnt = l_cnt[0];
            for (int q = 1; q < W; q++) { s = s + l_sum[q]; cnt += l_cnt[q]; }
        }
        // ---- stop rule (numbas.py:728-740), the same decision in every lane
        const double norm = cnt != 0 ? s / (double)cnt : NAN;
        if (isnan(norm) || norm > 1e100) {
            overflow = 1; done = 1; sweeps = loop + 1;
            break;
        }
        flag1 = fabs(norm - normPrev) / normPrev;
        flag2 = (double)loop;
        wrote = 1;
        if (flag1 < a.stop.tolerance || loop >= a.stop.mxLoop || norm == 0.0) {
            done = 1; sweeps = loop + 1;
            break;
        }
        normPrev = norm;
        loop += 1;
    }
#undef XINV_STD1D_UPD

#pragma unroll
    for (int k = 0; k < PPL; k++)
        if (valid & (1u << k)) Sg[g0 + k] = S[k];
    if constexpr (MULTI) __syncthreads();                       // (every wavefront has read the control block)
    if (w == 0 && lane == 0) {
        cp->normPrev = normPrev; cp->flag1 = flag1; cp->flag2 = flag2;
        cp->loop = loop; cp->sweeps = sweeps;
        cp->overflow = overflow; cp->wrote = wrote;
        cp->done = done;
    }
}

// xinv_tu_std1d.hip: one launch of `a.budget` sweeps over every member (shape chosen from a.xc as above)
__attribute__((visibility("hidden"))) int xinv_launch_std1d(const Std1dArgs &a, hipStream_t st);
// the shape of a member of xc points: points per lane and wavefronts (0, 0 above XINV_STD1D_MAX_XC)
static inline void xinv_std1d_shape(int64_t xc, int *ppl, int *nwave)
{
    *ppl = 0; *nwave = 0;
    if (xc <= XINV_STD1D_WAVE_XC) {
        int p = 2;
        while (64 * p < xc) p *= 2;
        *ppl = p; *nwave = 1;
    } else if (xc <= XINV_STD1D_MAX_XC) {
        *ppl = 8; *nwave = (int)((xc + 511) / 512);
    }
}
