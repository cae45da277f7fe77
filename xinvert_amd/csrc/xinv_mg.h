// xinv_mg.h -- grid transfers of invert_MultiGrid (xinvert_amd/multigrid.py): restriction of a forcing to a coarse grid
// and prolongation of a coarse solution to the next finer grid's initial guess.
//
// Both kernels work on the [nbatch][core...] layout of core._batch_layout / core.Resident with 1 to 3 core dims; the
// host pads the core to three dims with leading length-1 dims (ratio 1, identity tables), which changes no summation
// or blend order.  A workgroup of XINV_MG_WG lanes owns XINV_MG_WG consecutive points of one row of the last axis; the
// row is a wave-uniform counter (batch member and the slower core indices follow from it by scalar divisions) and the
// workgroups stride over the rows, so any element count fits a 32-bit grid.  Indexing is 64-bit.
//
// k_mg_restrict: one coarse point per lane.  Coarse point (b, J0, J1, J2) owns the fine block
//     J_a * r_a + o_a,  o_a = 0 .. r_a - 1   (the trailing n_a % r_a fine points belong to no block)
// and sums the block's points that are not `undef` (nan != 0: NaN points instead) in lexicographic offset order, from
// 0.0: ((0.0 + v0) + v1) + ...; the result is sum / count (one division), `undef` when the block has no valid point.
//
// k_mg_prolong: one fine point per lane.  The host tables give, per axis a and fine index i, two coarse indices
// lo[i], hi[i] and a weight w[i]; the value is the d-linear blend nested from the slowest axis to the fastest
//     2-D:  (1 - wy) * ((1 - wx) * c[ylo, xlo] + wx * c[ylo, xhi]) + wy * ((1 - wx) * c[yhi, xlo] + wx * c[yhi, xhi])
// (1 - w evaluated each time it appears).  The fine point is NOT written -- it keeps the value the ordinary solve starts
// from -- where the fine forcing equals `undef`, on the first / last index of an axis whose bit is set in keep_edges,
// and where the blend is not finite.
//
// Only + - * / are evaluated, in the order above (-ffp-contract=off), so tests/mg_model.py reproduces both bit for
// bit.  Tables and data are read with VECTOR loads (-amdgpu-scalarize-global-loads=0, no __restrict__ / const-space
// pointers): only the argument segment goes through the scalar unit (tools/smem_audit.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define XINV_MG_WG 256
#define XINV_MG_MAXBLOCKS (1 << 20)

struct MgRestrictArgs {
    const double *fine;
    double *coarse;
    int64_t fn[3], cn[3], r[3];         // fine / coarse lengths and ratios of the (padded) core, slowest first
    int64_t fslice, cslice;             // elements of one fine / coarse member
    int64_t rows, nbx;                  // coarse rows (nbatch * cn0 * cn1), workgroups per row
    double undef;
    int nan;                            // 1: NaN points are the undefined ones
};

struct MgProlongArgs {
    const double *coarse;
    double *fine;
    const double *force;                // fine forcing (null: every point is defined)
    const int64_t *lo[3], *hi[3];       // per axis, fine length entries
    const double *w[3];
    int64_t fn[3], cn[3];
    int64_t fslice, cslice;
    int64_t rows, nbx;                  // fine rows (nbatch * fn0 * fn1), workgroups per row
    double undef;
    int keep;                           // bit a: keep the edge indices of (padded) axis a
    int nd;                             // real core dims (1 .. 3): the blend's nesting depth
};

int xinv_launch_mg_restrict(const MgRestrictArgs &a, int64_t nblocks, hipStream_t st);
int xinv_launch_mg_prolong(const MgProlongArgs &a, int64_t nblocks, hipStream_t st);

#ifdef XINV_MG_DEVICE

__global__ void __launch_bounds__(XINV_MG_WG) k_mg_restrict(MgRestrictArgs a)
{
    const int64_t total = a.rows * a.nbx;
    for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const int64_t row = blk / a.nbx;
        const int64_t x = (blk - row * a.nbx) * XINV_MG_WG + threadIdx.x;
        if (x >= a.cn[2]) continue;
        const int64_t j1 = row % a.cn[1], t = row / a.cn[1];
        const int64_t j0 = t % a.cn[0], b = t / a.cn[0];
        const double *src = a.fine + b * a.fslice + ((j0 * a.r[0]) * a.fn[1] + j1 * a.r[1]) * a.fn[2] + x * a.r[2];
        double sum = 0.0, cnt = 0.0;
        for (int64_t o0 = 0; o0 < a.r[0]; ++o0)
            for (int64_t o1 = 0; o1 < a.r[1]; ++o1) {
                const double *p = src + (o0 * a.fn[1] + o1) * a.fn[2];
                for (int64_t o2 = 0; o2 < a.r[2]; ++o2) {
                    const double v = p[o2];
                    const bool bad = a.nan ? (v != v) : (v == a.undef);
                    if (!bad) {
                        sum = sum + v;
                        cnt = cnt + 1.0;
                    }
                }
            }
        a.coarse[b * a.cslice + (j0 * a.cn[1] + j1) * a.cn[2] + x] = cnt > 0.0 ? sum / cnt : a.undef;
    }
}

template <int ND>
__global__ void __launch_bounds__(XINV_MG_WG) k_mg_prolong(MgProlongArgs a)
{
    const int64_t total = a.rows * a.nbx;
    for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const int64_t row = blk / a.nbx;
        const int64_t x = (blk - row * a.nbx) * XINV_MG_WG + threadIdx.x;
        if (x >= a.fn[2]) continue;
        const int64_t i1 = row % a.fn[1], t = row / a.fn[1];
        const int64_t i0 = t % a.fn[0], b = t / a.fn[0];
        const int64_t fi = b * a.fslice + (i0 * a.fn[1] + i1) * a.fn[2] + x;
        if (a.force && a.force[fi] == a.undef) continue;
        if (((a.keep & 1) && (i0 == 0 || i0 == a.fn[0] - 1)) || ((a.keep & 2) && (i1 == 0 || i1 == a.fn[1] - 1)) ||
            ((a.keep & 4) && (x == 0 || x == a.fn[2] - 1)))
            continue;
        const double *c = a.coarse + b * a.cslice;
        const int64_t xl = a.lo[2][x], xh = a.hi[2][x];
        const double wx = a.w[2][x];
        double v;
        if (ND == 1) {
            v = (1.0 - wx) * c[xl] + wx * c[xh];
        } else {
            const int64_t yl = a.lo[1][i1], yh = a.hi[1][i1];
            const double wy = a.w[1][i1];
            if (ND == 2) {
                const double *cl = c + yl * a.cn[2], *ch = c + yh * a.cn[2];
                v = (1.0 - wy) * ((1.0 - wx) * cl[xl] + wx * cl[xh]) + wy * ((1.0 - wx) * ch[xl] + wx * ch[xh]);
            } else {
                const int64_t zl = a.lo[0][i0], zh = a.hi[0][i0];
                const double wz = a.w[0][i0];
                const double *ll = c + (zl * a.cn[1] + yl) * a.cn[2], *lh = c + (zl * a.cn[1] + yh) * a.cn[2];
                const double *hl = c + (zh * a.cn[1] + yl) * a.cn[2], *hh = c + (zh * a.cn[1] + yh) * a.cn[2];
                const double vl = (1.0 - wy) * ((1.0 - wx) * ll[xl] + wx * ll[xh]) +
                                  wy * ((1.0 - wx) * lh[xl] + wx * lh[xh]);
                const double vh = (1.0 - wy) * ((1.0 - wx) * hl[xl] + wx * hl[xh]) +
                                  wy * ((1.0 - wx) * hh[xl] + wx * hh[xh]);
                v = (1.0 - wz) * vl + wz * vh;
            }
        }
        if (__builtin_isfinite(v)) a.fine[fi] = v;
    }
}

#endif
