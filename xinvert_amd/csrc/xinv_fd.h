// xinv_fd.h -- finite-difference operators of the reference's finitediffs.py (FiniteDiff, deriv, deriv2): one launch per
// public call, every output point from the caller's C-contiguous inputs in their own dim order.
//
// The operand is viewed as rows of the LAST axis: nx = shape[ndim-1] points per row, nr = elements / nx rows.  A workgroup
// of 256 lanes owns 256 consecutive points of a row and marches down `rb` consecutive rows, so the neighbours along the
// second-to-last axis (rows r-1, r+1) are the lines the same workgroup fetched one or two steps earlier: they come from
// the vector L1 / L2, and HBM sees each input about once (halo: 2 rows in rb).  Neighbours along the last axis are the
// adjacent lanes' lines.  The index of a point along any axis a is x (the last axis) or (r / srow_a) % n_a, srow_a = the
// axis's stride in rows, kept as a wave-uniform counter through the march (one division per workgroup).
//
// A call is a list of up to XINV_FD_MAXT terms combined by `mode`:
//   XINV_FD_EACH  out[t] = term t                       (deriv, deriv2, grad: one output per term)
//   XINV_FD_SUM   out[0] = ((0 + term 0) + term 1) + ... (divg, tension_strain, Laplacian; python's sum(re) from int 0)
//   XINV_FD_DIFF  out[0] = term 0 - term 1               (one vorticity component)
// and, for SUM, a keep mask along one axis (the Laplacian's |lat| == 90 -> 0).  A term is one derivative of one input:
//   f(j)    = (neg ? -in : in)[.. j ..] * pw[j]          (pre-weight along any axis; divg's / vort's cos(lat) weighting)
//   padding = BC per end (fixed: the fill, extend: f(0) / f(n-1), reflect: f(1) / f(n-2), periodic: f(n-1) / f(0)),
//             evaluated in registers from the neighbour the BC names; nothing padded is materialised
//   center  = numpy.gradient on the padded axis: (fp - fm) / (2 dx) when the padded coordinate is uniform, else
//             (a fm + b f0) + c fp with numpy's per-index weights; then / divisor
//   forward = (f0 - fp) / (c[i] - c[i+1]) / divisor, NaN at i = n-1;  backward = (fm - f0) / (c[i-1] - c[i]) / divisor,
//             NaN at i = 0 (no padding: xarray's shift)
//   second  = ((fp - f0) - (f0 - fm)) / h2[i] / divisor2, h2 = the squared lower spacing of the padded coordinate;
//             metric 1 adds the literal +0 of the reference's `+ metric` (metric = 0), metric 2 adds
//             ((-(center / msc)) * tan[i]) / R (the Laplacian's Y metric term)
// The divisor is a scalar or a per-index table along any axis (the X derivative over cos(lat) runs along Y).  Every table
// is built on the host with numpy; the device only evaluates + - * / in the model's order (-ffp-contract=off), so the
// results are the numpy restatement's bits.
//
// Tables are read with VECTOR loads (-amdgpu-scalarize-global-loads=0, no __restrict__ / const-space pointers): only the
// argument segment goes through the scalar unit (tools/smem_audit.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define XINV_FD_MAXT 4
#define XINV_FD_MAXIN 3
#define XINV_FD_WG 256

enum { XINV_FD_CENTER = 0, XINV_FD_FORWARD = 1, XINV_FD_BACKWARD = 2, XINV_FD_SECOND = 3 };
enum { XINV_FD_EACH = 0, XINV_FD_SUM = 1, XINV_FD_DIFF = 2 };
enum { XINV_FD_BC_FIXED = 0, XINV_FD_BC_EXTEND = 1, XINV_FD_BC_PERIODIC = 2, XINV_FD_BC_REFLECT = 3 };

struct FdTerm {
    const double *src;                 // the input this term differentiates
    const double *wa, *wb, *wc;        // centre: numpy.gradient's non-uniform weights per index of the derivative axis
    const double *dd;                  // forward / backward: coordinate differences; second: h^2 (per index)
    const double *pw;                  // pre-weight table (null: none)
    const double *sc;                  // divisor table (second: divisor^2) (null: the scalar scs)
    const double *tn;                  // metric 2: tan(lat) per index of the derivative axis
    int64_t n, srow, stride;           // derivative axis: length, stride in rows (0: the last axis), stride in elements
    int64_t pn, psrow;                 // pre-weight axis (used when !psame)
    int64_t sn, ssrow;                 // divisor axis
    double fl, fr;                     // fixed-BC fills (left, right)
    double twodx;                      // uniform centre: 2 * dx of the padded coordinate
    double scs;                        // scalar divisor (second: divisor^2)
    double msc, R;                     // metric 2: the first derivative's divisor, the radius
    int kind, neg, bcl, bcr, uniform, metric, psame;
};

struct FdArgs {
    double *out[XINV_FD_MAXT];
    const double *mask;                // SUM: keep flag per index of the mask axis (0 -> the output is 0)
    int64_t mn, msrow;
    int64_t nx, nr, nbx, rb;           // points per row, rows, workgroups per row, rows per workgroup
    int nt, mode;
    FdTerm t[XINV_FD_MAXT];
};

int xinv_launch_fd(const FdArgs &a, int64_t nblocks, hipStream_t st);

#ifdef XINV_FD_DEVICE

// Index along one axis for the rows a workgroup marches through: one division where the march starts, then a counter
// stepped without branches (row r's index along an axis of row stride s is (r / s) % n; s = 0 marks the last axis,
// whose index is the lane's x).
struct XinvFdCtr {
    int64_t i, c, n, s;
};

__device__ __forceinline__ void xinv_fd_ctr_init(XinvFdCtr &k, int64_t s, int64_t n, int64_t r)
{
    k.s = s; k.n = n;
    k.i = s ? (r / s) % n : 0;
    k.c = s ? r % s : 0;
}

__device__ __forceinline__ void xinv_fd_ctr_step(XinvFdCtr &k)
{
    const int64_t c1 = k.c + 1;
    const bool wrap = c1 == k.s;
    k.c = wrap ? 0 : c1;
    const int64_t i1 = k.i + (wrap ? 1 : 0);
    k.i = i1 == k.n ? 0 : i1;
}

__device__ __forceinline__ int64_t xinv_fd_ctr_idx(const XinvFdCtr &k, int64_t x) { return k.s ? k.i : x; }

// The three raw values a term reads at its point (index ia along the derivative axis, element q): the point and the
// neighbours jm / jp the BC names at the ends (reflect: 1 / n-2, periodic: n-1 / 0, otherwise the point itself, whose
// value the fixed BC then replaces).  Branch-free: the loads of several rows can all be in flight at once.
struct XinvFdRaw {
    double m, o, p;
    int64_t jm, jp;
};

__device__ __forceinline__ void xinv_fd_load(const FdTerm &t, int64_t q, int64_t ia, XinvFdRaw &w)
{
    const int64_t n = t.n;
    w.jm = ia > 0 ? ia - 1 : (t.bcl == XINV_FD_BC_REFLECT ? 1 : t.bcl == XINV_FD_BC_PERIODIC ? n - 1 : ia);
    w.jp = ia < n - 1 ? ia + 1 : (t.bcr == XINV_FD_BC_REFLECT ? n - 2 : t.bcr == XINV_FD_BC_PERIODIC ? 0 : ia);
    w.m = t.src[q + (w.jm - ia) * t.stride];
    w.o = t.src[q];
    w.p = t.src[q + (w.jp - ia) * t.stride];
}

// f at index j of the derivative axis from its raw value; pi: the pre-weight index when the pre-weight runs along
// another axis
__device__ __forceinline__ double xinv_fd_f(const FdTerm &t, double raw, int64_t j, int64_t pi)
{
    double v = t.neg ? -raw : raw;
    if (t.pw) v = v * t.pw[t.psame ? j : pi];
    return v;
}

// ia / pi / si: the point's index along the derivative, pre-weight and divisor axes
__device__ __forceinline__ double xinv_fd_term(const FdTerm &t, const XinvFdRaw &w, int64_t ia, int64_t pi, int64_t si)
{
    const int64_t n = t.n;
    const double div = t.sc ? t.sc[si] : t.scs;
    const double f0 = xinv_fd_f(t, w.o, ia, pi);
    if (t.kind == XINV_FD_FORWARD) {
        if (ia == n - 1) return __builtin_nan("");
        return ((f0 - xinv_fd_f(t, w.p, w.jp, pi)) / t.dd[ia]) / div;
    }
    if (t.kind == XINV_FD_BACKWARD) {
        if (ia == 0) return __builtin_nan("");
        return ((xinv_fd_f(t, w.m, w.jm, pi) - f0) / t.dd[ia]) / div;
    }
    // (extend: jm / jp is the point itself, so f(jm) / f(jp) is f0)
    const double fm = (ia == 0 && t.bcl == XINV_FD_BC_FIXED) ? t.fl : xinv_fd_f(t, w.m, w.jm, pi);
    const double fp = (ia == n - 1 && t.bcr == XINV_FD_BC_FIXED) ? t.fr : xinv_fd_f(t, w.p, w.jp, pi);
    if (t.kind == XINV_FD_CENTER) {
        const double g = t.uniform ? (fp - fm) / t.twodx : (t.wa[ia] * fm + t.wb[ia] * f0) + t.wc[ia] * fp;
        return g / div;
    }
    double v = (((fp - f0) - (f0 - fm)) / t.dd[ia]) / div;
    if (t.metric == 1) {
        v = v + 0.0;
    } else if (t.metric == 2) {
        const double g = t.uniform ? (fp - fm) / t.twodx : (t.wa[ia] * fm + t.wb[ia] * f0) + t.wc[ia] * fp;
        v = v + ((-(g / t.msc)) * t.tn[ia]) / t.R;
    }
    return v;
}

// U consecutive rows from r: indices, then every load of the U rows, then the arithmetic, then the stores (k_fd: U = 1).
template <int NT, int U>
__device__ __forceinline__ void xinv_fd_rows(const FdArgs &a, int64_t r, int64_t x, XinvFdCtr *ka, XinvFdCtr *kp,
                                             XinvFdCtr *ks, XinvFdCtr &km)
{
    int64_t ia[U][NT], pi[U][NT], si[U][NT], mi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            ia[u][t] = xinv_fd_ctr_idx(ka[t], x);
            pi[u][t] = xinv_fd_ctr_idx(kp[t], x);
            si[u][t] = xinv_fd_ctr_idx(ks[t], x);
            xinv_fd_ctr_step(ka[t]);
            xinv_fd_ctr_step(kp[t]);
            xinv_fd_ctr_step(ks[t]);
        }
        mi[u] = xinv_fd_ctr_idx(km, x);
        xinv_fd_ctr_step(km);
    }
    XinvFdRaw w[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) xinv_fd_load(a.t[t], (r + u) * a.nx + x, ia[u][t], w[u][t]);
    double v[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) v[u][t] = xinv_fd_term(a.t[t], w[u][t], ia[u][t], pi[u][t], si[u][t]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t q = (r + u) * a.nx + x;
        if (a.mode == XINV_FD_EACH) {
#pragma unroll
            for (int t = 0; t < NT; ++t) a.out[t][q] = v[u][t];
        } else if (a.mode == XINV_FD_DIFF) {
            a.out[0][q] = v[u][0] - v[u][NT > 1 ? 1 : 0];
        } else {
            double acc = 0.0 + v[u][0];
#pragma unroll
            for (int t = 1; t < NT; ++t) acc = acc + v[u][t];
            if (a.mask && a.mask[mi[u]] == 0.0) acc = 0.0;
            a.out[0][q] = acc;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(XINV_FD_WG) void k_fd(FdArgs a)
{
    const int64_t b = blockIdx.x;
    const int64_t bx = b % a.nbx, by = b / a.nbx;
    const int64_t x = bx * XINV_FD_WG + threadIdx.x;
    if (x >= a.nx) return;
    const int64_t r0 = by * a.rb;
    const int64_t r1 = r0 + a.rb < a.nr ? r0 + a.rb : a.nr;
    XinvFdCtr ka[NT], kp[NT], ks[NT], km;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        xinv_fd_ctr_init(ka[t], a.t[t].srow, a.t[t].n, r0);
        xinv_fd_ctr_init(kp[t], a.t[t].pw && !a.t[t].psame ? a.t[t].psrow : 0, a.t[t].pn, r0);
        xinv_fd_ctr_init(ks[t], a.t[t].sc ? a.t[t].ssrow : 0, a.t[t].sn, r0);
    }
    xinv_fd_ctr_init(km, a.mask ? a.msrow : 0, a.mn, r0);
    // (one row per step: four rows per step, loads of all four first, measured slower -- 88 VGPRs and a 10.8k-instruction
    // body for two terms; curl 0.99 -> 1.14 ms on 8 x 1800 x 3600)
    for (int64_t r = r0; r < r1; ++r) xinv_fd_rows<NT, 1>(a, r, x, ka, kp, ks, km);
}

#endif // XINV_FD_DEVICE
