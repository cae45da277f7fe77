// xinv_tridiag_host.h -- host side of k_tridiag (xinv_tridiag.h): the argument checks of xinv_tridiag_f64[_dev], the
// per-device workspace of the forward pass, the host-pointer staging, and the direct solve of the 1-D standard form
// behind XINV_PATH_DIRECT1D.  Included by xinv_hip.hip only, after xinv_std1d_host.h (Std1dProblem).
#pragma once
#include "xinv_tridiag.h"

// One call as the ABI describes it; strides: x, a, b, c, d, a0, cn (elements; 0 = shared).
struct TridiagCall {
    double *x;
    const double *a, *b, *c, *d, *a0, *cn;
    int64_t nbatch, n;
    int64_t s[7];
};

static int tridiag_fail(const char *what)
{
    t_err = std::string("xinv_tridiag: ") + what;
    return XINV_ERR_ARG;
}

static int tridiag_validate(const TridiagCall &c, const int64_t *strides)
{
    if (!c.x || !c.a || !c.b || !c.c || !c.d) return tridiag_fail("null array");
    if (!strides) return tridiag_fail("null strides");
    if ((c.a0 == nullptr) != (c.cn == nullptr)) return tridiag_fail("a0 and cn come together (both NULL: trace)");
    if (c.n < 2) return tridiag_fail("a system needs n >= 2");
    if (c.nbatch < 1) return tridiag_fail("nbatch < 1");
    if (c.nbatch > ((int64_t)1 << 36)) return tridiag_fail("nbatch is too large");
    const int64_t need[7] = { c.n, c.n - 1, c.n, c.n - 1, c.n, 1, 1 };
    for (int q = 0; q < (c.a0 ? 7 : 5); q++) {
        if (c.s[q] < 0) return tridiag_fail("negative batch stride");
        if (c.nbatch > 1 && c.s[q] < need[q] && !(q > 0 && c.s[q] == 0))
            return tridiag_fail("batch stride must be 0 (shared; not x) or at least one system's length");
    }
    return XINV_OK;
}

// the forward pass's workspace: `arrays` x [nbatch][n] doubles and, `ovf`, one word per member.  A queued
// xinv_tridiag_f64_dev solve may still be using ws->tri, on any stream: `st`, the stream the solve will run on, is ordered
// behind it here -- or the calling thread, before the buffer is freed to grow.
static int tridiag_workspace(Workspace *ws, hipStream_t st, int64_t nbatch, int64_t n, int arrays, bool ovf)
{
    const size_t need = (size_t)arrays * (size_t)nbatch * (size_t)n * sizeof(double);
    int rc = ws->tri_user.wait(st, !ws->tri || ws->tri_cap < need);
    if (rc) return rc;
    rc = ensure_dev(&ws->tri, &ws->tri_cap, need);
    if (rc || !ovf) return rc;
    if ((rc = ensure_dev(&ws->tri_ovf, &ws->tri_ovf_cap, (size_t)nbatch * sizeof(int)))) return rc;
    return ensure_pinned(&ws->h_tri_ovf, &ws->h_tri_ovf_cap, (size_t)nbatch * sizeof(int), hipHostMallocDefault);
}

// Device arrays, on `st`, with the device already selected.  Returns with the kernel queued: the lock covers the launch,
// the event covers the kernel, so calls from several streams or threads take turns on the device's one buffer.
static int tridiag_run_dev(const TridiagCall &c, hipStream_t st)
{
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> lock(ws->busy);
    const bool cyc = c.a0 != nullptr;
    int rc = tridiag_workspace(ws, st, c.nbatch, c.n, cyc ? 3 : 1, false);
    if (rc) return rc;
    TridiagArgs a;
    memset(&a, 0, sizeof a);
    a.x = c.x; a.sx = c.nbatch > 1 ? c.s[0] : c.n;
    a.p[0] = c.a; a.p[1] = c.b; a.p[2] = c.c; a.p[3] = c.d;
    for (int q = 0; q < 4; q++) a.sp[q] = c.nbatch > 1 ? c.s[1 + q] : 0;
    a.a0 = c.a0; a.cn = c.cn;
    a.sa0 = c.nbatch > 1 ? c.s[5] : 0; a.scn = c.nbatch > 1 ? c.s[6] : 0;
    const int64_t plane = c.nbatch * c.n;
    a.wg = ws->tri; a.wu = ws->tri + plane; a.wv = ws->tri + 2 * plane;
    a.nbatch = c.nbatch; a.n = c.n;
    xinv_launch_tridiag(a, false, cyc, st);
    HIPCHK(hipGetLastError());
    return ws->tri_user.mark(st);
}

static int tridiag_solve_dev(const TridiagCall &c, const int64_t *strides, hipStream_t st)
{
    int rc = tridiag_validate(c, strides);
    if (rc) return rc;
    return tridiag_run_dev(c, st);
}

// Host arrays: upload (a shared array once), one solve, download x.  Like std1d_solve_host it is the plain entry
// (PlainStage): one device block allocated and freed per call, pageable copies on the null stream.  "No hipMalloc in
// steady state" holds for the device entry and the direct path, whose scratch is the workspace; a caller who minds keeps
// its arrays on the device.
static int tridiag_solve_host(const TridiagCall &hc, const int64_t *strides)
{
    int rc = tridiag_validate(hc, strides);
    if (rc) return rc;
    PlainStage stage;
    const int64_t nb = hc.nbatch, n = hc.n;
    const bool cyc = hc.a0 != nullptr;
    const double *src[6] = { hc.a, hc.b, hc.c, hc.d, hc.a0, hc.cn };
    const int64_t len[6] = { n - 1, n, n - 1, n, 1, 1 };
    const int narr = cyc ? 6 : 4;
    int64_t rows[6], total = nb * n;
    for (int q = 0; q < narr; q++) {
        rows[q] = (nb == 1 || hc.s[1 + q] == 0) ? 1 : nb;
        total += rows[q] * len[q];
    }
    if ((rc = stage.open((size_t)total * sizeof(double)))) return rc;
    TridiagCall c = hc;
    c.x = stage.carve(nb * n); c.s[0] = n;
    const double *dev[6] = {};
    for (int q = 0; q < narr; q++) {
        double *at = stage.carve(rows[q] * len[q]);
        if ((rc = stage.up_rows(at, src[q], rows[q], len[q], hc.s[1 + q]))) return rc;
        dev[q] = at;
        c.s[1 + q] = rows[q] > 1 ? len[q] : 0;
    }
    c.a = dev[0]; c.b = dev[1]; c.c = dev[2]; c.d = dev[3];
    if (cyc) { c.a0 = dev[4]; c.cn = dev[5]; }
    stage.uploads_queued();
    if ((rc = tridiag_run_dev(c, stage.st))) return rc;
    stage.run_done();
    if ((rc = stage.down_rows(hc.x, c.x, nb, n, hc.s[0]))) return rc;
    return stage.finish(true);
}

// XINV_PATH_DIRECT1D: the 1-D standard form's fixed point in one launch (std1d_run hands over; `p` holds DEVICE arrays).
// optArg, mxLoop, tolerance and the sweep options play no part; flags = [overflow, 0, 0].
static int std1d_direct_run(const Std1dProblem &p, double *flags, const xinv_options &o, hipStream_t st)
{
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> lock(ws->busy);
    const bool per = p.BCx == XINV_BC_PERIODIC;
    int rc = tridiag_workspace(ws, st, p.nbatch, p.xc, per ? 3 : 1, true);
    if (rc) return rc;
    memset(&t_stats, 0, sizeof t_stats);
    TridiagArgs a;
    memset(&a, 0, sizeof a);
    a.x = p.S; a.sx = p.nbatch > 1 ? p.sS : p.xc;
    a.p[0] = p.A; a.p[1] = p.B; a.p[2] = p.F;
    a.sp[0] = p.nbatch > 1 ? p.sA : 0; a.sp[1] = p.nbatch > 1 ? p.sB : 0; a.sp[2] = p.nbatch > 1 ? p.sF : 0;
    const int64_t plane = p.nbatch * p.xc;
    a.wg = ws->tri; a.wu = ws->tri + plane; a.wv = ws->tri + 2 * plane;
    a.ovf = ws->tri_ovf;
    a.nbatch = p.nbatch; a.n = p.xc;
    a.delxSqr = p.delxSqr; a.undef = p.undef; a.ext = p.BCx == XINV_BC_EXTEND;
    hipEvent_t e0 = ws->ev0[0], e1 = ws->ev1[0];
    const bool timing = o.timing != 0 && e0 && e1;
    if (timing) HIPCHK(hipEventRecord(e0, st));
    xinv_launch_tridiag(a, true, per, st);
    HIPCHK(hipGetLastError());
    if (timing) HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(ws->h_tri_ovf, ws->tri_ovf, (size_t)p.nbatch * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ws->tri_user.pending = false;                        // (`st` waited on the event, and has drained)
    for (int64_t m = 0; m < p.nbatch; m++) {
        flags[3 * m] = ws->h_tri_ovf[m] ? 1.0 : 0.0;
        flags[3 * m + 1] = 0.0;
        flags[3 * m + 2] = 0.0;
    }
    t_stats.path = XINV_PATH_DIRECT1D;
    t_stats.lanes = 1;
    t_stats.devices = 1;
    t_stats.sweep_launches = 1;
    if (timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        t_stats.sweep_ms = ms;
    }
    return XINV_OK;
}
