// xinv_resid_host.h -- host side of k_resid2d / k_resid3d (xinv_resid.h): the argument checks of xinv_residual_*_f64_dev /
// _batched, the per-device buffer of the norm partials, and the host-pointer staging.  Included by xinv_hip.hip only.
#pragma once
#include "xinv_resid.h"

// One call as the ABI describes it; s[]: batch strides of R, S and the form's arrays, in that order (elements; 0 = shared).
struct ResidCall {
    int kind;
    double *R;
    const double *S;
    const double *c[8];
    int64_t nbatch, zc, yc, xc;
    int64_t s[10];
    int BCz, BCy, BCx;
    XinvScal sc_;
};

static ResidCall mk_resid(int kind, double *R, const double *S, const double *const *c, int64_t nbatch, const int64_t *st,
                          int64_t zc, int64_t yc, int64_t xc, int BCz, int BCy, int BCx, const XinvScal &sc)
{
    ResidCall r;
    memset(&r, 0, sizeof r);
    r.kind = kind; r.R = R; r.S = S; r.nbatch = nbatch; r.zc = zc; r.yc = yc; r.xc = xc;
    for (int q = 0; q < FORM[kind].ncoef; q++) r.c[q] = c[q];
    if (st)
        for (int q = 0; q < 2 + FORM[kind].ncoef; q++) r.s[q] = st[q];
    r.BCz = BCz; r.BCy = BCy; r.BCx = BCx;
    r.sc_ = sc;
    return r;
}

static int resid_fail(const char *what)
{
    t_err = std::string("xinv_residual: ") + what;
    return XINV_ERR_ARG;
}

static int resid_form(int kind)
{
    return kind == KIND_STD2D ? RESID_STD2D : kind == KIND_GEN2D ? RESID_GEN2D : kind == KIND_STD2DT ? RESID_STD2DT
         : kind == KIND_STD3D ? RESID_STD3D : RESID_GEN3D;
}

// The shapes and codes the solve entries refuse (validate, xinv_host.h) are refused here, and R may not overlap an input.
static int resid_validate(const ResidCall &c, const int64_t *strides)
{
    const int nc = FORM[c.kind].ncoef;
    if (!c.R || !c.S) return resid_fail("null R or S");
    if (!strides) return resid_fail("null strides");
    for (int q = 0; q < nc; q++)
        if (!c.c[q] && !(q == 1 && FORM[c.kind].null_B)) return resid_fail("null coefficient array");
    if (c.nbatch < 1) return resid_fail("nbatch < 1");
    if (c.yc < 3 || c.xc < 3 || (is3d(c.kind) && c.zc < 3)) return resid_fail("every core dimension needs at least 3 points");
    if (!bc_ok(c.BCy) || !bc_ok(c.BCx) || (is3d(c.kind) && !bc_ok(c.BCz))) return resid_fail("unknown boundary-condition code");
    const int64_t n = c.zc * c.yc * c.xc;
    for (int q = 0; q < 2 + nc; q++) {
        if (c.s[q] < 0) return resid_fail("negative batch stride");
        if (c.nbatch > 1 && c.s[q] < n && !(q > 0 && c.s[q] == 0))
            return resid_fail("batch stride must be 0 (shared; not R) or at least one slice");
    }
    // [lo, hi) of every array over the whole batch: R against each input
    auto span = [&](const double *p, int64_t stride, const double *&lo, const double *&hi) {
        lo = p; hi = p + (c.nbatch - 1) * stride + n;
    };
    const double *rlo, *rhi, *lo, *hi;
    span(c.R, c.s[0], rlo, rhi);
    span(c.S, c.s[1], lo, hi);
    if (rlo < hi && lo < rhi) return resid_fail("R overlaps S");
    for (int q = 0; q < nc; q++) {
        if (!c.c[q]) continue;
        span(c.c[q], c.s[2 + q], lo, hi);
        if (rlo < hi && lo < rhi) return resid_fail("R overlaps a coefficient array");
    }
    return XINV_OK;
}

// Device arrays, on `st`, with the device already selected.  Without `norms` the launch is only queued.  With them the
// partials live in the workspace's one buffer: the call holds the device's lock until the norms are on the host, so the
// next user finds the buffer idle.
static int resid_run_dev(const ResidCall &c, double *norms, hipStream_t st)
{
    ResidArgs a;
    memset(&a, 0, sizeof a);
    a.R = c.R; a.S = c.S; a.sR = c.s[0]; a.sS = c.s[1];
    for (int q = 0; q < FORM[c.kind].ncoef; q++) { a.c[q] = c.c[q]; a.sc[q] = c.s[2 + q]; }
    a.zc = c.zc; a.yc = c.yc; a.xc = c.xc;
    a.per = c.BCx == XINV_BC_PERIODIC;
    a.sc_ = c.sc_;
    const bool nine = FORM[c.kind].null_B ? c.c[1] != nullptr : true;
    if (!norms) {
        if (xinv_launch_resid(resid_form(c.kind), nine, a, c.nbatch, nullptr, st)) return resid_fail("the grid is too large");
        HIPCHK(hipGetLastError());
        return XINV_OK;
    }
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> lock(ws->busy);
    a.nslot = xinv_resid_slots(is3d(c.kind), c.zc, c.yc, c.xc);
    const size_t nparts = (size_t)c.nbatch * (size_t)a.nslot * 4;
    int rc = ensure_dev(&ws->res_part, &ws->res_part_cap, (nparts + (size_t)c.nbatch * 4) * sizeof(double));
    if (rc) return rc;
    a.part = ws->res_part;
    double *dn = ws->res_part + nparts;
    if (xinv_launch_resid(resid_form(c.kind), nine, a, c.nbatch, dn, st)) return resid_fail("the grid is too large");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(norms, dn, (size_t)c.nbatch * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return XINV_OK;
}

static int resid_dev(const ResidCall &c, const int64_t *strides, double *norms, hipStream_t st)
{
    int rc = resid_validate(c, strides);
    if (rc) return rc;
    return resid_run_dev(c, norms, st);
}

// `rows` slices of n elements, `stride` apart on the host, packed on the device (packed on the host too: one plain copy)
static int resid_up(PlainStage &stage, double *dev, const double *host, int64_t rows, int64_t n, int64_t stride)
{
    if (rows == 1 || stride == n) return stage.up(dev, host, rows * n);
    return stage.up_rows(dev, host, rows, n, stride);
}

// Host arrays: upload (a shared array once), one launch, download R -- the plain entry of the side families (PlainStage).
// Of the options only `device` plays a part; the ones that change what the host arrays mean are refused.
static int resid_host(const ResidCall &hc, const int64_t *strides, double *norms, const xinv_options *opt_in)
{
    xinv_options o;
    fill_options(o, opt_in);
    int rc = resid_validate(hc, strides);
    if (rc) return rc;
    if (o.ndev > 1 || o.ndev < 0) return resid_fail("one device only (xinv_options.ndev must be 0 or 1)");
    if (o.f32_mask != 0 || o.prep_flags != 0 || o.rowconst_mask != 0)
        return resid_fail("float64 arrays in full only (f32_mask, prep_flags and rowconst_mask must be 0)");
    int nvis = 0;
    if (hipGetDeviceCount(&nvis) != hipSuccess || nvis < 1) {
        (void)hipGetLastError();
        t_err = "no HIP device available";
        return XINV_ERR_NODEV;
    }
    DeviceGuard dg;
    PlainStage stage;
    HIPCHK(dg.select(o.ndev == 1 ? o.device_ids[0] : o.device));
    const int nc = FORM[hc.kind].ncoef;
    const int64_t nb = hc.nbatch, n = hc.zc * hc.yc * hc.xc;
    auto rows = [&](int64_t s) { return (s == 0 || nb == 1) ? (int64_t)1 : nb; };
    int64_t total = nb * n + rows(hc.s[1]) * n;
    for (int q = 0; q < nc; q++)
        if (hc.c[q]) total += rows(hc.s[2 + q]) * n;
    if ((rc = stage.open((size_t)total * sizeof(double)))) return rc;
    ResidCall c = hc;
    c.R = stage.carve(nb * n); c.s[0] = n;
    {
        double *dS = stage.carve(rows(hc.s[1]) * n);
        if ((rc = resid_up(stage, dS, hc.S, rows(hc.s[1]), n, hc.s[1]))) return rc;
        c.S = dS; c.s[1] = rows(hc.s[1]) > 1 ? n : 0;
    }
    for (int q = 0; q < nc; q++) {
        if (!hc.c[q]) continue;
        const int64_t r = rows(hc.s[2 + q]);
        double *d = stage.carve(r * n);
        if ((rc = resid_up(stage, d, hc.c[q], r, n, hc.s[2 + q]))) return rc;
        c.c[q] = d; c.s[2 + q] = r > 1 ? n : 0;
    }
    stage.uploads_queued();
    if ((rc = resid_run_dev(c, norms, stage.st))) return rc;
    stage.run_done();
    if (nb == 1 || hc.s[0] == n) rc = stage.down(hc.R, c.R, nb * n);          // (packed on the host too: one plain copy)
    else rc = stage.down_rows(hc.R, c.R, nb, n, hc.s[0]);
    if (rc) return rc;
    return stage.finish(true);
}
