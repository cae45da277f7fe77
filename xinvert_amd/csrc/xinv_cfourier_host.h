// xinv_cfourier_host.h -- host side of the direct Fourier solve of the 2-D general form (xinv_cfourier.h): the argument
// checks of xinv_fourier_general_2d_f64_dev / _batched, the solve on device arrays and the host-pointer staging.  The row
// transform, its tables and the workspace are those of xinv_fourier_host.h.  Included by xinv_hip.hip only, after it.
#pragma once
#include "xinv_cfourier.h"

struct CFourierCall {
    double *S;
    const double *c[5];                  // A, C, D, E, Fc: one value per row
    const double *G;
    int64_t nbatch, yc, xc;
    int64_t s[7];                        // batch strides of S, A, C, D, E, Fc, G (elements; 0 = shared, not S)
    double delx, delxSqr, ratio, ratioSqr, undef;
};

static int cfourier_validate(const CFourierCall &c, const int64_t *strides, const double *flags)
{
    if (!c.S || !c.G || !flags) return fourier_fail("null array");
    for (int q = 0; q < 5; q++)
        if (!c.c[q]) return fourier_fail("null array");
    if (!strides) return fourier_fail("null strides");
    if (c.nbatch < 1) return fourier_fail("nbatch < 1");
    if (c.yc < 3 || c.xc < 3) return fourier_fail("every core dimension needs at least 3 points");
    const int64_t n = c.yc * c.xc;
    for (int q = 0; q < 7; q++) {
        const int64_t need = (q == 0 || q == 6) ? n : c.yc;
        if (c.s[q] < 0) return fourier_fail("negative batch stride");
        if (c.nbatch > 1 && c.s[q] < need && !(q > 0 && c.s[q] == 0))
            return fourier_fail("batch stride must be 0 (shared; not S) or at least one member (A, C, D, E, F: one value per row)");
    }
    return XINV_OK;
}

// Device arrays, on `st`, with the device already selected.  The workspace's one buffer holds the spectrum
// [nbatch][yc][K] complex, then the factors [nset][2][yc][K] complex, then lo and up [nset][2][yc]; it is locked, ordered
// and grown as fourier_run_dev does.
static int cfourier_run_dev(const CFourierCall &c, double *flags, hipStream_t st)
{
    RowDftArgs d;
    memset(&d, 0, sizeof d);
    int rc = fourier_factor(c.xc, d.radix, &d.npass);
    if (rc) return rc;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> lock(ws->busy);
    const int64_t nb = c.nbatch, yc = c.yc, xc = c.xc, K = xc / 2 + 1, plane = yc * K;
    int64_t sc[5];
    bool shared = true;
    for (int q = 0; q < 5; q++) {
        sc[q] = nb > 1 ? c.s[1 + q] : 0;
        shared = shared && sc[q] == 0;
    }
    const int64_t nset = shared ? 1 : nb;
    const size_t need = ((size_t)nb * (size_t)plane * 2 + (size_t)nset * (size_t)plane * 4 + (size_t)nset * 2 * (size_t)yc) * sizeof(double);
    if ((rc = ws->four_user.wait(st, !ws->four || ws->four_cap < need))) return rc;
    if ((rc = ensure_dev(&ws->four, &ws->four_cap, need))) return rc;
    if ((rc = ensure_dev(&ws->four_cnt, &ws->four_cnt_cap, (size_t)nb * 2 * sizeof(int)))) return rc;
    if ((rc = ensure_pinned(&ws->h_four_cnt, &ws->h_four_cnt_cap, (size_t)nb * 2 * sizeof(int), hipHostMallocDefault))) return rc;
    const double *tab = nullptr;
    if ((rc = fourier_tables(ws, xc, &tab))) return rc;
    memset(&t_stats, 0, sizeof t_stats);
    const int64_t sS = nb > 1 ? c.s[0] : 0, sG = nb > 1 ? c.s[6] : 0;
    double *spec = ws->four, *fac = spec + (size_t)nb * plane * 2, *lu = fac + (size_t)nset * plane * 4;
    int *bad = ws->four_cnt, *ovf = ws->four_cnt + nb;

    // 1. the check pass, before anything is written
    HIPCHK(hipMemsetAsync(ws->four_cnt, 0, (size_t)nb * 2 * sizeof(int), st));
    CFourierCheckArgs k;
    memset(&k, 0, sizeof k);
    k.S = c.S; k.G = c.G; k.sS = sS; k.sG = sG;
    for (int q = 0; q < 5; q++) { k.c[q] = c.c[q]; k.sc[q] = sc[q]; }
    k.yc = yc; k.xc = xc; k.undef = c.undef; k.bad = bad;
    xinv_launch_fourier_gcheck(k, nb, st);
    HIPCHK(hipGetLastError());
    if ((rc = ws->four_user.mark(st))) return rc;
    HIPCHK(hipMemcpyAsync(ws->h_four_cnt, bad, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ws->four_user.pending = false;
    for (int64_t m = 0; m < nb; m++)
        if (ws->h_four_cnt[m])
            return fourier_fail("member " + std::to_string(m) + " holds undef at " + std::to_string(ws->h_four_cnt[m]) +
                                " of the points the solve reads (G, A, C, D, E, F on the interior rows, S on rows 0 and yc-1): "
                                "a masked problem is for the sweeps");

    // 2. the factors of every wavenumber's system, per coefficient set
    hipEvent_t e0 = ws->ev0[0], e1 = ws->ev1[0];
    const bool timing = e0 && e1;
    if (timing) HIPCHK(hipEventRecord(e0, st));
    CFourierFactorArgs f;
    memset(&f, 0, sizeof f);
    f.fac = fac; f.lu = lu;
    f.A = c.c[0]; f.C = c.c[1]; f.D = c.c[2]; f.E = c.c[3]; f.Fc = c.c[4];
    f.sA = sc[0]; f.sC = sc[1]; f.sD = sc[2]; f.sE = sc[3]; f.sFc = sc[4];
    f.lam = tab + 2 * xc; f.sig = tab + 2 * xc + K;
    f.yc = yc; f.K = K;
    f.delx = c.delx; f.delxSqr = c.delxSqr; f.ratio = c.ratio; f.ratioSqr = c.ratioSqr;
    xinv_launch_fourier_cfactor(f, nset, st);
    HIPCHK(hipGetLastError());

    // 3. forward transforms: G * delxSqr on rows 1 .. yc-2, S on rows 0 and yc-1
    d.tw = tab; d.n = (int)xc;
    d.spec = spec; d.s_member = 2 * plane; d.s_first = 2 * K; d.s_step = 2 * K;
    d.real = const_cast<double *>(c.G); d.r_member = sG; d.r_first = xc; d.r_step = xc;
    d.rpm = yc - 2; d.nrows = nb * (yc - 2); d.scale = c.delxSqr;
    if ((rc = fourier_rowdft(d, false, st))) return rc;
    RowDftArgs e = d;
    e.real = c.S; e.r_member = sS; e.r_first = 0; e.r_step = (yc - 1) * xc;
    e.s_first = 0; e.s_step = 2 * (yc - 1) * K;
    e.rpm = 2; e.nrows = nb * 2; e.scale = 1.0;
    if ((rc = fourier_rowdft(e, false, st))) return rc;

    // 4. the substitution, one complex tridiagonal system per wavenumber and member
    CFourierSubstArgs t;
    memset(&t, 0, sizeof t);
    t.spec = spec; t.fac = fac; t.lu = lu;
    t.sfac = nset > 1 ? 4 * plane : 0; t.slu = nset > 1 ? 2 * yc : 0;
    t.yc = yc; t.K = K; t.ovf = ovf;
    xinv_launch_fourier_csubst(t, nb, st);
    HIPCHK(hipGetLastError());

    // 5. back to rows 1 .. yc-2 of S
    d.real = c.S; d.r_member = sS;
    if ((rc = fourier_rowdft(d, true, st))) return rc;
    if (timing) HIPCHK(hipEventRecord(e1, st));
    if ((rc = ws->four_user.mark(st))) return rc;
    HIPCHK(hipMemcpyAsync(ws->h_four_cnt, ovf, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ws->four_user.pending = false;                       // (`st` has drained)
    for (int64_t m = 0; m < nb; m++) {
        flags[3 * m] = ws->h_four_cnt[m] ? 1.0 : 0.0;
        flags[3 * m + 1] = 0.0;
        flags[3 * m + 2] = 0.0;
    }
    t_stats.path = XINV_PATH_FOURIER2D;
    t_stats.lanes = 1;
    t_stats.devices = 1;
    t_stats.sweep_launches = 5;
    if (timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        t_stats.sweep_ms = ms;
    }
    return XINV_OK;
}

static int cfourier_dev(const CFourierCall &c, const int64_t *strides, double *flags, hipStream_t st)
{
    int rc = cfourier_validate(c, strides, flags);
    if (rc) return rc;
    return cfourier_run_dev(c, flags, st);
}

// Host arrays: upload (a shared array once), the solve, download S -- the plain entry of the side families (PlainStage).  Of
// the options only `device` plays a part.  On an error nothing is downloaded: the caller's S is untouched.
static int cfourier_host(const CFourierCall &hc, const int64_t *strides, double *flags, const xinv_options *opt_in)
{
    xinv_options o;
    fill_options(o, opt_in);
    int rc = cfourier_validate(hc, strides, flags);
    if (rc) return rc;
    if (o.ndev > 1 || o.ndev < 0) return fourier_fail("one device only (xinv_options.ndev must be 0 or 1)");
    if (o.f32_mask != 0 || o.prep_flags != 0 || o.rowconst_mask != 0)
        return fourier_fail("float64 arrays only, A, C, D, E and F one value per row (f32_mask, prep_flags and rowconst_mask must be 0)");
    {
        int radix[XINV_DFT_MAX_PASS], np = 0;
        if ((rc = fourier_factor(hc.xc, radix, &np))) return rc;          // (before anything is uploaded)
    }
    int nvis = 0;
    if (hipGetDeviceCount(&nvis) != hipSuccess || nvis < 1) {
        (void)hipGetLastError();
        t_err = "no HIP device available";
        return XINV_ERR_NODEV;
    }
    DeviceGuard dg;
    PlainStage stage;
    HIPCHK(dg.select(o.ndev == 1 ? o.device_ids[0] : o.device));
    const int64_t nb = hc.nbatch, n = hc.yc * hc.xc;
    const double *src[6] = { hc.c[0], hc.c[1], hc.c[2], hc.c[3], hc.c[4], hc.G };
    int64_t len[6], rows[6], total = nb * n;
    for (int q = 0; q < 6; q++) {
        len[q] = q < 5 ? hc.yc : n;
        rows[q] = (nb == 1 || hc.s[1 + q] == 0) ? 1 : nb;
        total += rows[q] * len[q];
    }
    if ((rc = stage.open((size_t)total * sizeof(double)))) return rc;
    CFourierCall c = hc;
    c.S = stage.carve(nb * n); c.s[0] = n;
    if ((rc = stage.up_rows(c.S, hc.S, nb, n, hc.s[0]))) return rc;
    const double *dev[6] = {};
    for (int q = 0; q < 6; q++) {
        double *at = stage.carve(rows[q] * len[q]);
        if ((rc = stage.up_rows(at, src[q], rows[q], len[q], hc.s[1 + q]))) return rc;
        dev[q] = at;
        c.s[1 + q] = rows[q] > 1 ? len[q] : 0;
    }
    for (int q = 0; q < 5; q++) c.c[q] = dev[q];
    c.G = dev[5];
    stage.uploads_queued();
    if ((rc = cfourier_run_dev(c, flags, stage.st))) return rc;
    stage.run_done();
    if ((rc = stage.down_rows(hc.S, c.S, nb, n, hc.s[0]))) return rc;
    return stage.finish(false);
}
