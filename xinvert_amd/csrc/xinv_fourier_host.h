// xinv_fourier_host.h -- host side of the direct Fourier solve (xinv_fourier.h): the factorisation of the row length, the
// per-device tables (twiddles, lambda) and workspace, the argument checks of xinv_fourier_standard_2d_f64_dev / _batched and
// of xinv_rowdft_f64_dev, and the host-pointer staging.  Included by xinv_hip.hip only.
#pragma once
#include "xinv_fourier.h"

struct FourierCall {
    double *S;
    const double *A, *C, *F;
    int64_t nbatch, yc, xc;
    int64_t s[4];                        // batch strides of S, A, C, F (elements; 0 = shared, not S)
    double delxSqr, ratioSqr, undef;
};

static int fourier_fail(const std::string &what)
{
    t_err = "xinv_fourier: " + what;
    return XINV_ERR_ARG;
}

// n = 4^a 2^b 3^c 5^d within the LDS budget -> the passes' radices; otherwise the error names n and what is wrong with it
static int fourier_factor(int64_t n, int *radix, int *npass)
{
    if (n < 2) return fourier_fail("a row needs at least 2 points, got " + std::to_string(n));
    int64_t r = n;
    int np = 0;
    const int order[4] = { 4, 2, 3, 5 };
    for (int q = 0; q < 4; q++)
        while (r % order[q] == 0) {
            if (np < XINV_DFT_MAX_PASS) radix[np] = order[q];
            np++;
            r /= order[q];
        }
    if (r != 1) {
        int64_t f = 7;
        while (r % f != 0 && f * f <= r) f += 2;
        if (r % f != 0) f = r;
        return fourier_fail("the row length " + std::to_string(n) + " has the prime factor " + std::to_string(f) +
                            " (the transform takes products of 2, 3 and 5)");
    }
    if (n > XINV_DFT_MAX_N || np > XINV_DFT_MAX_PASS)
        return fourier_fail("the row length " + std::to_string(n) + " is beyond the transform's LDS budget (at most " +
                            std::to_string(XINV_DFT_MAX_N) + " points)");
    *npass = np;
    return XINV_OK;
}

// The tables of one row length: [n] complex exp(-2 pi i t / n), then [K] lambda_k = 4 sin^2(pi k / n), rounded once from
// long double.  Built on the first call with that length and kept for the life of the process (at most 96 KB each), so a
// queued kernel never sees its table change.  Under the workspace's lock.
static int fourier_tables(Workspace *ws, int64_t n, const double **tab)
{
    for (const auto &e : ws->four_tab)
        if (e.first == n) { *tab = e.second; return XINV_OK; }
    const int64_t K = n / 2 + 1;
    std::vector<double> h((size_t)(2 * n + K));
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int64_t t = 0; t < n; t++) {
        const long double ang = 2.0L * pi * (long double)t / (long double)n;
        h[2 * t] = (double)cosl(ang);
        h[2 * t + 1] = (double)-sinl(ang);
    }
    for (int64_t k = 0; k < K; k++) {
        const long double s = sinl(pi * (long double)k / (long double)n);
        h[2 * n + k] = (double)(4.0L * s * s);
    }
    double *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, h.size() * sizeof(double)));
    const hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); HIPCHK(e); }
    ws->four_tab.push_back({ n, d });
    *tab = d;
    return XINV_OK;
}

static int fourier_rowdft(RowDftArgs &a, bool inverse, hipStream_t st)
{
    const int e = xinv_launch_rowdft(a, inverse, st);
    if (e) HIPCHK((hipError_t)e);
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

// xinv_rowdft_f64_dev: `nrows` rows, packed; only queued (the tables are never rewritten: nothing to order)
static int rowdft_dev(double *out, const double *in, int64_t nrows, int64_t n, int inverse, hipStream_t st)
{
    if (!out || !in) return fourier_fail("null array");
    if (out == in) return fourier_fail("the transform is not in place");
    if (nrows < 1) return fourier_fail("nrows < 1");
    RowDftArgs a;
    memset(&a, 0, sizeof a);
    int rc = fourier_factor(n, a.radix, &a.npass);
    if (rc) return rc;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> lock(ws->busy);
    if ((rc = fourier_tables(ws, n, &a.tw))) return rc;
    const int64_t K = n / 2 + 1;
    a.real = inverse ? out : const_cast<double *>(in);
    a.spec = inverse ? const_cast<double *>(in) : out;
    a.nrows = nrows; a.rpm = nrows;
    a.r_step = n; a.s_step = 2 * K;
    a.scale = 1.0;
    a.n = (int)n;
    return fourier_rowdft(a, inverse != 0, st);
}

static int fourier_validate(const FourierCall &c, const int64_t *strides, const double *flags)
{
    if (!c.S || !c.A || !c.C || !c.F || !flags) return fourier_fail("null array");
    if (!strides) return fourier_fail("null strides");
    if (c.nbatch < 1) return fourier_fail("nbatch < 1");
    if (c.yc < 3 || c.xc < 3) return fourier_fail("every core dimension needs at least 3 points");
    const int64_t n = c.yc * c.xc;
    const int64_t need[4] = { n, c.yc, c.yc, n };
    for (int q = 0; q < 4; q++) {
        if (c.s[q] < 0) return fourier_fail("negative batch stride");
        if (c.nbatch > 1 && c.s[q] < need[q] && !(q > 0 && c.s[q] == 0))
            return fourier_fail("batch stride must be 0 (shared; not S) or at least one member (A, C: one value per row)");
    }
    return XINV_OK;
}

// Device arrays, on `st`, with the device already selected.  The spectrum and the forward factors live in the workspace's one
// buffer: the device's lock covers the call, the event covers what the call leaves queued when it returns early with an
// error; the next user of the buffer -- on any stream -- is ordered behind it, or waits on the host before the buffer grows.
static int fourier_run_dev(const FourierCall &c, double *flags, hipStream_t st)
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
    const size_t need = (size_t)nb * (size_t)plane * 3 * sizeof(double);
    if ((rc = ws->four_user.wait(st, !ws->four || ws->four_cap < need))) return rc;
    if ((rc = ensure_dev(&ws->four, &ws->four_cap, need))) return rc;
    if ((rc = ensure_dev(&ws->four_cnt, &ws->four_cnt_cap, (size_t)nb * 2 * sizeof(int)))) return rc;
    if ((rc = ensure_pinned(&ws->h_four_cnt, &ws->h_four_cnt_cap, (size_t)nb * 2 * sizeof(int), hipHostMallocDefault))) return rc;
    const double *tab = nullptr;
    if ((rc = fourier_tables(ws, xc, &tab))) return rc;
    memset(&t_stats, 0, sizeof t_stats);
    const int64_t sS = nb > 1 ? c.s[0] : 0, sA = nb > 1 ? c.s[1] : 0, sC = nb > 1 ? c.s[2] : 0, sF = nb > 1 ? c.s[3] : 0;
    double *spec = ws->four, *gam = ws->four + (size_t)nb * plane * 2;
    int *bad = ws->four_cnt, *ovf = ws->four_cnt + nb;

    // 1. the check pass, before anything is written
    HIPCHK(hipMemsetAsync(ws->four_cnt, 0, (size_t)nb * 2 * sizeof(int), st));
    FourierCheckArgs k;
    memset(&k, 0, sizeof k);
    k.S = c.S; k.A = c.A; k.C = c.C; k.F = c.F;
    k.sS = sS; k.sA = sA; k.sC = sC; k.sF = sF;
    k.yc = yc; k.xc = xc; k.undef = c.undef; k.bad = bad;
    xinv_launch_fourier_check(k, nb, st);
    HIPCHK(hipGetLastError());
    if ((rc = ws->four_user.mark(st))) return rc;
    HIPCHK(hipMemcpyAsync(ws->h_four_cnt, bad, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ws->four_user.pending = false;
    for (int64_t m = 0; m < nb; m++)
        if (ws->h_four_cnt[m])
            return fourier_fail("member " + std::to_string(m) + " holds undef at " + std::to_string(ws->h_four_cnt[m]) +
                                " of the points the solve reads (F, A, C on the interior rows, S on rows 0 and yc-1): "
                                "a masked problem is for the sweeps");

    // 2. forward transforms: F * delxSqr on rows 1 .. yc-2, S on rows 0 and yc-1
    hipEvent_t e0 = ws->ev0[0], e1 = ws->ev1[0];
    const bool timing = e0 && e1;
    if (timing) HIPCHK(hipEventRecord(e0, st));
    d.tw = tab; d.n = (int)xc;
    d.spec = spec; d.s_member = 2 * plane; d.s_first = 2 * K; d.s_step = 2 * K;
    d.real = const_cast<double *>(c.F); d.r_member = sF; d.r_first = xc; d.r_step = xc;
    d.rpm = yc - 2; d.nrows = nb * (yc - 2); d.scale = c.delxSqr;
    if ((rc = fourier_rowdft(d, false, st))) return rc;
    RowDftArgs e = d;
    e.real = c.S; e.r_member = sS; e.r_first = 0; e.r_step = (yc - 1) * xc;
    e.s_first = 0; e.s_step = 2 * (yc - 1) * K;
    e.rpm = 2; e.nrows = nb * 2; e.scale = 1.0;
    if ((rc = fourier_rowdft(e, false, st))) return rc;

    // 3. one tridiagonal system per wavenumber
    FourierTriArgs t;
    memset(&t, 0, sizeof t);
    t.spec = spec; t.gam = gam; t.A = c.A; t.C = c.C; t.lam = tab + 2 * xc;
    t.sA = sA; t.sC = sC; t.yc = yc; t.K = K; t.ratioSqr = c.ratioSqr; t.ovf = ovf;
    xinv_launch_fourier_tri(t, nb, st);
    HIPCHK(hipGetLastError());

    // 4. back to rows 1 .. yc-2 of S
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
    t_stats.sweep_launches = 4;
    if (timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        t_stats.sweep_ms = ms;
    }
    return XINV_OK;
}

static int fourier_dev(const FourierCall &c, const int64_t *strides, double *flags, hipStream_t st)
{
    int rc = fourier_validate(c, strides, flags);
    if (rc) return rc;
    return fourier_run_dev(c, flags, st);
}

// Host arrays: upload (a shared array once), the solve, download S -- the plain entry of the side families (PlainStage).  Of
// the options only `device` plays a part.  On an error nothing is downloaded: the caller's S is untouched.
static int fourier_host(const FourierCall &hc, const int64_t *strides, double *flags, const xinv_options *opt_in)
{
    xinv_options o;
    fill_options(o, opt_in);
    int rc = fourier_validate(hc, strides, flags);
    if (rc) return rc;
    if (o.ndev > 1 || o.ndev < 0) return fourier_fail("one device only (xinv_options.ndev must be 0 or 1)");
    if (o.f32_mask != 0 || o.prep_flags != 0 || o.rowconst_mask != 0)
        return fourier_fail("float64 arrays only, A and C one value per row (f32_mask, prep_flags and rowconst_mask must be 0)");
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
    const double *src[3] = { hc.A, hc.C, hc.F };
    const int64_t len[3] = { hc.yc, hc.yc, n };
    int64_t rows[3], total = nb * n;
    for (int q = 0; q < 3; q++) {
        rows[q] = (nb == 1 || hc.s[1 + q] == 0) ? 1 : nb;
        total += rows[q] * len[q];
    }
    if ((rc = stage.open((size_t)total * sizeof(double)))) return rc;
    FourierCall c = hc;
    c.S = stage.carve(nb * n); c.s[0] = n;
    if ((rc = stage.up_rows(c.S, hc.S, nb, n, hc.s[0]))) return rc;
    const double *dev[3] = {};
    for (int q = 0; q < 3; q++) {
        double *at = stage.carve(rows[q] * len[q]);
        if ((rc = stage.up_rows(at, src[q], rows[q], len[q], hc.s[1 + q]))) return rc;
        dev[q] = at;
        c.s[1 + q] = rows[q] > 1 ? len[q] : 0;
    }
    c.A = dev[0]; c.C = dev[1]; c.F = dev[2];
    stage.uploads_queued();
    if ((rc = fourier_run_dev(c, flags, stage.st))) return rc;
    stage.run_done();
    if ((rc = stage.down_rows(hc.S, c.S, nb, n, hc.s[0]))) return rc;
    return stage.finish(false);
}
