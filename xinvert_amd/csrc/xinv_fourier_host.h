// xinv_fourier_host.h -- host side of the direct Fourier solve (xinv_fourier.h): the factorisation of the row length, the
// per-device tables (twiddles, lambda) and workspace, the argument checks of xinv_fourier_standard_2d_f64_dev / _batched and
// of xinv_rowdft_f64_dev, the host-pointer staging, and the plans (xinv_fourier_plan_*: factor once, solve many).  Included by
// xinv_hip.hip only.
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

// The tables of one row length: [n] complex exp(-2 pi i t / n), then [K] lambda_k = 4 sin^2(pi k / n), then [K] sigma_k =
// sin(2 pi k / n) (the general form's: xinv_cfourier.h; sigma_0 and, for even n, sigma_{n/2} are exactly 0), rounded once
// from long double.  Built on the first call with that length and kept for the life of the process (at most 128 KB each),
// so a queued kernel never sees its table change.  Under the workspace's lock.
static int fourier_tables(Workspace *ws, int64_t n, const double **tab)
{
    for (const auto &e : ws->four_tab)
        if (e.first == n) { *tab = e.second; return XINV_OK; }
    const int64_t K = n / 2 + 1;
    std::vector<double> h((size_t)(2 * n + 2 * K));
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int64_t t = 0; t < n; t++) {
        const long double ang = 2.0L * pi * (long double)t / (long double)n;
        h[2 * t] = (double)cosl(ang);
        h[2 * t + 1] = (double)-sinl(ang);
    }
    for (int64_t k = 0; k < K; k++) {
        const long double s = sinl(pi * (long double)k / (long double)n);
        h[2 * n + k] = (double)(4.0L * s * s);
        h[2 * n + K + k] = (k == 0 || 2 * k == n) ? 0.0 : (double)sinl(2.0L * pi * (long double)k / (long double)n);
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

// ------------------------------------------------------------------ plans: one operator, many forcings
// What depends on A, C, ratioSqr and xc alone -- the factors inv_j, gamma_j of every wavenumber's system -- is computed once
// (k_fourier_factor) and kept with the plan's own copies of A and C, its own spectrum buffer and its own status words, so a
// solve takes neither the device's workspace nor its lock and never stops the host.  The plan's event is recorded behind
// every solve: the next solve (on any stream) is ordered behind it, status and destroy wait for it on the host.
#define XINV_FPLAN_MAGIC 0x58465031u     /* "XFP1" */
struct xinv_fourier_plan {
    unsigned magic = XINV_FPLAN_MAGIC;
    int device = 0;
    int64_t nbatch = 0, yc = 0, xc = 0, K = 0, nset = 0;
    int64_t pA = 0, pC = 0;              // member strides of the plan's copies (0 = shared)
    double delxSqr = 0, ratioSqr = 0, undef = 0;
    double *coef = nullptr;              // A [nbatch or 1][yc], then C [nbatch or 1][yc]
    const double *A = nullptr, *C = nullptr;
    double *fac = nullptr;               // [nset][2][yc][K]: inv, gamma
    double *spec = nullptr;              // [nbatch][yc][K] complex
    int *cnt = nullptr, *h_cnt = nullptr;   // undef counts [nbatch], then overflow words [nbatch]; the pinned mirror
    const double *tab = nullptr;         // the row length's twiddles [xc] complex, then lambda [K] (the workspace owns them)
    RowDftArgs dft;                      // radices and table: what every transform of the plan shares
    hipEvent_t ev = nullptr;
    bool solved = false;                 // `ev` has been recorded
    std::mutex mu;
};

static void fplan_free(xinv_fourier_plan *p)
{
    if (p->ev) {
        if (p->solved) (void)hipEventSynchronize(p->ev);
        (void)hipEventDestroy(p->ev);
    }
    if (p->coef) (void)hipFree(p->coef);
    if (p->fac) (void)hipFree(p->fac);
    if (p->spec) (void)hipFree(p->spec);
    if (p->cnt) (void)hipFree(p->cnt);
    if (p->h_cnt) (void)hipHostFree(p->h_cnt);
    p->magic = 0;
    delete p;
}

// The allocations, the copies of A and C with their undef count, the factors.  On an error the caller frees the plan.
static int fplan_fill(xinv_fourier_plan *p, const double *A, const double *C, int64_t sA, int64_t sC, hipStream_t st)
{
    const int64_t nb = p->nbatch, yc = p->yc, K = p->K, plane = yc * K;
    const int64_t nA = sA ? nb : 1, nC = sC ? nb : 1;
    HIPCHK(hipMalloc((void **)&p->coef, (size_t)(nA + nC) * yc * sizeof(double)));
    double *dA = p->coef, *dC = p->coef + nA * yc;
    HIPCHK(hipMemcpy2DAsync(dA, (size_t)yc * sizeof(double), A, (size_t)(sA ? sA : yc) * sizeof(double),
                            (size_t)yc * sizeof(double), (size_t)nA, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpy2DAsync(dC, (size_t)yc * sizeof(double), C, (size_t)(sC ? sC : yc) * sizeof(double),
                            (size_t)yc * sizeof(double), (size_t)nC, hipMemcpyDeviceToDevice, st));
    std::vector<double> h((size_t)((nA + nC) * yc));
    HIPCHK(hipMemcpyAsync(h.data(), p->coef, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t m = 0; m < nb; m++) {
        const double *a = h.data() + (nA > 1 ? m * yc : 0), *c = h.data() + nA * yc + (nC > 1 ? m * yc : 0);
        int64_t cnt = 0;
        for (int64_t j = 1; j <= yc - 1; j++) cnt += a[j] == p->undef;
        for (int64_t j = 1; j <= yc - 2; j++) cnt += c[j] == p->undef;
        if (cnt)
            return fourier_fail("member " + std::to_string(m) + " holds undef at " + std::to_string(cnt) +
                                " of the points the plan reads (A on rows 1 .. yc-1, C on rows 1 .. yc-2): "
                                "a masked problem is for the sweeps");
    }
    p->A = dA; p->C = dC;
    p->pA = nA > 1 ? yc : 0; p->pC = nC > 1 ? yc : 0;
    p->nset = (nA > 1 || nC > 1) ? nb : 1;
    HIPCHK(hipMalloc((void **)&p->fac, (size_t)p->nset * (size_t)plane * 2 * sizeof(double)));
    HIPCHK(hipMalloc((void **)&p->spec, (size_t)nb * (size_t)plane * 2 * sizeof(double)));
    HIPCHK(hipMalloc((void **)&p->cnt, (size_t)nb * 2 * sizeof(int)));
    HIPCHK(hipHostMalloc((void **)&p->h_cnt, (size_t)nb * 2 * sizeof(int), hipHostMallocDefault));
    memset(p->h_cnt, 0, (size_t)nb * 2 * sizeof(int));
    HIPCHK(hipEventCreateWithFlags(&p->ev, hipEventDisableTiming));
    FourierFactorArgs f;
    memset(&f, 0, sizeof f);
    f.fac = p->fac; f.A = p->A; f.C = p->C; f.lam = p->tab + 2 * p->xc;
    f.sA = p->pA; f.sC = p->pC; f.yc = yc; f.K = K; f.ratioSqr = p->ratioSqr;
    xinv_launch_fourier_factor(f, p->nset, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));                    // the plan is ready for a solve on any stream
    return XINV_OK;
}

static int fplan_create(xinv_fourier_plan **out, const double *A, const double *C, int64_t nbatch, const int64_t *strides,
                        int64_t yc, int64_t xc, double delxSqr, double ratioSqr, double undef, hipStream_t st)
{
    if (!out) return fourier_fail("null plan");
    *out = nullptr;
    if (!A || !C) return fourier_fail("null array");
    if (!strides) return fourier_fail("null strides");
    if (nbatch < 1) return fourier_fail("nbatch < 1");
    if (yc < 3 || xc < 3) return fourier_fail("every core dimension needs at least 3 points");
    for (int q = 0; q < 2; q++) {
        if (strides[q] < 0) return fourier_fail("negative batch stride");
        if (nbatch > 1 && strides[q] != 0 && strides[q] < yc)
            return fourier_fail("batch stride must be 0 (shared; not S) or at least one member (A, C: one value per row)");
    }
    RowDftArgs d;
    memset(&d, 0, sizeof d);
    int rc = fourier_factor(xc, d.radix, &d.npass);
    if (rc) return rc;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    const double *tab = nullptr;
    {
        Workspace *ws = get_ws(device);
        std::lock_guard<std::recursive_mutex> lock(ws->busy);
        if ((rc = fourier_tables(ws, xc, &tab))) return rc;
    }
    xinv_fourier_plan *p = new xinv_fourier_plan();
    p->device = device;
    p->nbatch = nbatch; p->yc = yc; p->xc = xc; p->K = xc / 2 + 1;
    p->delxSqr = delxSqr; p->ratioSqr = ratioSqr; p->undef = undef;
    p->tab = tab;
    d.tw = tab; d.n = (int)xc;
    p->dft = d;
    if ((rc = fplan_fill(p, A, C, nbatch > 1 ? strides[0] : 0, nbatch > 1 ? strides[1] : 0, st))) {
        fplan_free(p);
        return rc;
    }
    *out = p;
    return XINV_OK;
}

// Only queues on `st`: zero the status words, the check pass, the two forward transforms into the plan's spectrum, the
// substitution, the inverse transform (a member with a non-zero undef count is skipped: its S stays), the status words to
// their pinned mirror, the plan's event.
static int fplan_solve(xinv_fourier_plan *p, double *S, const double *F, int64_t sS, int64_t sF, hipStream_t st)
{
    if (!p || p->magic != XINV_FPLAN_MAGIC) return fourier_fail("xinv_fourier_plan_solve_f64_dev: not a live plan");
    if (!S || !F) return fourier_fail("null array");
    const int64_t nb = p->nbatch, yc = p->yc, xc = p->xc, K = p->K, plane = yc * K, n = yc * xc;
    if (sS < 0 || sF < 0) return fourier_fail("negative batch stride");
    if (nb > 1 && (sS < n || (sF != 0 && sF < n)))
        return fourier_fail("batch stride must be 0 (shared; not S) or at least one member (A, C: one value per row)");
    if (nb == 1) sS = sF = 0;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    if (device != p->device)
        return fourier_fail("the plan lives on device " + std::to_string(p->device) + ", the current device is " +
                            std::to_string(device));
    std::lock_guard<std::mutex> lock(p->mu);
    if (p->solved) HIPCHK(hipStreamWaitEvent(st, p->ev, 0));      // the spectrum and the status words are the plan's
    int *bad = p->cnt, *ovf = p->cnt + nb;
    int rc;
    HIPCHK(hipMemsetAsync(p->cnt, 0, (size_t)nb * 2 * sizeof(int), st));
    FourierCheckArgs k;
    memset(&k, 0, sizeof k);
    k.S = S; k.A = p->A; k.C = p->C; k.F = F;
    k.sS = sS; k.sA = p->pA; k.sC = p->pC; k.sF = sF;
    k.yc = yc; k.xc = xc; k.undef = p->undef; k.bad = bad;
    xinv_launch_fourier_check(k, nb, st);
    HIPCHK(hipGetLastError());

    RowDftArgs d = p->dft;
    d.spec = p->spec; d.s_member = 2 * plane; d.s_first = 2 * K; d.s_step = 2 * K;
    d.real = const_cast<double *>(F); d.r_member = sF; d.r_first = xc; d.r_step = xc;
    d.rpm = yc - 2; d.nrows = nb * (yc - 2); d.scale = p->delxSqr;
    if ((rc = fourier_rowdft(d, false, st))) return rc;
    RowDftArgs e = d;
    e.real = S; e.r_member = sS; e.r_first = 0; e.r_step = (yc - 1) * xc;
    e.s_first = 0; e.s_step = 2 * (yc - 1) * K;
    e.rpm = 2; e.nrows = nb * 2; e.scale = 1.0;
    if ((rc = fourier_rowdft(e, false, st))) return rc;

    FourierSubstArgs t;
    memset(&t, 0, sizeof t);
    t.spec = p->spec; t.fac = p->fac; t.A = p->A;
    t.sA = p->pA; t.sfac = p->nset > 1 ? 2 * plane : 0;
    t.yc = yc; t.K = K; t.ratioSqr = p->ratioSqr; t.ovf = ovf;
    xinv_launch_fourier_subst(t, nb, st);
    HIPCHK(hipGetLastError());

    d.real = S; d.r_member = sS; d.skip = bad;
    if ((rc = fourier_rowdft(d, true, st))) return rc;
    HIPCHK(hipMemcpyAsync(p->h_cnt, p->cnt, (size_t)nb * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(p->ev, st));
    p->solved = true;
    return XINV_OK;
}

// Waits for the plan's last solve; flags[m] = {overflow, 0, 0}, bad[m] = the member's undef count (both filled before the error)
static int fplan_status(xinv_fourier_plan *p, double *flags, int *bad)
{
    if (!p || p->magic != XINV_FPLAN_MAGIC) return fourier_fail("xinv_fourier_plan_status: not a live plan");
    if (!flags) return fourier_fail("null array");
    std::lock_guard<std::mutex> lock(p->mu);
    if (p->solved) HIPCHK(hipEventSynchronize(p->ev));
    const int64_t nb = p->nbatch;
    int64_t first = -1;
    for (int64_t m = 0; m < nb; m++) {
        flags[3 * m] = p->h_cnt[nb + m] ? 1.0 : 0.0;
        flags[3 * m + 1] = 0.0;
        flags[3 * m + 2] = 0.0;
        if (bad) bad[m] = p->h_cnt[m];
        if (p->h_cnt[m] && first < 0) first = m;
    }
    if (first >= 0)
        return fourier_fail("member " + std::to_string(first) + " holds undef at " + std::to_string(p->h_cnt[first]) +
                            " of the points the solve reads (F on the interior rows, S on rows 0 and yc-1); its S was "
                            "left as it was, the other members are solved: a masked problem is for the sweeps");
    return XINV_OK;
}

static int fplan_destroy(xinv_fourier_plan *p)
{
    if (!p) return XINV_OK;
    if (p->magic != XINV_FPLAN_MAGIC) return fourier_fail("xinv_fourier_plan_destroy: not a live plan");
    { std::lock_guard<std::mutex> lock(p->mu); }         // (a solve that is still queuing finishes first)
    fplan_free(p);
    return XINV_OK;
}
