// xinv_fourier_host.h -- host side of the direct Fourier solves (xinv_fourier.h, xinv_cfourier.h): the factorisation of the
// row length, the per-device tables (twiddles, lambda, sigma), xinv_rowdft_f64_dev, and the one pipeline behind the one-shot
// entries of both forms and the plans -- the call and its argument checks (fourier_validate), the three transforms
// (fourier_dfts), the steps of a one-shot solve around the form's own kernels (fourier_open, fourier_checked,
// fourier_close), the standard form's solve, the device and host-pointer entries of both forms (fourier_dev, fourier_host)
// and the plans (xinv_fourier_plan_*: factor once, solve many).  Included by xinv_hip.hip only.
#pragma once
#include "xinv_fourier.h"

// One array of a call, as the checks and the staging see it.
struct FourierArr {
    double *p;                           // (only S is written)
    int64_t len;                         // doubles per member: yc * xc, or yc for a coefficient (one value per row)
    int64_t stride;                      // batch stride in elements; 0 = shared (not S)
};

// One call of either one-shot form (mk_fourier of xinv_hip.hip fills it).
struct FourierCall {
    FourierArr a[7];                     // the ABI's order: S, the coefficients (A, C / A, C, D, E, Fc), the forcing (F / G)
    int na;                              // 4 / 7
    const char *letters, *letters_and;   // the coefficients as the messages name them: "A, C" and "A and C"
    int64_t nbatch, yc, xc;
    double delx, delxSqr, ratio, ratioSqr, undef;       // (the standard form: delxSqr, ratioSqr, undef)
    double *S() const { return a[0].p; }
    const double *coef(int q) const { return a[1 + q].p; }
    const double *forcing() const { return a[na - 1].p; }
    int64_t stride(int q) const { return nbatch > 1 ? a[q].stride : 0; }      // as the kernels take it: one member has none
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

// The argument checks of every entry that takes arrays with batch strides: the one-shot forms (S, the coefficients, the
// forcing), a plan's create (A, C) and its solve (S, F).  `own0`: a[0] is S, which no two members share; `strides`: the
// caller passed its array of strides (a plan's solve takes them as two scalars: true); `letters`: the form's coefficients,
// as the stride rule names them.
static int fourier_validate(const FourierArr *a, int na, bool own0, bool strides, int64_t nbatch, int64_t yc, int64_t xc,
                            const char *letters)
{
    for (int q = 0; q < na; q++)
        if (!a[q].p) return fourier_fail("null array");
    if (!strides) return fourier_fail("null strides");
    if (nbatch < 1) return fourier_fail("nbatch < 1");
    if (yc < 3 || xc < 3) return fourier_fail("every core dimension needs at least 3 points");
    for (int q = 0; q < na; q++) {
        if (a[q].stride < 0) return fourier_fail("negative batch stride");
        if (nbatch > 1 && a[q].stride < a[q].len && !(a[q].stride == 0 && !(own0 && q == 0)))
            return fourier_fail(std::string("batch stride must be 0 (shared; not S) or at least one member (") + letters +
                                ": one value per row)");
    }
    return XINV_OK;
}

// The three transforms of a solve: forward, F * delxSqr on rows 1 .. yc-2 and S on rows 0 and yc-1 into the spectrum
// [nb][yc][K] complex; inverse, rows 1 .. yc-2 of the spectrum back to S.  `base`: the radices, the table and the row
// length; `skip`: null, or a word per member (RowDftArgs::skip) for the inverse.
struct FourierDfts { RowDftArgs fwdF, fwdS, inv; };

static FourierDfts fourier_dfts(const RowDftArgs &base, double *spec, double *S, const double *F, int64_t sS, int64_t sF,
                                int64_t nb, int64_t yc, int64_t xc, double delxSqr, const int *skip)
{
    const int64_t K = xc / 2 + 1, plane = yc * K;
    FourierDfts t;
    RowDftArgs &d = t.fwdF, &e = t.fwdS;
    d = base;
    d.spec = spec; d.s_member = 2 * plane; d.s_first = 2 * K; d.s_step = 2 * K;
    d.real = const_cast<double *>(F); d.r_member = sF; d.r_first = xc; d.r_step = xc;
    d.rpm = yc - 2; d.nrows = nb * (yc - 2); d.scale = delxSqr;
    e = d;
    e.real = S; e.r_member = sS; e.r_first = 0; e.r_step = (yc - 1) * xc;
    e.s_first = 0; e.s_step = 2 * (yc - 1) * K;
    e.rpm = 2; e.nrows = nb * 2; e.scale = 1.0;
    t.inv = d;
    t.inv.real = S; t.inv.r_member = sS; t.inv.skip = skip;
    return t;
}

static int fourier_forward(FourierDfts &t, hipStream_t st)
{
    const int rc = fourier_rowdft(t.fwdF, false, st);
    return rc ? rc : fourier_rowdft(t.fwdS, false, st);
}

// flags[m] = {overflow, 0, 0} from the members' overflow words on the host
static void fourier_flags(double *flags, const int *ovf, int64_t nb)
{
    for (int64_t m = 0; m < nb; m++) {
        flags[3 * m] = ovf[m] ? 1.0 : 0.0;
        flags[3 * m + 1] = 0.0;
        flags[3 * m + 2] = 0.0;
    }
}

// ------------------------------------------------------------------ the one-shot solves on device arrays
// A one-shot solve of either form is fourier_open, the form's check kernel, fourier_checked, the form's own kernels around
// fourier_forward and the inverse transform, fourier_close.  The spectrum and the form's factors live in the workspace's one
// buffer: the device's lock covers the call, the event covers what the call leaves queued when it returns early with an
// error; the next user of the buffer -- on any stream -- is ordered behind it, or waits on the host before the buffer grows.
struct FourierRun {
    Workspace *ws = nullptr;
    std::unique_lock<std::recursive_mutex> lock;         // the device's, to the end of the solve
    RowDftArgs dft;                      // radices, table, row length: what the solve's transforms share
    const double *tab = nullptr;         // twiddles [xc] complex, lambda [K], sigma [K]
    double *spec = nullptr, *rest = nullptr;             // the spectrum [nbatch][yc][K] complex; behind it, what the form asked for
    int *bad = nullptr, *ovf = nullptr;  // undef counts [nbatch], overflow words [nbatch]: zeroed
    bool timing = false;
};

// With the device already selected: the row length's radices, the workspace behind its last user with `rest` doubles behind
// the spectrum, the tables, the status words zeroed on `st`.
static int fourier_open(FourierRun &r, const FourierCall &c, size_t rest, hipStream_t st)
{
    memset(&r.dft, 0, sizeof r.dft);
    int rc = fourier_factor(c.xc, r.dft.radix, &r.dft.npass);
    if (rc) return rc;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = r.ws = get_ws(device);
    r.lock = std::unique_lock<std::recursive_mutex>(ws->busy);
    const size_t nb = (size_t)c.nbatch, spec = nb * (size_t)(c.yc * (c.xc / 2 + 1)) * 2;
    const size_t need = (spec + rest) * sizeof(double), words = nb * 2 * sizeof(int);
    if ((rc = ws->four_user.wait(st, !ws->four || ws->four_cap < need))) return rc;
    if ((rc = ensure_dev(&ws->four, &ws->four_cap, need))) return rc;
    if ((rc = ensure_dev(&ws->four_cnt, &ws->four_cnt_cap, words))) return rc;
    if ((rc = ensure_pinned(&ws->h_four_cnt, &ws->h_four_cnt_cap, words, hipHostMallocDefault))) return rc;
    if ((rc = fourier_tables(ws, c.xc, &r.tab))) return rc;
    memset(&t_stats, 0, sizeof t_stats);
    r.dft.tw = r.tab; r.dft.n = (int)c.xc;
    r.spec = ws->four; r.rest = ws->four + spec;
    r.bad = ws->four_cnt; r.ovf = ws->four_cnt + nb;
    HIPCHK(hipMemsetAsync(ws->four_cnt, 0, words, st));
    return XINV_OK;
}

// One of the solve's two host synchronisations: `nb` status words to the pinned mirror, behind the workspace's event
static int fourier_mirror(Workspace *ws, const int *words, int64_t nb, hipStream_t st)
{
    const int rc = ws->four_user.mark(st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ws->h_four_cnt, words, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ws->four_user.pending = false;                       // (`st` has drained)
    return XINV_OK;
}

// Behind the form's check kernel, before anything is written: the undef counts, the refusal (`reads`: the arrays the solve
// reads on the interior rows), the start of the timed span.
static int fourier_checked(FourierRun &r, int64_t nb, const char *reads, hipStream_t st)
{
    Workspace *ws = r.ws;
    HIPCHK(hipGetLastError());
    const int rc = fourier_mirror(ws, r.bad, nb, st);
    if (rc) return rc;
    for (int64_t m = 0; m < nb; m++)
        if (ws->h_four_cnt[m])
            return fourier_fail("member " + std::to_string(m) + " holds undef at " + std::to_string(ws->h_four_cnt[m]) +
                                " of the points the solve reads (" + reads + " on the interior rows, S on rows 0 and yc-1): "
                                "a masked problem is for the sweeps");
    r.timing = ws->ev0[0] && ws->ev1[0];
    if (r.timing) HIPCHK(hipEventRecord(ws->ev0[0], st));
    return XINV_OK;
}

// Behind the inverse transform: the end of the timed span, the overflow words, the flags and the statistics of a solve of
// `launches` kernels.
static int fourier_close(FourierRun &r, int64_t nb, int launches, double *flags, hipStream_t st)
{
    Workspace *ws = r.ws;
    if (r.timing) HIPCHK(hipEventRecord(ws->ev1[0], st));
    const int rc = fourier_mirror(ws, r.ovf, nb, st);
    if (rc) return rc;
    fourier_flags(flags, ws->h_four_cnt, nb);
    t_stats.path = XINV_PATH_FOURIER2D;
    t_stats.lanes = 1;
    t_stats.devices = 1;
    t_stats.sweep_launches = launches;
    if (r.timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ws->ev0[0], ws->ev1[0]));
        t_stats.sweep_ms = ms;
    }
    return XINV_OK;
}

typedef int (*FourierSolve)(const FourierCall &, double *, hipStream_t);

// The standard form: the workspace holds the forward factors [nbatch][yc][K] behind the spectrum
static int fourier_run_dev(const FourierCall &c, double *flags, hipStream_t st)
{
    FourierRun r;
    const int64_t nb = c.nbatch, yc = c.yc, xc = c.xc, K = xc / 2 + 1;
    int rc = fourier_open(r, c, (size_t)nb * (size_t)(yc * K), st);
    if (rc) return rc;
    FourierCheckArgs k;
    memset(&k, 0, sizeof k);
    k.S = c.S(); k.A = c.coef(0); k.C = c.coef(1); k.F = c.forcing();
    k.sS = c.stride(0); k.sA = c.stride(1); k.sC = c.stride(2); k.sF = c.stride(3);
    k.yc = yc; k.xc = xc; k.undef = c.undef; k.bad = r.bad;
    xinv_launch_fourier_check(k, nb, st);
    if ((rc = fourier_checked(r, nb, "F, A, C", st))) return rc;

    FourierDfts d = fourier_dfts(r.dft, r.spec, c.S(), c.forcing(), k.sS, k.sF, nb, yc, xc, c.delxSqr, nullptr);
    if ((rc = fourier_forward(d, st))) return rc;
    FourierTriArgs t;                                    // one tridiagonal system per wavenumber
    memset(&t, 0, sizeof t);
    t.spec = r.spec; t.gam = r.rest; t.A = k.A; t.C = k.C; t.lam = r.tab + 2 * xc;
    t.sA = k.sA; t.sC = k.sC; t.yc = yc; t.K = K; t.ratioSqr = c.ratioSqr; t.ovf = r.ovf;
    xinv_launch_fourier_tri(t, nb, st);
    HIPCHK(hipGetLastError());
    if ((rc = fourier_rowdft(d.inv, true, st))) return rc;
    return fourier_close(r, nb, 4, flags, st);
}

static int fourier_dev(const FourierCall &c, const int64_t *strides, double *flags, FourierSolve run, hipStream_t st)
{
    if (!flags) return fourier_fail("null array");
    const int rc = fourier_validate(c.a, c.na, true, strides != nullptr, c.nbatch, c.yc, c.xc, c.letters);
    return rc ? rc : run(c, flags, st);
}

// Host arrays: upload (a shared array once), the solve, download S -- the plain entry of the side families (PlainStage).  Of
// the options only `device` plays a part.  On an error nothing is downloaded: the caller's S is untouched.
static int fourier_host(const FourierCall &hc, const int64_t *strides, double *flags, FourierSolve run, const xinv_options *opt_in)
{
    xinv_options o;
    fill_options(o, opt_in);
    if (!flags) return fourier_fail("null array");
    int rc = fourier_validate(hc.a, hc.na, true, strides != nullptr, hc.nbatch, hc.yc, hc.xc, hc.letters);
    if (rc) return rc;
    if (o.ndev > 1 || o.ndev < 0) return fourier_fail("one device only (xinv_options.ndev must be 0 or 1)");
    if (o.f32_mask != 0 || o.prep_flags != 0 || o.rowconst_mask != 0)
        return fourier_fail(std::string("float64 arrays only, ") + hc.letters_and +
                            " one value per row (f32_mask, prep_flags and rowconst_mask must be 0)");
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
    const int64_t nb = hc.nbatch;
    int64_t rows[7], total = 0;
    for (int q = 0; q < hc.na; q++) {
        rows[q] = (q == 0 || (nb > 1 && hc.a[q].stride != 0)) ? nb : 1;
        total += rows[q] * hc.a[q].len;
    }
    if ((rc = stage.open((size_t)total * sizeof(double)))) return rc;
    FourierCall c = hc;
    for (int q = 0; q < hc.na; q++) {
        const int64_t len = hc.a[q].len;
        c.a[q].p = stage.carve(rows[q] * len);
        c.a[q].stride = (q == 0 || rows[q] > 1) ? len : 0;
        if ((rc = stage.up_rows(c.a[q].p, hc.a[q].p, rows[q], len, hc.a[q].stride))) return rc;
    }
    stage.uploads_queued();
    if ((rc = run(c, flags, stage.st))) return rc;
    stage.run_done();
    if ((rc = stage.down_rows(hc.S(), c.S(), nb, hc.a[0].len, hc.a[0].stride))) return rc;
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
    const FourierArr a[2] = { { const_cast<double *>(A), yc, strides ? strides[0] : 0 },
                              { const_cast<double *>(C), yc, strides ? strides[1] : 0 } };
    int rc = fourier_validate(a, 2, false, strides != nullptr, nbatch, yc, xc, "A, C");
    if (rc) return rc;
    RowDftArgs d;
    memset(&d, 0, sizeof d);
    if ((rc = fourier_factor(xc, d.radix, &d.npass))) return rc;
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
    const int64_t nb = p->nbatch, yc = p->yc, xc = p->xc, K = p->K, plane = yc * K, n = yc * xc;
    const FourierArr a[2] = { { S, n, sS }, { const_cast<double *>(F), n, sF } };
    if (S && F && (sS < 0 || sF < 0)) return fourier_fail("negative batch stride");      // (either, before the rule on S)
    int rc = fourier_validate(a, 2, true, true, nb, yc, xc, "A, C");
    if (rc) return rc;
    if (nb == 1) sS = sF = 0;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    if (device != p->device)
        return fourier_fail("the plan lives on device " + std::to_string(p->device) + ", the current device is " +
                            std::to_string(device));
    std::lock_guard<std::mutex> lock(p->mu);
    if (p->solved) HIPCHK(hipStreamWaitEvent(st, p->ev, 0));      // the spectrum and the status words are the plan's
    int *bad = p->cnt, *ovf = p->cnt + nb;
    HIPCHK(hipMemsetAsync(p->cnt, 0, (size_t)nb * 2 * sizeof(int), st));
    FourierCheckArgs k;
    memset(&k, 0, sizeof k);
    k.S = S; k.A = p->A; k.C = p->C; k.F = F;
    k.sS = sS; k.sA = p->pA; k.sC = p->pC; k.sF = sF;
    k.yc = yc; k.xc = xc; k.undef = p->undef; k.bad = bad;
    xinv_launch_fourier_check(k, nb, st);
    HIPCHK(hipGetLastError());

    FourierDfts d = fourier_dfts(p->dft, p->spec, S, F, sS, sF, nb, yc, xc, p->delxSqr, bad);
    if ((rc = fourier_forward(d, st))) return rc;

    FourierSubstArgs t;
    memset(&t, 0, sizeof t);
    t.spec = p->spec; t.fac = p->fac; t.A = p->A;
    t.sA = p->pA; t.sfac = p->nset > 1 ? 2 * plane : 0;
    t.yc = yc; t.K = K; t.ratioSqr = p->ratioSqr; t.ovf = ovf;
    xinv_launch_fourier_subst(t, nb, st);
    HIPCHK(hipGetLastError());

    if ((rc = fourier_rowdft(d.inv, true, st))) return rc;
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
    fourier_flags(flags, p->h_cnt + nb, nb);
    for (int64_t m = 0; m < nb; m++) {
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
