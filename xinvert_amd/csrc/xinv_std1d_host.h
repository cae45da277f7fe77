// xinv_std1d_host.h -- host driver of the 1-D standard form (k_std1d, xinv_std1d.h): argument checks, the chain of
// bounded launches with its polls of the pinned control-block mirror, and the host-pointer staging.  Included by
// xinv_hip.hip only, after xinv_sweep.h (ensure_mirror, member_flags, ws_ready).
#pragma once
#include "xinv_std1d.h"

#define XINV_STD1D_BUDGET 2048          /* default sweeps per launch (xinv_options.sweeps_per_launch = 0) */
#define XINV_STD1D_CHECK_EVERY 4        /* default launches between two polls (xinv_options.check_every = 0) */

struct Std1dProblem {
    double *S;
    const double *A, *B, *F;
    int64_t nbatch, xc;
    int64_t sS, sA, sB, sF;
    int BCx;
    double delxSqr, optArg, undef;
    int64_t mxLoop;
    double tolerance;
};

// XINV_PATH_DIRECT1D (xinv_tridiag_host.h): the fixed point of the sweeps from one tridiagonal solve per member
static int std1d_direct_run(const Std1dProblem &p, double *flags, const xinv_options &o, hipStream_t st);

static int std1d_validate(const Std1dProblem &p, const double *flags, const xinv_options &o)
{
    if (!p.S || !p.A || !p.B || !p.F || !flags) return fail_arg("null array or flags");
    if (p.nbatch < 1) return fail_arg("nbatch < 1");
    if (p.xc < 3) return fail_arg("the 1-D form needs xc >= 3");
    if (p.xc > XINV_STD1D_MAX_XC && o.path != XINV_PATH_DIRECT1D) {
        char b[160];
        snprintf(b, sizeof b, "the 1-D form holds at most %d points per member (16 wavefronts x 64 lanes x 8), got xc = %lld",
                 XINV_STD1D_MAX_XC, (long long)p.xc);
        t_err = b;
        return XINV_ERR_ARG;
    }
    if (!bc_ok(p.BCx)) return fail_arg("unknown boundary-condition code");
    if (p.mxLoop < 0) return fail_arg("mxLoop < 0");
    if (p.nbatch > 1 && p.sS < p.xc) return fail_arg("S batch stride smaller than one member");
    for (int64_t s : { p.sA, p.sB, p.sF })
        if (p.nbatch > 1 && s != 0 && s < p.xc) return fail_arg("coefficient batch stride must be 0 (shared) or >= xc");
    if (o.ndev > 1 || o.ndev < 0) return fail_arg("the 1-D form runs on one device (xinv_options.ndev must be 0 or 1)");
    if (o.f32_mask != 0) return fail_arg("the 1-D form takes float64 arrays only (xinv_options.f32_mask must be 0)");
    if (o.prep_flags != 0) return fail_arg("the 1-D form has no front-end passes (xinv_options.prep_flags must be 0)");
    if (o.flags & XINV_FLAG_FMA) return fail_arg("XINV_FLAG_FMA is not available for the 1-D form");
    if (o.sweeps_per_launch < 0) return fail_arg("sweeps_per_launch < 0");
    return XINV_OK;
}

// The solve on DEVICE arrays, on `st`, with the device already selected.
static int std1d_run(const Std1dProblem &p, double *flags, const xinv_options &o, hipStream_t st)
{
    if (o.path == XINV_PATH_DIRECT1D) return std1d_direct_run(p, flags, o, st);
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> lock(ws->busy);
    int rc = ws->tail.wait(st);                          // (a previous plan solve's tail may still read the control blocks)
    if (rc) return rc;
    rc = ensure_dev(&ws->ctl, &ws->ctl_cap, (size_t)p.nbatch * sizeof(XinvCtl));
    if (rc) return rc;
    rc = ensure_mirror(ws, p.nbatch);
    if (rc) return rc;
    memset(&t_stats, 0, sizeof t_stats);

    XinvCtl *hc = ws->hctl;
    for (int64_t m = 0; m < p.nbatch; m++) {
        memset(&hc[m], 0, sizeof hc[m]);
        hc[m].normPrev = DBL_MAX;                              // numbas.py:681
    }
    HIPCHK(hipMemcpyAsync(ws->ctl, hc, (size_t)p.nbatch * sizeof(XinvCtl), hipMemcpyHostToDevice, st));

    Std1dArgs a;
    memset(&a, 0, sizeof a);
    a.S = p.S; a.A = p.A; a.B = p.B; a.F = p.F;
    a.sS = p.sS; a.sA = p.sA; a.sB = p.sB; a.sF = p.sF;
    a.ctl = ws->ctl; a.nbatch = p.nbatch; a.xc = p.xc; a.BCx = p.BCx;
    int ppl = 0;
    xinv_std1d_shape(p.xc, &ppl, &a.nwave);
    a.budget = o.sweeps_per_launch > 0 ? o.sweeps_per_launch : XINV_STD1D_BUDGET;
    a.delxSqr = p.delxSqr; a.optArg = p.optArg; a.undef = p.undef;
    a.stop.mxLoop = p.mxLoop; a.stop.tolerance = p.tolerance; a.stop.stop_on_zero_norm = 1;

    // every member is done after ceil((mxLoop + 1) / budget) launches; polls in between, every `ce` launches
    const int64_t need = (p.mxLoop + 1 + a.budget - 1) / a.budget;
    const int64_t ce = o.check_every > 0 ? o.check_every : XINV_STD1D_CHECK_EVERY;
    hipEvent_t e0 = ws->ev0[0], e1 = ws->ev1[0];
    const bool timing = o.timing != 0 && e0 && e1;
    if (timing) HIPCHK(hipEventRecord(e0, st));
    int64_t launched = 0;
    while (launched < need) {
        const int64_t n = std::min<int64_t>(ce, need - launched);
        for (int64_t i = 0; i < n; i++) {
            if (xinv_launch_std1d(a, st)) return fail_arg("k_std1d: no variant for this xc");
            HIPCHK(hipGetLastError());
        }
        launched += n;
        if (launched >= need) break;
        HIPCHK(hipMemcpyAsync(hc, ws->ctl, (size_t)p.nbatch * sizeof(XinvCtl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool all = true;
        for (int64_t m = 0; m < p.nbatch && all; m++) all = hc[m].done != 0;
        if (all) break;
    }
    if (timing) HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(hc, ws->ctl, (size_t)p.nbatch * sizeof(XinvCtl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t sweeps_max = 0;
    for (int64_t m = 0; m < p.nbatch; m++) {
        member_flags(hc[m], flags + 3 * m);
        sweeps_max = std::max<int64_t>(sweeps_max, hc[m].sweeps);
    }
    t_stats.path = XINV_PATH_WAVE1D;
    t_stats.colours = (p.BCx == XINV_BC_PERIODIC && (p.xc & 1)) ? 3 : 2;
    t_stats.sweeps_per_launch = a.budget;
    t_stats.lanes = 1;
    t_stats.devices = 1;
    t_stats.sweep_launches = launched;
    t_stats.sweeps_max = sweeps_max;
    if (timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        t_stats.sweep_ms = ms;
    }
    return XINV_OK;
}

// `device` (xinv_options.device) selected for the scope of `dg`, its workspace ready for a solve
static int std1d_device(DeviceGuard &dg, int device)
{
    HIPCHK(dg.select(device));
    HIPCHK(hipGetDevice(&device));
    return ws_ready(get_ws(device));
}

static int std1d_solve_dev(const Std1dProblem &p, double *flags, const xinv_options *opt_in, hipStream_t st)
{
    xinv_options o;
    fill_options(o, opt_in);
    int rc = std1d_validate(p, flags, o);
    if (rc) return rc;
    DeviceGuard dg;
    if ((rc = std1d_device(dg, o.device))) return rc;
    return std1d_run(p, flags, o, st);
}

// Host arrays: upload (a stride-0 array once), solve, download S.  The arrays are small (a member of the sweeps is at most 64 KiB).
static int std1d_solve_host(const Std1dProblem &hp, double *flags, const xinv_options *opt_in)
{
    xinv_options o;
    fill_options(o, opt_in);
    int rc = std1d_validate(hp, flags, o);
    if (rc) return rc;
    DeviceGuard dg;
    PlainStage stage;
    if ((rc = std1d_device(dg, o.device))) return rc;
    const int64_t xc = hp.xc, nb = hp.nbatch;
    auto rows = [&](int64_t s) { return (s == 0 || nb == 1) ? (int64_t)1 : nb; };
    const int64_t nA = rows(hp.sA), nB = rows(hp.sB), nF = rows(hp.sF);
    if ((rc = stage.open((size_t)(nb + nA + nB + nF) * (size_t)xc * sizeof(double)))) return rc;
    double *dS = stage.carve(nb * xc), *dA = stage.carve(nA * xc), *dB = stage.carve(nB * xc), *dF = stage.carve(nF * xc);
    Std1dProblem p = hp;
    p.S = dS; p.A = dA; p.B = dB; p.F = dF;
    p.sS = xc; p.sA = nA > 1 ? xc : 0; p.sB = nB > 1 ? xc : 0; p.sF = nF > 1 ? xc : 0;
    if ((rc = stage.up_rows(dS, hp.S, nb, xc, hp.sS)) || (rc = stage.up_rows(dA, hp.A, nA, xc, hp.sA)) ||
        (rc = stage.up_rows(dB, hp.B, nB, xc, hp.sB)) || (rc = stage.up_rows(dF, hp.F, nF, xc, hp.sF)))
        return rc;
    stage.uploads_queued();
    if ((rc = std1d_run(p, flags, o, stage.st))) return rc;
    stage.run_done();
    if ((rc = stage.down_rows(hp.S, dS, nb, xc, hp.sS)) || (rc = stage.finish(false))) return rc;
    t_stats.host_chunks = 1;                             // (beside what std1d_run wrote)
    return XINV_OK;
}
