// xinv_fd_host.h -- host side of the finite-difference operators (k_fd, xinv_fd.h): the call's term list checked and
// turned into kernel arguments, the launch geometry, and the host-pointer staging.  Included by xinv_hip.hip only.
#pragma once
#include "xinv_fd.h"

#define XINV_FD_ITERM 15
#define XINV_FD_DTERM 6

// One call as the ABI describes it (include/xinv.h, "finite differences").  The pointers are device pointers here.
struct FdCall {
    const double *const *in;
    int nin;
    double *const *out;
    int nout;
    int ndim;
    const int64_t *shape;
    int mode, nterms;
    const int64_t *iterm;
    const double *dterm;
    const double *tab;
    int64_t ntab;
    int mask_axis;
    int64_t mask_off;
};

static int fd_fail(const char *what)
{
    t_err = std::string("xinv_fd: ") + what;
    return XINV_ERR_ARG;
}

// Checks everything but the array pointers' targets; fills `a` (pointers into c.tab / c.in / c.out) and the element count.
static int fd_args(const FdCall &c, FdArgs &a, int64_t *elems, int64_t *nblocks)
{
    memset(&a, 0, sizeof a);
    if (c.ndim < 1 || c.ndim > 16 || !c.shape) return fd_fail("ndim must be 1..16 with a shape");
    int64_t total = 1;
    for (int d = 0; d < c.ndim; ++d) {
        if (c.shape[d] < 1) return fd_fail("every shape entry must be >= 1");
        if (total > INT64_MAX / c.shape[d]) return fd_fail("shape overflows int64");
        total *= c.shape[d];
    }
    if (c.mode < XINV_FD_EACH || c.mode > XINV_FD_DIFF) return fd_fail("unknown mode");
    if (c.nterms < 1 || c.nterms > XINV_FD_MAXT) return fd_fail("nterms must be 1..4");
    if (c.mode == XINV_FD_DIFF && c.nterms != 2) return fd_fail("mode DIFF takes exactly two terms");
    if (c.nin < 1 || c.nin > XINV_FD_MAXIN || !c.in) return fd_fail("nin must be 1..3");
    if (c.nout != (c.mode == XINV_FD_EACH ? c.nterms : 1) || !c.out) return fd_fail("nout must be nterms (EACH) or 1");
    for (int k = 0; k < c.nin; ++k)
        if (!c.in[k]) return fd_fail("null input");
    for (int k = 0; k < c.nout; ++k)
        if (!c.out[k]) return fd_fail("null output");
    if (!c.iterm || !c.dterm) return fd_fail("null term description");
    if (c.ntab < 0 || (c.ntab > 0 && !c.tab)) return fd_fail("null table");
    const int64_t nx = c.shape[c.ndim - 1];
    // rows between two neighbours along axis d (0: the last axis)
    auto srow = [&](int d) -> int64_t {
        int64_t s = 1;
        for (int e = d + 1; e < c.ndim - 1; ++e) s *= c.shape[e];
        return d == c.ndim - 1 ? 0 : s;
    };
    auto estride = [&](int d) -> int64_t {
        int64_t s = 1;
        for (int e = d + 1; e < c.ndim; ++e) s *= c.shape[e];
        return s;
    };
    auto table = [&](int64_t off, int64_t len, const double **p) -> int {
        if (off < 0 || len < 0 || off > c.ntab - len) return fd_fail("table offset out of range");
        *p = c.tab + off;
        return XINV_OK;
    };
    auto bc_ok = [](int64_t b) { return b >= XINV_FD_BC_FIXED && b <= XINV_FD_BC_REFLECT; };
    for (int t = 0; t < c.nterms; ++t) {
        const int64_t *I = c.iterm + (size_t)t * XINV_FD_ITERM;
        const double *D = c.dterm + (size_t)t * XINV_FD_DTERM;
        FdTerm &T = a.t[t];
        const int64_t kind = I[0], in = I[1], ax = I[3], bcl = I[4], bcr = I[5], metric = I[7], pax = I[8], sax = I[9];
        if (kind < XINV_FD_CENTER || kind > XINV_FD_SECOND) return fd_fail("unknown scheme (kind)");
        if (in < 0 || in >= c.nin) return fd_fail("term input out of range");
        if (ax < 0 || ax >= c.ndim) return fd_fail("derivative axis out of range");
        const int64_t n = c.shape[ax];
        if (n < 2) return fd_fail("the derivative axis needs at least 2 points");
        if (!bc_ok(bcl) || !bc_ok(bcr)) return fd_fail("unknown boundary condition");
        if ((bcl == XINV_FD_BC_PERIODIC) != (bcr == XINV_FD_BC_PERIODIC))
            return fd_fail("'periodic' cannot be mixed with other BCs");
        if (metric < 0 || metric > 2 || (metric && kind != XINV_FD_SECOND)) return fd_fail("bad metric");
        if (pax < -1 || pax >= c.ndim || sax < -1 || sax >= c.ndim) return fd_fail("table axis out of range");
        T.src = c.in[in];
        T.kind = (int)kind; T.neg = I[2] != 0; T.bcl = (int)bcl; T.bcr = (int)bcr;
        T.uniform = I[6] != 0; T.metric = (int)metric;
        T.n = n; T.srow = srow((int)ax); T.stride = estride((int)ax);
        T.fl = D[0]; T.fr = D[1]; T.twodx = D[2]; T.scs = D[3]; T.msc = D[4]; T.R = D[5];
        int rc;
        const bool centre = kind == XINV_FD_CENTER || metric == 2;
        if (centre && !T.uniform) {
            const double *w;
            if ((rc = table(I[10], 3 * n, &w))) return rc;
            T.wa = w; T.wb = w + n; T.wc = w + 2 * n;
        }
        if (kind != XINV_FD_CENTER && (rc = table(I[11], n, &T.dd))) return rc;
        if (pax >= 0) {
            const int64_t pn = c.shape[pax];
            if ((rc = table(I[12], pn, &T.pw))) return rc;
            T.psame = pax == ax; T.pn = pn; T.psrow = srow((int)pax);
        }
        if (sax >= 0) {
            const int64_t sn = c.shape[sax];
            if ((rc = table(I[13], sn, &T.sc))) return rc;
            T.sn = sn; T.ssrow = srow((int)sax);
        }
        if (metric == 2 && (rc = table(I[14], n, &T.tn))) return rc;
    }
    if (c.mask_axis >= 0) {
        if (c.mode != XINV_FD_SUM || c.mask_axis >= c.ndim) return fd_fail("a mask needs mode SUM and a valid axis");
        a.mn = c.shape[c.mask_axis]; a.msrow = srow(c.mask_axis);
        int rc = table(c.mask_off, a.mn, &a.mask);
        if (rc) return rc;
    }
    for (int k = 0; k < c.nout; ++k) a.out[k] = c.out[k];
    a.nt = c.nterms; a.mode = c.mode;
    a.nx = nx; a.nr = total / nx;
    a.nbx = (nx + XINV_FD_WG - 1) / XINV_FD_WG;
    // rows per workgroup: long marches (the row halo is 2 in rb) while keeping some 4096 workgroups in the grid
    // (and at most 2^24 workgroups: grid x 256 lanes stays below 2^32)
    const int64_t maxb = ((int64_t)1 << 24) - 1;
    if (a.nbx > maxb) return fd_fail("the last axis is too long");
    a.rb = std::max<int64_t>(1, std::min<int64_t>(32, a.nr * a.nbx / 4096));
    a.rb = std::max<int64_t>(a.rb, (a.nr + maxb / a.nbx - 1) / (maxb / a.nbx));
    const int64_t nby = (a.nr + a.rb - 1) / a.rb;
    *elems = total;
    *nblocks = a.nbx * nby;
    return XINV_OK;
}

// Device arrays, on `st`, with the device already selected.
static int fd_run_dev(const FdCall &c, hipStream_t st)
{
    FdArgs a;
    int64_t elems = 0, nblocks = 0;
    int rc = fd_args(c, a, &elems, &nblocks);
    if (rc) return rc;
    if (xinv_launch_fd(a, nblocks, st)) return fd_fail("no kernel for this term count");
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

// Host arrays: upload inputs and tables, one launch, download the outputs.
static int fd_run_host(const FdCall &hc)
{
    FdArgs a;
    int64_t elems = 0, nblocks = 0;
    int rc = fd_args(hc, a, &elems, &nblocks);          // (argument checks before any allocation)
    if (rc) return rc;
    PlainStage stage;
    if ((rc = stage.open((size_t)(hc.nin + hc.nout) * (size_t)elems * sizeof(double) + (size_t)hc.ntab * sizeof(double) + 64)))
        return rc;
    const double *din[XINV_FD_MAXIN];
    double *dout[XINV_FD_MAXT];
    for (int k = 0; k < hc.nin; ++k) {
        double *at = stage.carve(elems);
        if ((rc = stage.up(at, hc.in[k], elems))) return rc;
        din[k] = at;
    }
    for (int k = 0; k < hc.nout; ++k) dout[k] = stage.carve(elems);
    double *dtab = stage.carve(hc.ntab);
    if (hc.ntab && (rc = stage.up(dtab, hc.tab, hc.ntab))) return rc;
    FdCall c = hc;
    c.in = din; c.out = dout; c.tab = dtab;
    stage.uploads_queued();
    if ((rc = fd_run_dev(c, stage.st))) return rc;
    stage.run_done();
    for (int k = 0; k < hc.nout; ++k)
        if ((rc = stage.down(hc.out[k], dout[k], elems))) return rc;
    return stage.finish(true);
}
