// xinv_hostptr.h -- the host-pointer entries of libxinv_hip.so: upload -> solve -> download pipelined over member
// chunks (uploader / downloader threads through the library's pinned staging rings, two chunk solves in flight),
// and the in-call split of the batch axis over several GPUs (one host thread per device, bound to the GPU's NUMA
// node).  Included by xinv_hip.hip only, after xinv_sweep.h.
#pragma once

// ------------------------------------------------------------------ the solve (host ptrs)
struct HostEvents {                                   // destroyed on every return path
    std::vector<hipEvent_t> e;
    ~HostEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    int make(hipEvent_t *out, bool timing)
    {
        hipEvent_t x = nullptr;
        HIPCHK(timing ? hipEventCreate(&x) : hipEventCreateWithFlags(&x, hipEventDisableTiming));
        e.push_back(x);
        *out = x;
        return XINV_OK;
    }
};

// Member chunks of the upload / solve / download pipeline: sizes in members, in batch order.
// Chunking hides PCIe time behind sweeps (chunk c+1 travels and chunk c-1 returns while chunk c sweeps) but
// costs twice: every chunk repeats the once-per-solve detection / planning passes (~0.5 ms), and a chunk fills
// the 256 CUs less evenly than the whole batch (the 3-D kernels run ceil(workgroups / 256) rounds of one
// workgroup per CU).
static std::vector<int64_t> host_chunks(const Problem &p, const xinv_options &opt)
{
    const int64_t nb = p.nbatch;
    std::vector<int64_t> out;
    if (nb <= 1) { out.push_back(nb); return out; }
    if (opt.host_chunk > 0) {
        const int64_t mc = std::min<int64_t>(opt.host_chunk, nb);
        for (int64_t m0 = 0; m0 < nb; m0 += mc) out.push_back(std::min(mc, nb - m0));
        return out;
    }
    if (opt.host_chunk < 0) {                              // -k: a ramp 1, 2, 4, .. up to k members, then chunks of k
        const int64_t kmax = -(int64_t)opt.host_chunk;
        int64_t left = nb, c = 1;
        while (left > 0) { const int64_t t = std::min(std::min(c, kmax), left); out.push_back(t); left -= t; c *= 2; }
        return out;
    }
    const int64_t n = p.zc * p.yc * p.xc;
    int per_member = 1;                                   // S
    for (int q = 0; q < p.ncoef; q++) per_member += (p.c[q] && p.sc[q] != 0 && !((p.rowconst >> q) & 1u)) ? 1 : 0;
    const double member_bytes = (double)n * 8.0 * per_member;
    const double total = member_bytes * (double)nb;
    // Round 5: TWO chunk solves are in flight on the device at a time (solve_host_one), so the holes a small chunk leaves
    // on the 256 CUs are filled by its neighbour's launches, and what remains to be minimised is the exposed first
    // upload / last download against the fixed cost of a chunk (~0.5 ms of planning, launches of few workgroups).
    // Measured (profiles/r05_host_pipeline.txt): C5, 15 volumes -- 1 chunk 212 ms, [4, 7, 4] (round 4's split) 172,
    // chunks of 2 volumes 161, of 1 volume 200; C4, 8 members -- 1 chunk 15.4 ms, chunks of 2 members 14.1, of 1: 17.2.
    if (is3d(p.kind)) {
        if (total < 100663296.0 || nb < 4) { out.push_back(nb); return out; }
        // Round 6 (profiles/r06_host_pipeline.txt; C5 x 15, ms): chunks of three volumes, THREE chunk solves in flight, each
        // one launch chain (no lanes inside a chunk): 148; chunks of two, two in flight -- round 5 -- 160-167; three
        // in flight 155; chunks of four 154-168; ramps 1, 2, 4, .. 163-173.  The remainder LAST.
        const int64_t per = nb >= 6 ? 3 : 2;
        for (int64_t m0 = 0; m0 < nb; m0 += per) out.push_back(std::min(per, nb - m0));
        return out;
    }
    // 2-D forms, end of round 6 (TWO chunk solves in flight, the copy streams at high priority; wall ms of 500 sweeps,
    // profiles/r06_host_pipeline.txt): 1440 x 720 general form (17 MB a member) x 3 members -- chunks of 1: 8.5, one chunk 7.5;
    // x 6 -- 1: 13.3, 2: 12.0, 3: 12.9; x 8 -- 1: 17.2, 2: 14.0, 4: 15.9; x 12 -- 2: 19.0, 3: 22.4, 4: 20.2, 6: 19.3; x 16 --
    // 2: 23.9, 4: 26.2, 8: 23.6; x 32 -- 2: 42.8, 4: 49.0, 8: 41.5, 16: 40.6; x 64 -- 8: 82.0, 16: 71.7, 32: 72.8.  3600 x 1800
    // standard form (104 MB a member) x 2 -- 1: 16.7, one chunk 18.1; x 3 -- 1: 20.5, one chunk 25.1; x 8 -- 1: 43.7, 2: 45.8,
    // 4: 48.4.  Odd chunks lose (their two lanes are uneven).  Large members travel one by one; small ones in pairs up to 16
    // members, in four chunks beyond.  (FOUR chunk solves in flight are faster in a fresh process -- C4 x 8 13.1 against
    // 13.7, x 16 21.6 --, but in a process that has run resident solves before -- bench.py -- every second process lands on
    // 15-16 ms: the chains then share the runtime's hardware queues unevenly; two in flight give 12.8-13.1 every time.)
    if (total < 50331648.0) { out.push_back(nb); return out; }
    int64_t per;
    if (member_bytes >= 67108864.0) per = 1;
    else if (nb < 4) { out.push_back(nb); return out; }
    else per = nb <= 16 ? 2 : ((std::max<int64_t>(2, nb / 4) + 1) & ~(int64_t)1);
    for (int64_t m0 = 0; m0 < nb; m0 += per) out.push_back(std::min(per, nb - m0));
    return out;
}

// One device: upload -> solve -> download, pipelined over member chunks by three actors:
//   the UPLOADER thread stages every upload through the library's pinned ring (xinv_host.h) in batch order --
//     shared coefficient arrays first, then S and the per-member arrays chunk by chunk, an event after each chunk;
//   the CALLING thread solves chunk c as soon as its event is recorded (the compute stream waits for ITS event only,
//     so chunk c+1 travels while chunk c sweeps);
//   the DOWNLOADER thread brings each solved chunk's S back through its own ring, overlapping the sweeps of chunk c+1.
// Both DMA directions and the CUs are busy at once; what stays exposed is the first chunk's upload and the
// last chunk's download.  Members are independent (reference core.py:129: no cross-slice state), so the
// chunking cannot change any result.
struct HostActors {                                   // joins the helper threads and drains the streams on EVERY return path
    std::thread up, down;
    std::vector<std::thread> solvers;                 // helper threads: chunk solves in flight beside the calling thread's
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> chunk_ready;                    // set by the uploader once chunk c's event is recorded
    std::deque<std::function<int()>> dq;              // download jobs
    bool d_closed = false, abort = false;
    int u_rc = 0, d_rc = 0, s2_rc = 0;                // (s2: the first failing helper solver thread's verdict -- kept here: this
    std::string u_err, d_err, s2_err;                 //  object outlives the threads on every return path)
    std::vector<hipStream_t> streams;
    void close_downloads() { { std::lock_guard<std::mutex> lk(mu); d_closed = true; } cv.notify_all(); }
    ~HostActors()
    {
        { std::lock_guard<std::mutex> lk(mu); abort = true; d_closed = true; }
        cv.notify_all();
        for (auto &t : solvers) if (t.joinable()) t.join();      // (before the downloader: they still queue download jobs)
        if (up.joinable()) up.join();
        if (down.joinable()) down.join();
        for (hipStream_t s : streams) (void)hipStreamSynchronize(s);      // nothing of this call stays in flight
    }
};

// a host array's bytes over the batch -- the extent a pinning covers: arr 0 = S, q + 1 = coefficient q
static size_t host_bytes(const Problem &p, int arr)
{
    const int64_t stride = arr == 0 ? p.sS : p.sc[arr - 1];
    const int64_t len = (arr > 0 && ((p.rowconst >> (arr - 1)) & 1u)) ? p.zc * p.yc : p.zc * p.yc * p.xc;
    return (size_t)((p.nbatch - 1) * stride + len) * (((p.f32 >> arr) & 1u) ? 4 : 8);
}

// the sweep stats of one more chunk solve (one after another: sweep_ms summed) or device (side by side: the longest)
static void merge_sweep_stats(xinv_stats &acc, const xinv_stats &s, bool side_by_side)
{
    acc.sweep_launches += s.sweep_launches;
    acc.sweeps_max = std::max(acc.sweeps_max, s.sweeps_max);
    acc.sweep_ms = side_by_side ? std::max(acc.sweep_ms, s.sweep_ms) : acc.sweep_ms + s.sweep_ms;
    acc.recovered_members += s.recovered_members;
}

// The state of one device's host-pointer call, shared by its steps below.  Members are destroyed in reverse order of
// declaration, so `act` must stay the LAST member: its destructor joins the helper threads and drains the streams before
// the upload ops, events, buffers and registrations they use go.
struct HostCall {
    Problem &p;                                       // the caller's arrays
    Problem d;                                        // the same problem on the device
    double *flags;
    const xinv_options &opt;
    xinv_options o1;                                  // what every chunk solve runs with
    std::chrono::steady_clock::time_point wall0;      // entry: the trace's clock
    int device, fq, ninfl = 1;                        // fq: the forcing (last array); ninfl: chunk solves in flight
    int64_t n, hsS, nchunk;                           // points of a member; the host stride of S; member chunks
    Workspace *ws; DevPool *pool = nullptr;
    Pinned pin;                                       // opt-in registration of the caller's arrays (off by default)
    hipStream_t sup = nullptr, sdn = nullptr, scp = nullptr;
    HostEvents ev;
    hipEvent_t e_up0, e_up1, e_dn0, e_dn1;            // the copy streams' first and last copies
    std::vector<int64_t> chunks, first;               // member chunks; first[c]: chunk c's first member
    std::vector<hipEvent_t> e_chunk;                  // recorded on `sup` behind chunk c's uploads
    std::vector<std::function<int()>> shared_ops;     // the uploader's work: before the first chunk, then chunk by chunk
    std::vector<std::vector<std::function<int()>>> chunk_ops;
    bool rolling, roll2d, per_member[10], do_prep = false;   // per_member[q]: coefficient q travels with its chunk
    float *tmpC[10], *tmpS_up = nullptr, *tmpS_dn = nullptr;   // float32 scratch of coefficient q, of S (nullptr: float64)
    double *d_rowscale = nullptr;
    std::vector<Workspace *> wss; std::vector<hipStream_t> scps;     // chunk solve slot k: workspace, compute stream
    xinv_stats acc{}; bool acc_set = false;           // the chunk solves' stats, merged
    unsigned shared_um = 0;                           // shared arrays an earlier chunk's plan found constant along x
    HostActors act;                                   // (the last member: see above)

    HostCall(Problem &p_, double *fl, const xinv_options &o, const Pinned *outer, int dev, Workspace *w,
             std::chrono::steady_clock::time_point t0)
        : p(p_), d(p_), flags(fl), opt(o), o1(o), wall0(t0), device(dev), fq(p_.ncoef - 1), n(p_.zc * p_.yc * p_.xc),
          hsS(p_.nbatch > 1 ? p_.sS : n), ws(w)
    {
        pin.outer = outer;                            // (a per-device call of a multi-device solve uses the parent's registrations)
        pin.enabled = outer == nullptr && (Pinned::env_allowed() || (opt.flags & XINV_FLAG_PIN_HOST));
        // The rolling batch (round 6; roll() below): ONE chain of launches over the members that have arrived and are not done
        // yet, instead of one solve per chunk.  For the standard 3-D form with shared coefficient arrays (its plan reads nothing
        // of a member's own), on the streaming path, where the planner is left to itself.
        // (xinv_options.host_inflight = -1 takes it for any batch of two or more: the tests' small volumes)
        roll2d = (p.kind == KIND_STD2D || p.kind == KIND_GEN2D);     // (2-D: only where no tile is fully masked, see roll)
        rolling = (p.kind == KIND_STD3D || roll2d) && (opt.host_chunk == 0 || opt.host_inflight < 0) && opt.host_inflight <= 0 &&
                  opt.path != XINV_PATH_COLOUR && !(p.BCx == XINV_BC_PERIODIC && (p.xc & 1) && p.xc < 64) &&
                  ((!roll2d && p.nbatch >= 4 && (double)n * 16.0 * (double)p.nbatch >= 100663296.0) || (opt.host_inflight < 0 && p.nbatch >= 2));
        // (2-D forms roll on request only -- host_inflight = -1 --: C4 x 8, 500 sweeps: 15.0 ms rolling against 13.4 in chunks of
        //  two members, two chunk solves in flight (7.6 resident).  The 2-D tiling is chosen for the whole batch -- 240 workgroups
        //  per member where the chip holds a thousand --, so a launch over two members of eight takes two thirds of the time of
        //  one over all eight, there are no lanes, and the two plans cost a millisecond: profiles/r06_host_pipeline.txt)
        for (int q = 0; q + 1 < p.ncoef; q++) rolling = rolling && (p.c[q] ? (p.nbatch == 1 || p.sc[q] == 0) : (roll2d && q == 1));
        // (3-D: a volume per upload event; 2-D: the chunk scheme's chunks -- it takes over when the forcing has masked tiles)
        chunks = (rolling && !roll2d) ? std::vector<int64_t>((size_t)p.nbatch, 1) : host_chunks(p, opt);
        nchunk = (int64_t)chunks.size();
        first.assign((size_t)nchunk + 1, 0);
        for (int64_t c = 0; c < nchunk; c++) first[(size_t)c + 1] = first[(size_t)c] + chunks[(size_t)c];
    }
    static bool trace_on() { static const bool on = XINV_ENV_INT("XINV_HOST_TRACE", 0) != 0; return on; }
    void trace(const char *what, long long k = -1) const   // XINV_HOST_TRACE=1: the call's phases on stderr (ms since entry)
    {
        if (!trace_on()) return;
        const double ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        if (k < 0) fprintf(stderr, "[xinv host %8.3f ms] %s\n", ms_, what);
        else fprintf(stderr, "[xinv host %8.3f ms] %s #%lld\n", ms_, what, k);
    }
    // with act.mu held: wait until chunk c has been uploaded (c < 0: no wait), then the uploader's verdict
    int wait_chunk(std::unique_lock<std::mutex> &lk, int64_t c)
    {
        if (c >= 0) act.cv.wait(lk, [&] { return act.chunk_ready[(size_t)c] != 0 || act.abort; });
        if (act.u_rc) { t_err = act.u_err; return act.u_rc; }
        if (act.abort) { t_err = "host-pointer solve aborted"; return XINV_ERR_HIP; }
        return XINV_OK;
    }
    int wait_chunk(int64_t c) { std::unique_lock<std::mutex> lk(act.mu); return wait_chunk(lk, c); }
    // host <-> device on `sup` (up) or `sdn`: `members` pieces of `len` elements of `esz` bytes (host stride hstride,
    // device stride len), one copy where they are contiguous
    int copy_pieces(bool up, const void *host, const void *dev, int64_t members, int64_t hstride, int64_t len, size_t esz)
    {
        auto one = [&](char *h, char *dv, size_t bytes) -> int {
            if (pin.covers(h, bytes)) {                // registered in place: the DMA reads / writes the caller's memory
                if (up) HIPCHK(hipMemcpyAsync(dv, h, bytes, hipMemcpyHostToDevice, sup));
                else HIPCHK(hipMemcpyAsync(h, dv, bytes, hipMemcpyDeviceToHost, sdn));
                return XINV_OK;
            }
            return up ? stage_h2d(ws->ring_up, sup, (double *)dv, (const double *)h, bytes)
                      : stage_d2h(ws->ring_down, sdn, (double *)h, (const double *)dv, bytes);
        };
        char *hs = (char *)host, *dv = (char *)dev;
        if (members == 1 || hstride == len) return one(hs, dv, (size_t)members * len * esz);
        for (int64_t m = 0; m < members; m++)
            if (int r = one(hs + (size_t)m * hstride * esz, dv + (size_t)m * len * esz, (size_t)len * esz)) return r;
        return XINV_OK;
    }
    // members [m0, m0 + members) of a float64 host array, or (tmp != nullptr) a float32 one: uploaded as it is -- half the
    // bytes over PCIe -- into `tmp` and promoted on the device (exact), in stream order
    int h2d(double *dev, const double *host, int64_t m0, int64_t members, int64_t hstride, int64_t len, float *tmp = nullptr)
    {
        const char *h = (const char *)host + (size_t)m0 * hstride * (tmp ? 4 : 8);
        if (!tmp) return copy_pieces(true, h, dev + m0 * len, members, hstride, len, 8);
        if (int r = copy_pieces(true, h, tmp, members, hstride, len, 4)) return r;
        const int64_t cnt = members * len;
        hipLaunchKernelGGL(k_promote_f32, dim3((unsigned)std::min<int64_t>(4096, (cnt + 255) / 256)), dim3(256), 0, sup,
                           (const float *)tmp, dev + m0 * len, cnt);
        return XINV_OK;
    }
    // (scratch for the float32 uploads of array arr -- 0 = S, q + 1 = coefficient q --: one buffer per array, as large as
    //  its largest piece; pieces follow each other in stream order on `sup`, so the buffer is free again when the next lands)
    int f32_tmp(int arr, int64_t elems, float **out)
    {
        double *t = nullptr;
        const int r = ((p.f32 >> arr) & 1u) ? pool_alloc(pool, (size_t)elems * sizeof(float), &t) : XINV_OK;
        *out = (float *)t;
        return r;
    }
    void prep_forcing(double *dF, int64_t nelem)      // front-end passes on the device (xinv_options.prep_flags)
    {
        hipLaunchKernelGGL(k_prep_forcing, dim3((unsigned)std::min<int64_t>(4096, (nelem + 255) / 256)), dim3(256), 0, sup, dF, nelem,
                           p.yc, p.xc, (const double *)d_rowscale, (opt.prep_flags & XINV_PREP_MASK_NAN) ? 1 : 0, opt.prep_undef, p.sc_.undef);
    }
};

// The streams, the device pool, the staging rings and the copy streams' timing events of the call
static int host_begin(HostCall &h)
{
    // The copy streams take the highest stream priority: the runtime keeps its hardware queues per priority, so the staged
    // copies (blit kernels on this runtime) no longer queue behind a chunk solve's launch chain that happens to share
    // their hardware queue -- C4 x 8 with four chunk solves in flight: 14.0 -> 12.8 ms, uploads no longer stretched to
    // 8 ms (profiles/r06_host_pipeline.txt; XINV_COPY_PRIO=0 in a hooks build: the round-5 streams).
    Workspace *ws = h.ws;
    for (hipStream_t *sp : { &ws->s_up, &ws->s_down, &ws->s_compute })
        if (!*sp) {
            if (sp != &ws->s_compute && XINV_ENV_INT("XINV_COPY_PRIO", 1)) {
                int lo_ = 0, hi_ = 0;
                if (hipDeviceGetStreamPriorityRange(&lo_, &hi_) != hipSuccess || hipStreamCreateWithPriority(sp, hipStreamNonBlocking, hi_) != hipSuccess) {
                    (void)hipGetLastError();             // (no priorities on this device / runtime: a plain stream)
                    *sp = nullptr;
                    HIPCHK(hipStreamCreateWithFlags(sp, hipStreamNonBlocking));
                }
            } else
                HIPCHK(hipStreamCreateWithFlags(sp, hipStreamNonBlocking));
        }
    h.sup = ws->s_up; h.sdn = ws->s_down; h.scp = ws->s_compute;
    h.pool = get_pool(h.device);
    h.pool->reset();
    h.pin.streams = { h.sup, h.sdn, h.scp };
    // a previous call that returned on an error may have left slots of the staging rings marked in flight, with
    // `dst` pointing into ITS host array: drain the (normally idle) copy streams and forget them
    HIPCHK(hipStreamSynchronize(h.sup)); HIPCHK(hipStreamSynchronize(h.sdn));
    ws->ring_up.reset(); ws->ring_down.reset();
    int rc;
    if ((rc = h.ev.make(&h.e_up0, true)) || (rc = h.ev.make(&h.e_up1, true)) || (rc = h.ev.make(&h.e_dn0, true)) || (rc = h.ev.make(&h.e_dn1, true))) return rc;
    return XINV_OK;
}

// The staging plan: device buffers now; what travels is queued for the uploader -- the shared arrays first, then S and the
// per-member arrays chunk by chunk, in coefficient order, an event after each chunk
static int host_stage(HostCall &h)
{
    h.d.rowconst = 0; h.d.sS = h.n;
    int rc;
    if ((rc = pool_alloc(h.pool, (size_t)h.p.nbatch * h.n * sizeof(double), &h.d.S))) return rc;
    h.pin.adopt(h.p.S, host_bytes(h.p, 0));
    const int64_t mmax_chunk = *std::max_element(h.chunks.begin(), h.chunks.end());
    if (!(h.opt.prep_flags & XINV_PREP_S_ZERO) && (rc = h.f32_tmp(0, mmax_chunk * h.n, &h.tmpS_up))) return rc;
    if ((rc = h.f32_tmp(0, h.p.nbatch * h.n, &h.tmpS_dn))) return rc;      // (downloads trail the solves: every chunk its own piece)
    for (int q = 0; q < h.p.ncoef; q++) {
        h.per_member[q] = false; h.tmpC[q] = nullptr;
        if (!h.p.c[q]) { h.d.c[q] = nullptr; h.d.sc[q] = 0; continue; }
        const int64_t hst = h.p.nbatch > 1 ? h.p.sc[q] : 0;
        const double *hq = h.p.c[q];
        double *dc;
        if ((h.p.rowconst >> q) & 1u) {                 // one value per row: upload rows, expand on the device
            const int64_t rows = h.p.zc * h.p.yc, xc = h.p.xc, members = (hst == 0) ? 1 : h.p.nbatch;
            double *drow;
            if ((rc = pool_alloc(h.pool, (size_t)members * rows * sizeof(double), &drow)) ||
                (rc = pool_alloc(h.pool, (size_t)members * h.n * sizeof(double), &dc)) ||
                (rc = h.f32_tmp(q + 1, members * rows, &h.tmpC[q]))) return rc;
            h.shared_ops.push_back([=, &h]() -> int {
                if (int r = h.h2d(drow, hq, 0, members, hst, rows, h.tmpC[q])) return r;
                hipLaunchKernelGGL(k_expand_rows, dim3(cdiv(rows * members, 4)), dim3(256), 0, h.sup, (const double *)drow, dc, rows, xc, members);
                return XINV_OK;
            });
            h.d.sc[q] = (hst == 0) ? 0 : h.n;
            h.d.known_um |= 1u << q;                  // (expanded from one value per row: constant along x by construction)
        } else {                                      // shared: travels ahead of the chunks; per member: with its chunk
            const bool pm = hst != 0;
            if ((rc = pool_alloc(h.pool, (size_t)(pm ? h.p.nbatch : 1) * h.n * sizeof(double), &dc))) return rc;
            h.pin.adopt(hq, host_bytes(h.p, q + 1));
            if ((rc = h.f32_tmp(q + 1, (pm ? mmax_chunk : 1) * h.n, &h.tmpC[q]))) return rc;
            if (!pm) h.shared_ops.push_back([=, &h]() -> int { return h.h2d(dc, hq, 0, 1, 0, h.n, h.tmpC[q]); });
            h.d.sc[q] = pm ? h.n : 0;
            h.per_member[q] = pm;
        }
        h.d.c[q] = dc;
    }
    // front-end passes on the device (xinv_options.prep_flags): the forcing is the last array
    h.do_prep = (h.opt.prep_flags & (XINV_PREP_MASK_NAN | XINV_PREP_MASK_VALUE)) != 0;
    if (h.do_prep && (h.opt.prep_flags & XINV_PREP_ROWSCALE)) {
        if (!h.opt.prep_rowscale) return fail_arg("XINV_PREP_ROWSCALE without prep_rowscale");
        if ((rc = pool_alloc(h.pool, (size_t)h.p.yc * sizeof(double), &h.d_rowscale))) return rc;
        h.shared_ops.push_back([&h]() -> int { return h.h2d(h.d_rowscale, h.opt.prep_rowscale, 0, 1, 0, h.p.yc); });
    }
    if (h.do_prep && !h.per_member[h.fq]) {
        double *dF = const_cast<double *>(h.d.c[h.fq]);
        h.shared_ops.push_back([=, &h]() -> int { h.prep_forcing(dF, h.n); return XINV_OK; });      // one shared forcing
    }
    h.e_chunk.assign((size_t)h.nchunk, nullptr);
    h.chunk_ops.resize((size_t)h.nchunk);
    for (int64_t c = 0; c < h.nchunk; c++) {
        const int64_t m0 = h.first[(size_t)c], nm = h.chunks[(size_t)c];
        if ((rc = h.ev.make(&h.e_chunk[(size_t)c], false))) return rc;
        auto &ops = h.chunk_ops[(size_t)c];
        if (h.opt.prep_flags & XINV_PREP_S_ZERO)
            ops.push_back([=, &h]() -> int { HIPCHK(hipMemsetAsync(h.d.S + m0 * h.n, 0, (size_t)nm * h.n * sizeof(double), h.sup)); return XINV_OK; });
        else
            ops.push_back([=, &h]() -> int { return h.h2d(h.d.S, h.p.S, m0, nm, h.hsS, h.n, h.tmpS_up); });
        for (int q = 0; q < h.p.ncoef; q++)
            if (h.per_member[q])
                ops.push_back([=, &h]() -> int {
                    double *dq = const_cast<double *>(h.d.c[q]);
                    if (int r = h.h2d(dq, h.p.c[q], m0, nm, h.p.sc[q], h.n, h.tmpC[q])) return r;
                    if (h.do_prep && q == h.fq) h.prep_forcing(dq + m0 * h.n, nm * h.n);
                    return XINV_OK;
                });
    }
    return XINV_OK;
}

// The uploader thread: the staging plan's ops in order, chunk c's event recorded behind its uploads, then chunk_ready[c]
static void uploader(HostCall &h)
{
    int r = (hipSetDevice(h.device) == hipSuccess) ? XINV_OK : XINV_ERR_HIP;
    auto run = [&](std::vector<std::function<int()>> &ops) {
        for (auto &f : ops) {
            { std::lock_guard<std::mutex> lk(h.act.mu); if (h.act.abort) r = r ? r : XINV_ERR_HIP; }
            if (r) return;
            try { r = f(); } catch (const std::exception &e) { t_err = e.what(); r = XINV_ERR_HIP; }
        }
    };
    if (!r && hipEventRecord(h.e_up0, h.sup) != hipSuccess) r = XINV_ERR_HIP;
    if (!r) run(h.shared_ops);
    h.trace("uploader: shared arrays queued");
    for (int64_t c = 0; c < h.nchunk; c++) {
        if (!r) run(h.chunk_ops[(size_t)c]);
        h.trace("uploader: chunk queued", c);
        if (!r && hipEventRecord(h.e_chunk[(size_t)c], h.sup) != hipSuccess) r = XINV_ERR_HIP;
        if (!r && c == h.nchunk - 1 && hipEventRecord(h.e_up1, h.sup) != hipSuccess) r = XINV_ERR_HIP;
        { std::lock_guard<std::mutex> lk(h.act.mu); h.act.chunk_ready[(size_t)c] = 1; if (r) { h.act.u_rc = r; h.act.u_err = t_err; } }
        h.act.cv.notify_all();
    }
}

// The downloader thread: the download jobs in the order they were handed over, until close_downloads()
static void downloader(HostCall &h)
{
    int r = (hipSetDevice(h.device) == hipSuccess) ? XINV_OK : XINV_ERR_HIP;
    bool first_job = true;
    for (;;) {
        std::function<int()> job;
        {
            std::unique_lock<std::mutex> lk(h.act.mu);
            h.act.cv.wait(lk, [&] { return h.act.d_closed || !h.act.dq.empty(); });
            if (h.act.dq.empty()) break;
            job = std::move(h.act.dq.front()); h.act.dq.pop_front();
            if (h.act.abort) continue;
        }
        if (r) continue;
        if (first_job) { if (hipEventRecord(h.e_dn0, h.sdn) != hipSuccess) r = XINV_ERR_HIP; first_job = false; }
        if (!r) { try { r = job(); } catch (const std::exception &e) { t_err = e.what(); r = XINV_ERR_HIP; } }
        h.trace("downloader: job queued / staged");
    }
    if (!r && first_job && hipEventRecord(h.e_dn0, h.sdn) != hipSuccess) r = XINV_ERR_HIP;
    if (!r && hipEventRecord(h.e_dn1, h.sdn) != hipSuccess) r = XINV_ERR_HIP;
    if (!r && hipStreamSynchronize(h.sdn) != hipSuccess) r = XINV_ERR_HIP;
    h.trace("downloader: drained");
    std::lock_guard<std::mutex> lk(h.act.mu);
    h.act.d_rc = r; if (r) h.act.d_err = t_err;
}

// The chunk solves in flight, their workspaces and compute streams, and what every chunk solve runs with
static int host_slots(HostCall &h)
{
    // Two chunk solves are in flight at a time (round 5): the even chunks on the calling thread (the device's workspace),
    // the odd ones on a helper thread with a workspace and a compute stream of its own.  A chunk fills the 256 CUs less
    // evenly than the whole batch -- the 3-D kernels run ceil(workgroups / 256) rounds, every 2-D launch ends with a
    // tail --; with the next chunk's launches already queued on the device those holes are filled, as the two launch
    // chains of a device-resident batch fill each other's (the lanes of run_sweeps).
    // How many chunk solves are in flight: every one is a chain of dependent launches, and a launch of a two-volume chunk
    // (276 tiles on 256 CUs) ends in a tail during which only the OTHER chains' launches keep the CUs busy.  Two chains
    // (round 5) left the chip 1.68 launches deep on average -- C5 x 15: 160 ms of which the GPU is busy 160, at 107 us per
    // volume and launch against 77 for the resident batch (profiles/r06_host_pipeline.txt) --; three / four fill the tails.
    // 2-D forms: two.  (Four -- possible since the copy streams have queues of their own; before, a third and fourth chain
    // stretched the uploads behind them to 8 ms -- are faster in a fresh process, C4 x 8 14.4 -> 13.3 ms, 3600 x 1800 x 8
    // 47.6 -> 43.6, and bimodal in one that has run resident solves before: bench.py's end_to_end leg 12.3-12.9 or 14.7-16.1
    // ms, process by process, against 12.8-13.1 with two; host_inflight = 4 asks for them.)  What is left against the
    // resident batch (C4 x 8, 2000 sweeps: 37.1 ms against 28.4 + 5 of copies) is kernel time of small launches: four
    // chains of two-member launches run 8.7 us per member and pass, the resident batch's two lanes of four 7.2
    // (tools/kernel_groups.sh; GPU_MAX_HW_QUEUES=8 makes the resident two-lane solve itself 7.6 -> 11.7 ms).
    h.ninfl = (int)std::min<int64_t>(h.nchunk, std::max(1, h.opt.host_inflight > 0 ? std::min(h.opt.host_inflight, XINV_MAX_INFLIGHT)
                                                                                    : (is3d(h.p.kind) ? 3 : XINV_ENV_INT("XINV_INFLIGHT_2D", XINV_DEFAULT_INFLIGHT))));
    h.wss.assign((size_t)h.ninfl, h.ws);
    h.scps.assign((size_t)h.ninfl, h.scp);
    for (int k = 1; k < h.ninfl; k++) {
        Workspace *w = h.wss[(size_t)k] = get_ws(h.device, k);
        if (!w->s_compute) HIPCHK(hipStreamCreateWithFlags(&w->s_compute, hipStreamNonBlocking));
        h.act.streams.push_back(h.scps[(size_t)k] = w->s_compute);
    }
    // the workspaces grow on demand: size them for the LARGEST chunk now, so that a later, larger chunk does not pay a
    // free + malloc of the ping-pong buffer (or of the pinned control-block mirror) mid-pipeline
    const int64_t mmax = *std::max_element(h.chunks.begin(), h.chunks.end());
    int rc;
    if (h.nchunk > 1 && h.p.kind != KIND_BIH2D)
        for (Workspace *w : h.wss) {
            if ((rc = ensure_dev(&w->S2, &w->S2_cap, (size_t)mmax * h.n * sizeof(double)))) return rc;
            if ((rc = ensure_dev(&w->ctl, &w->ctl_cap, (size_t)mmax * sizeof(XinvCtl))) || (rc = ensure_mirror(w, mmax))) return rc;
        }
    h.o1.device = h.device; h.o1.ndev = 0;
    if (is3d(h.p.kind) && h.nchunk > 1 && h.o1.lanes == 0) h.o1.lanes = 1;      // (several chunk solves in flight already: one chain each)
    return XINV_OK;
}

// members [m0, m0 + nm): S is final on the device in stream order of `cs` -- the output passes (de-mask, float32), then
// the hand-over to the downloader.  `after`: an event to record behind them for the downloader to wait on (the rolling
// batch: no host synchronisation of the compute stream); nullptr: synchronise `cs` here.
static int finish_members(HostCall &h, int64_t m0, int64_t nm, hipStream_t cs, hipEvent_t after)
{
    const bool demask = (h.opt.prep_flags & XINV_PREP_DEMASK) != 0;
    for (int64_t m = 0; demask && m < nm; m++) {
        const double *dF = h.d.c[h.fq] + (h.per_member[h.fq] ? (m0 + m) * h.n : 0);
        hipLaunchKernelGGL(k_demask, dim3((unsigned)std::min<int64_t>(4096, (h.n + 255) / 256)), dim3(256), 0, cs,
                           h.d.S + (m0 + m) * h.n, dF, h.n, h.p.sc_.undef, h.opt.demask_value);
    }
    if (h.tmpS_dn)                                   // float32 S: rounded on the device, half the bytes back
        hipLaunchKernelGGL(k_demote_f64, dim3((unsigned)std::min<int64_t>(4096, (nm * h.n + 255) / 256)), dim3(256), 0, cs,
                           (const double *)(h.d.S + m0 * h.n), h.tmpS_dn + m0 * h.n, nm * h.n);
    if (after) HIPCHK(hipEventRecord(after, cs));
    else if (demask || h.tmpS_dn) HIPCHK(hipStreamSynchronize(cs));
    const char *dS = h.tmpS_dn ? (const char *)h.tmpS_dn : (const char *)h.d.S;
    const size_t es = h.tmpS_dn ? 4 : 8;
    {
        std::lock_guard<std::mutex> lk(h.act.mu);
        h.act.dq.push_back([=, &h]() -> int {
            if (after) HIPCHK(hipStreamWaitEvent(h.sdn, after, 0));
            return h.copy_pieces(false, (const char *)h.p.S + (size_t)m0 * h.hsS * es, dS + (size_t)m0 * h.n * es, nm, h.hsS, h.n, es);
        });
    }
    h.act.cv.notify_all();
    return XINV_OK;
}

// one chunk: wait for its upload, solve it on `cs` (workspace `slot`), run the output passes, hand it to the downloader
static int do_chunk(HostCall &h, int64_t c, hipStream_t cs, int slot)
{
    const int64_t m0 = h.first[(size_t)c], nm = h.chunks[(size_t)c];
    int r;
    if ((r = h.wait_chunk(c))) return r;
    HIPCHK(hipStreamWaitEvent(cs, h.e_chunk[(size_t)c], 0));
    h.trace("solver: chunk's upload queued, solve starts", c);
    Problem dc = h.d;
    { std::lock_guard<std::mutex> lk(h.act.mu); dc.known_um |= h.shared_um; }     // (what an earlier chunk's plan found out)
    dc.nbatch = nm; dc.S = h.d.S + m0 * h.n;
    for (int q = 0; q < dc.ncoef; q++)
        if (dc.c[q] && dc.sc[q] != 0) dc.c[q] += m0 * dc.sc[q];
    if ((r = solve_dev(dc, h.flags + 3 * m0, &h.o1, cs, slot))) return r;
    if (h.trace_on()) { char b_[96]; snprintf(b_, sizeof b_, "solver: chunk solved (plan %.3f ms, sweeps %.3f ms)", t_stats.plan_ms, t_stats.sweep_ms); h.trace(b_, c); }
    {
        std::lock_guard<std::mutex> lk(h.act.mu);
        for (int q = 0; q < h.d.ncoef; q++)          // shared arrays found constant along x: the same for every chunk
            if (h.d.c[q] && h.d.sc[q] == 0 && ((t_detected_um >> q) & 1u)) h.shared_um |= 1u << q;
        if (!h.acc_set) { h.acc = t_stats; h.acc_set = true; }
        else merge_sweep_stats(h.acc, t_stats, false);
    }
    // solve_dev has returned: the chunk's S is final on the device
    return finish_members(h, m0, nm, cs, nullptr);
}

// helper solver thread k: chunks k, k + ninfl, .. on workspace slot k
static void chunk_solver(HostCall &h, int k)
{
    int r = (hipSetDevice(h.device) == hipSuccess) ? XINV_OK : XINV_ERR_HIP;
    for (int64_t c = k; c < h.nchunk && !r; c += h.ninfl)
        try { r = do_chunk(h, c, h.scps[(size_t)k], k); } catch (const std::exception &e) { t_err = e.what(); r = XINV_ERR_HIP; }
    if (r) { std::lock_guard<std::mutex> lk(h.act.mu); if (!h.act.s2_rc) { h.act.s2_rc = r; h.act.s2_err = t_err; } }
}

// The chunk scheme: solve chunk by chunk, ninfl chunk solves in flight; downloads trail on their own thread
static int chunk_scheme(HostCall &h)
{
    for (int k = 1; k < h.ninfl; k++) h.act.solvers.emplace_back(chunk_solver, std::ref(h), k);
    for (int64_t c = 0; c < h.nchunk; c += h.ninfl)
        if (int rc = do_chunk(h, c, h.scp, 0)) return rc;      // (HostActors' destructor stops and joins the helpers)
    for (auto &t : h.act.solvers) if (t.joinable()) t.join();
    if (h.act.s2_rc) { t_err = h.act.s2_err; return h.act.s2_rc; }
    return XINV_OK;
}

// ---- the rolling batch (standard 3-D form, shared coefficients) ---------------------------------------------------
// Every chunk solve above is a chain of small launches -- a two-volume launch of k_pipe3d is 276 tiles on 256 CUs -- and
// with two or three chains in flight the chip still ran at 107 us per volume and launch against 77 for the resident
// batch (profiles/r06_host_pipeline.txt).  Here ONE chain of launches sweeps the members [lo, hi) that have arrived and
// still have sweeps to do: a volume joins at the next even launch after its upload event (its S sits in buffer 0, the
// launches ping-pong), runs its L = ceil(sweeps / K) launches -- the device-side stop rule counts its sweeps, whatever
// the launch index -- and retires (FIFO: every member runs the same budget; a member the tolerance stopped earlier
// idles through its remaining launches as a no-op).  Members are independent (reference core.py:129), so what a
// launch covers cannot change any result.  The host stays two launches ahead of the GPU, so that a join is decided
// when the launch is about to run; a retired member's control block travels behind its last launch, its final state
// is put into S as finalise() does (the redo of a pass the stop rule fired in: from that pass's source, intact since),
// and the downloader takes it from there behind an event.
//
// Lanes (2-D forms): the members are cut into two halves at a chunk boundary, each half a rolling chain of its own on
// its own stream, the two chains' launches issued alternately by this thread -- the lanes of a resident solve
// (run_sweeps): one chain's launch boundary is covered by the other's launch.  (Chains issued by DIFFERENT host
// threads -- the chunk scheme -- do not alternate in the runtime's hardware queues: C4 x 8, 2000 sweeps, 37 ms in
// chunks against 28.4 resident + 5 of copies.)  The 3-D form keeps one chain: its launches fill the chip in rounds.
struct Lane { int64_t lo, hi, cj, cend, mend; hipStream_t s; };     // members [lo, hi) in flight, chunks [cj, cend) to join, up to member mend
struct Retired { int64_t a, b; hipEvent_t ctl_done; hipStream_t s; };   // members [a, b) past their last launch on `s`
struct Roll {                                        // what the steps of one rolling batch share
    static constexpr int NQ = 16;
    Plan pl;
    double plan_ms = 0.0, *buf[2];
    int64_t max_sweeps, L, nlaunch = 0, sweeps_max = 0;   // L: launches of a member
    int Kf, klast, nl = 1, pstep, dsteps;            // sweeps of a launch and of a member's last; lanes; pacing
    std::vector<int64_t> join;                       // member m joined at launch join[m]
    std::deque<Retired> fin;
    Lane lanes[2];
    hipEvent_t ev_l[2][NQ], ev_t0, ev_t1;            // each lane's pacing events; the sweeps' span
    XinvCtl *hc;
};

// The rolling batch's plan, workspace, launch budget, pacing and lanes.  *declined: the chunk scheme takes the call.
static int roll_plan(HostCall &h, Roll &R, bool *declined)
{
    int r;
    if ((r = h.wait_chunk(0))) return r;             // the plan needs the shared coefficient arrays: they travel ahead of member 0
    HIPCHK(hipStreamWaitEvent(h.scp, h.e_chunk[0], 0));
    if ((r = ws_ready(h.ws))) return r;
    memset(&t_stats, 0, sizeof t_stats);
    const auto t_plan0 = std::chrono::steady_clock::now();
    xinv_options oroll = h.o1;
    if (h.roll2d) {
        // 2-D: the plan of a batch reads every member's forcing (the lists of fully masked tiles) -- the rolling batch plans
        // before they have arrived.  The first chunk is planned alone: if IT has masked tiles to skip, the chunk scheme
        // takes the call; else the batch is planned without tile lists (a later member's masked tiles are swept like any
        // other: the update leaves masked points alone, the result is the same).  The pipelined pass's table of update
        // masks reads every member's forcing as well: the plan only allocates it, and every chunk's share is built when the
        // chunk joins its lane, behind its upload (roll_join).
        Problem d1 = h.d; d1.nbatch = h.chunks[0];
        Plan pa;
        if ((r = make_plan(d1, h.o1, h.ws, h.scp, pa))) return r;
        // (the point-factor stream of the general form with coefficients that vary along x folds the forcing's mask into the
        //  factors: it reads every member's forcing too)
        if (pa.path != XINV_PATH_FUSED || pa.skip || pa.pq) { *declined = true; return XINV_OK; }
        for (int q = 0; q < h.d.ncoef; q++)          // (what that plan found constant along x is not tested again)
            if (h.d.c[q] && h.d.sc[q] == 0 && ((t_detected_um >> q) & 1u)) h.d.known_um |= 1u << q;
        oroll.flags |= XINV_FLAG_NO_TILE_SKIP;
    }
    {
        Problem dr = h.d;                            // (the flag only for THIS plan: the chunk scheme, if it takes the call after
        dr.masks_by_chunk = h.roll2d;                //  all, plans each chunk whole)
        if ((r = make_plan(dr, oroll, h.ws, h.scp, R.pl))) return r;
    }
    if (R.pl.path != XINV_PATH_FUSED || R.pl.skip || R.pl.pq) {
        if (h.roll2d) { *declined = true; return XINV_OK; }
        t_err = "internal: rolling batch without a streaming kernel";
        return XINV_ERR_HIP;
    }
    R.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan0).count();
    // workspace (run_sweeps' own, without the lagged norm: never in 3-D)
    if ((r = solve_workspace(h.ws, h.scp, h.p.nbatch, true, partial_bytes(h.d, R.pl), false, h.p.nbatch * h.n, false))) return r;
    solve_init(h.ws, h.scp, h.p.nbatch, h.ws->partials_half);
    R.buf[0] = h.d.S; R.buf[1] = h.ws->S2; R.hc = h.ws->hctl;
    R.max_sweeps = h.d.stop.mxLoop + 1; R.Kf = R.pl.K;
    R.L = (R.max_sweeps + R.Kf - 1) / R.Kf; R.klast = (int)(R.max_sweeps - (R.L - 1) * R.Kf);
    R.join.assign((size_t)h.p.nbatch, -1);
    // How far the host runs ahead of the GPU: far enough that a wake-up of the pacing wait (20-50 us) never starves the
    // queue -- ~400 us of launches, two at least (a 3-D launch is 0.1-1 ms, a 2-D one 30-60 us) --, not so far that a
    // member that has just arrived waits long for the next join.
    const double est_launch_us = std::max(20.0, (double)h.p.nbatch * (double)h.n * R.pl.K / (R.pl.pipe ? 6.0e5 : (is3d(h.p.kind) ? 2.5e5 : 3.0e5)) * 0.6);
    const int depth = (int)std::min(12.0, std::max(2.0, 400.0 / est_launch_us));
    R.pstep = (h.roll2d && est_launch_us < 100.0) ? 4 : 1;          // launches per pacing event
    R.dsteps = std::max(1, (depth + R.pstep - 1) / R.pstep);        // pacing events the host runs ahead
    for (int q = 0; q < Roll::NQ; q++) if ((r = h.ev.make(&R.ev_l[0][q], false))) return r;
    if ((r = h.ev.make(&R.ev_t0, true)) || (r = h.ev.make(&R.ev_t1, true))) return r;
    HIPCHK(hipEventRecord(R.ev_t0, h.scp));
    R.nl = (h.roll2d && h.nchunk >= 2 && h.ninfl >= 2) ? 2 : 1;
    const int64_t csplit = R.nl == 2 ? (h.nchunk + 1) / 2 : h.nchunk;
    R.lanes[0] = { 0, 0, 0, csplit, h.first[(size_t)csplit], h.scp };
    R.lanes[1] = { h.first[(size_t)csplit], h.first[(size_t)csplit], csplit, h.nchunk, h.p.nbatch, R.nl == 2 ? h.scps[1] : h.scp };
    if (R.nl == 2) {                                 // the second chain starts behind the plan and k_solve_init
        hipEvent_t e_init;
        if ((r = h.ev.make(&e_init, false))) return r;
        HIPCHK(hipEventRecord(e_init, h.scp));
        HIPCHK(hipStreamWaitEvent(R.lanes[1].s, e_init, 0));
        for (int q = 0; q < Roll::NQ; q++) if ((r = h.ev.make(&R.ev_l[1][q], false))) return r;
    }
    return XINV_OK;
}

// A join point -- launch i even: buffer 0 is its source --: the chunks that have arrived join their lane
static int roll_join(HostCall &h, Roll &R, int64_t i)
{
    int64_t cn[2];
    {
        std::unique_lock<std::mutex> lk(h.act.mu);
        bool idle = true;
        for (int l = 0; l < R.nl; l++) idle = idle && R.lanes[l].hi == R.lanes[l].lo;
        int64_t cw = -1;                             // nobody active: wait for the next arrival (uploads come in batch order)
        if (idle) for (int l = R.nl - 1; l >= 0; l--) if (R.lanes[l].cj < R.lanes[l].cend) cw = R.lanes[l].cj;
        if (int r = h.wait_chunk(lk, cw)) return r;
        for (int l = 0; l < R.nl; l++)               // (chunks cj .. cn-1 of the lane have arrived)
            for (cn[l] = R.lanes[l].cj; cn[l] < R.lanes[l].cend && h.act.chunk_ready[(size_t)cn[l]]; ) cn[l]++;
    }
    for (int l = 0; l < R.nl; l++)
        for (Lane &ln = R.lanes[l]; ln.cj < cn[l]; ln.cj++) {
            HIPCHK(hipStreamWaitEvent(ln.s, h.e_chunk[(size_t)ln.cj], 0));
            if (h.roll2d)                            // (its forcing has arrived: the chunk's share of the update masks)
                if (int r = launch_pipe_masks(h.d, R.pl, h.ws, ln.s, h.first[(size_t)ln.cj],
                                              h.first[(size_t)ln.cj + 1] - h.first[(size_t)ln.cj])) return r;
            for (int64_t m = h.first[(size_t)ln.cj]; m < h.first[(size_t)ln.cj + 1]; m++) R.join[(size_t)m] = i;
            ln.hi = h.first[(size_t)ln.cj + 1];
        }
    return XINV_OK;
}

// Launch i of lane l: the members in flight, those on their last launch retired behind it; then the pacing
static int roll_launch(HostCall &h, Roll &R, int l, int64_t i)
{
    Lane &ln = R.lanes[l];
    const int64_t lo = ln.lo, hi = ln.hi;
    int r;
    if (hi > lo) {
        int64_t f = lo;                              // [lo, f): their last launch (klast sweeps)
        while (f < hi && i - R.join[(size_t)f] == R.L - 1) f++;
        const double *src = R.buf[i & 1]; double *dst = R.buf[(i + 1) & 1];
        if (R.klast == R.Kf) {                       // (a budget that is whole passes: one launch for everybody)
            r = launch_planned(h.d, R.pl, h.ws, ln.s, SweepLaunch{R.Kf, src, dst, lo, hi - lo}); if (r) return r; R.nlaunch++;
        } else {
            if (f > lo) { r = launch_planned(h.d, R.pl, h.ws, ln.s, SweepLaunch{R.klast, src, dst, lo, f - lo}); if (r) return r; R.nlaunch++; }
            if (hi > f) { r = launch_planned(h.d, R.pl, h.ws, ln.s, SweepLaunch{R.Kf, src, dst, f, hi - f}); if (r) return r; R.nlaunch++; }
        }
        if (f > lo) {
            HIPCHK(hipMemcpyAsync(R.hc + lo, h.ws->ctl + lo, (size_t)(f - lo) * sizeof(XinvCtl), hipMemcpyDeviceToHost, ln.s));
            Retired g{lo, f, nullptr, ln.s};
            if ((r = h.ev.make(&g.ctl_done, false))) return r;
            HIPCHK(hipEventRecord(g.ctl_done, ln.s));
            R.fin.push_back(g);
            ln.lo = f;
        }
    }
    // `depth` launches ahead of the GPU, no more.  (An event behind EVERY launch of a 2-D chain -- 30-60 us -- holds the
    //  next launch back by a few microseconds: the pacing events of those chains sit behind every fourth launch.)
    if (i % R.pstep == 0) {
        const int64_t e = i / R.pstep;
        HIPCHK(hipEventRecord(R.ev_l[l][e % Roll::NQ], ln.s));
        if (e >= R.dsteps) HIPCHK(hipEventSynchronize(R.ev_l[l][(e - R.dsteps) % Roll::NQ]));
    }
    return XINV_OK;
}

// A retired group whose control blocks have arrived: final state into S, flags, output passes, download
static int roll_finish(HostCall &h, Roll &R, const Retired &g)
{
    int r;
    for (int64_t m = g.a; m < g.b; m++) {
        const XinvCtl &c = R.hc[m];
        if (!c.done) { t_err = "internal: rolling batch: a member retired before its stop rule fired"; return XINV_ERR_HIP; }
        if (c.overflow == 2) { t_err = "internal: norm partials of a sweep launch never arrived (watchdog) in the rolling batch"; return XINV_ERR_HIP; }
        // (the member's launch rl that holds sweep sw ping-pongs from the buffer of its join's parity)
        const int64_t sw = c.sweeps, rl = (sw - 1) / R.Kf;
        const int src = xinv_pingpong_src(R.join[(size_t)m], rl);
        const XinvFinal w = xinv_final_in(rl * R.Kf, std::min<int64_t>((rl + 1) * R.Kf, R.max_sweeps), src, src ^ 1, 2, false, sw);
        for (int64_t q = 0; q < w.redo; q++) {       // stopped inside a pass: redo from its source, sweep by sweep
            SweepLaunch one{1, R.buf[xinv_redo_read(w.r, q)], R.buf[xinv_redo_write(w.r, q)], m, 1};
            one.force = one.no_ctl = 1;
            if ((r = launch_planned(h.d, R.pl, h.ws, g.s, one))) return r;
        }
        if (w.where != 0)
            HIPCHK(hipMemcpyAsync(h.d.S + m * h.n, h.ws->S2 + m * h.n, (size_t)h.n * sizeof(double), hipMemcpyDeviceToDevice, g.s));
        member_flags(c, h.flags + 3 * m);
        R.sweeps_max = std::max<int64_t>(R.sweeps_max, sw);
    }
    hipEvent_t after;
    if ((r = h.ev.make(&after, false))) return r;
    return finish_members(h, g.a, g.b - g.a, g.s, after);
}

// The rolling batch.  *declined: not taken, the chunk scheme takes the call
static int roll(HostCall &h, bool *declined)
{
    Roll R;
    *declined = false;
    int r;
    if ((r = roll_plan(h, R, declined)) || *declined) return r;
    auto active = [&]() { for (int l = 0; l < R.nl; l++) if (R.lanes[l].lo < R.lanes[l].mend) return true; return false; };
    for (int64_t i = 0; active(); i++) {
        if (!(i & 1) && (r = roll_join(h, R, i))) return r;
        for (int l = 0; l < R.nl; l++) if ((r = roll_launch(h, R, l, i))) return r;
        // (the retired groups of two chains do not finish in queue order: take whichever has arrived)
        for (size_t q = 0; q < R.fin.size(); ) {
            if (hipEventQuery(R.fin[q].ctl_done) == hipSuccess) {
                if ((r = roll_finish(h, R, R.fin[q]))) return r;
                R.fin.erase(R.fin.begin() + (std::ptrdiff_t)q);
            } else q++;
        }
        (void)hipGetLastError();                     // (hipEventQuery: hipErrorNotReady is not an error)
    }
    for (; !R.fin.empty(); R.fin.pop_front()) {
        HIPCHK(hipEventSynchronize(R.fin.front().ctl_done));
        if ((r = roll_finish(h, R, R.fin.front()))) return r;
    }
    if (R.nl == 2) HIPCHK(hipStreamSynchronize(R.lanes[1].s));
    HIPCHK(hipEventRecord(R.ev_t1, h.scp));
    HIPCHK(hipStreamSynchronize(h.scp));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, R.ev_t0, R.ev_t1));
    plan_stats(h.d, R.pl, R.nl, 0);                  // (a launch covers the members in flight: no count of cut tiles)
    t_stats.sweep_launches = R.nlaunch; t_stats.sweeps_max = R.sweeps_max; t_stats.sweep_ms = ms; t_stats.plan_ms = R.plan_ms; t_stats.rolling = 1;
    h.acc = t_stats; h.acc_set = true;
    return XINV_OK;
}

static int solve_host_one(Problem &p, double *flags, const xinv_options &opt, const Pinned *outer)
{
    const auto wall0 = std::chrono::steady_clock::now();
    DeviceGuard dg;
    HIPCHK(dg.select(opt.device));
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    // the staging rings, the device pool and the solver workspace are per device: hold the device for the whole
    // upload -> solve -> download sequence
    Workspace *ws = get_ws(device);
    std::lock_guard<std::recursive_mutex> host_lock(ws->busy);
    HostCall h(p, flags, opt, outer, device, ws, wall0);      // (the road -- rolling batch or chunk scheme -- and the chunks)
    int rc;
    if ((rc = host_begin(h)) || (rc = host_stage(h))) return rc;
    h.trace("set up: device buffers, ops queued for the uploader");
    h.act.streams = { h.sup, h.sdn, h.scp };
    h.act.chunk_ready.assign((size_t)h.nchunk, 0);
    h.act.up = std::thread(uploader, std::ref(h));
    h.act.down = std::thread(downloader, std::ref(h));
    if ((rc = host_slots(h))) return rc;
    bool declined = true;                            // (the chunk scheme, unless the rolling batch takes the call)
    if (h.rolling && (rc = roll(h, &declined))) return rc;
    if (declined && (rc = chunk_scheme(h))) return rc;
    h.trace("solves done");
    // join the uploader and downloader, their verdicts, the call's stats
    h.act.close_downloads();
    h.act.up.join(); h.act.down.join();
    h.trace("uploader and downloader joined");
    if (h.act.u_rc) { t_err = h.act.u_err; return h.act.u_rc; }
    if (h.act.d_rc) { t_err = h.act.d_err; return h.act.d_rc; }
    HIPCHK(hipStreamSynchronize(h.sup));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, h.e_up0, h.e_up1));
    HIPCHK(hipEventElapsedTime(&b, h.e_dn0, h.e_dn1));
    t_stats = h.acc;
    t_stats.h2d_ms = a; t_stats.d2h_ms = b; t_stats.host_chunks = (int32_t)h.nchunk; t_stats.devices = 1;
    t_stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return XINV_OK;
}

// Host-pointer entry: one device, or the batch axis split in contiguous blocks over a device list
// (the reference loops slices in ONE process, core.py:129-139; so does this --
// one host thread per GPU, no collective, S and flags land in the caller's arrays).
static int solve_host(Problem &p, double *flags, const xinv_options *opt_in)
{
    xinv_options opt;
    fill_options(opt, opt_in);
    p.rowconst = (unsigned)opt.rowconst_mask & ((1u << p.ncoef) - 1u);
    p.f32 = (unsigned)opt.f32_mask & ((2u << p.ncoef) - 1u);
    int rc = validate(p, flags);
    if (rc) return rc;
    int nvis = 0;
    if (hipGetDeviceCount(&nvis) != hipSuccess || nvis < 1) {
        (void)hipGetLastError();
        t_err = "no HIP device available";
        return XINV_ERR_NODEV;
    }
    std::vector<int> devs;
    if (opt.ndev < 0) {                                // every visible GPU
        for (int i = 0; i < nvis; i++) devs.push_back(i);
    } else if (opt.ndev > 0) {
        if (opt.ndev > XINV_MAX_DEVICES) return fail_arg("ndev exceeds XINV_MAX_DEVICES");
        for (int i = 0; i < opt.ndev; i++) {
            if (opt.device_ids[i] < 0 || opt.device_ids[i] >= nvis) return fail_arg("device_ids: no such device");
            devs.push_back(opt.device_ids[i]);
        }
    }
    if ((int64_t)devs.size() > p.nbatch) devs.resize((size_t)p.nbatch);
    g_copy_pool.start();                               // (here: before a per-device thread below is bound to a NUMA node)
    if (devs.size() <= 1) {
        if (devs.size() == 1) opt.device = devs[0];
        return solve_host_one(p, flags, opt, nullptr);
    }

    const auto wall0 = std::chrono::steady_clock::now();
    const int nd = (int)devs.size();
    // host ranges pinned ONCE for every device (portable registration); the per-device threads
    // then copy straight out of / into the caller's arrays
    Pinned pin;                                        // (opt-in: the per-device calls stage through their own rings otherwise)
    pin.enabled = Pinned::env_allowed() || (opt.flags & XINV_FLAG_PIN_HOST);
    pin.flags = hipHostRegisterPortable;
    auto esz = [&](int arr) { return ((p.f32 >> arr) & 1u) ? (size_t)4 : (size_t)8; };
    pin.adopt(p.S, host_bytes(p, 0));
    for (int q = 0; q < p.ncoef; q++)
        if (p.c[q]) pin.adopt(p.c[q], host_bytes(p, q + 1));
    struct Result { int rc = 0; std::string err; xinv_stats st; };
    std::vector<Result> res((size_t)nd);
    std::vector<std::thread> th;
    const int64_t q0 = p.nbatch / nd, r0 = p.nbatch % nd;
    for (int i = 0; i < nd; i++) {
        const int64_t lo = i * q0 + std::min<int64_t>(i, r0), hi = lo + q0 + (i < r0 ? 1 : 0);
        th.emplace_back([&, i, lo, hi]() {
            Problem sub = p;
            sub.nbatch = hi - lo;
            sub.S = (double *)((char *)p.S + (size_t)lo * p.sS * esz(0));          // (strides count elements of the array's type)
            for (int q = 0; q < p.ncoef; q++)
                if (p.c[q]) sub.c[q] = (const double *)((const char *)p.c[q] + (size_t)lo * p.sc[q] * esz(q + 1));
            xinv_options o1 = opt;
            o1.device = devs[(size_t)i]; o1.ndev = 0;
            // (this thread only lives for the call: nothing to undo; the copy pool's workers, started above, do not inherit it)
            (void)bind_thread_to_device_node(o1.device);
            int r;
            try { r = solve_host_one(sub, flags + 3 * lo, o1, &pin); }
            catch (const std::exception &e) { t_err = e.what(); r = XINV_ERR_HIP; }
            catch (...) { t_err = "unknown C++ exception"; r = XINV_ERR_HIP; }
            res[(size_t)i].rc = r; res[(size_t)i].err = t_err; res[(size_t)i].st = t_stats;
        });
    }
    for (auto &t : th) t.join();
    t_stats = res[0].st;
    for (int i = 0; i < nd; i++) {
        if (res[(size_t)i].rc) { t_err = res[(size_t)i].err; return res[(size_t)i].rc; }
        if (i == 0) continue;
        const xinv_stats &s = res[(size_t)i].st;
        merge_sweep_stats(t_stats, s, true);
        t_stats.h2d_ms = std::max(t_stats.h2d_ms, s.h2d_ms);
        t_stats.d2h_ms = std::max(t_stats.d2h_ms, s.d2h_ms);
        t_stats.host_chunks += s.host_chunks;
    }
    t_stats.devices = nd;
    t_stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return XINV_OK;
}

