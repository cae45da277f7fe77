// xinv_launch.h -- how a solve is laid out on the GPU: the plan (path, colours, tiling, x-uniform
// streams, masked-tile skipping, the kernel of every pass length), the one launch and occupancy query of the sweep
// kernels (xinv_dispatch.h), the colour-pass launches and the once-per-solve detection passes.  Included by xinv_hip.hip only.
#pragma once

// ------------------------------------------------------------------ launch helpers
static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

#if XINV_TEST_HOOKS
static thread_local int *t_hook_record = nullptr;    // device int[3] {tile, launch tag, member}, or nullptr
#endif

struct Plan {
    int path, base, seam, ncol;
    int K, RY, nsg, nrb;     // nsg: 2-D = workgroups per member (partials sizing); 3-D = x strips
    int nkc, KC;             // 3-D: k chunks and planes per chunk
    bool K2;                 // 3-D standard form: passes of two sweeps (k_pipe3d) with the tiling below
    int nsg2, nrb2, nkc2, KC2;
    int joff2;               // k_pipe3d: rows its row blocks are shifted up by ('extend': p3_extend_joff; 0 elsewhere)
    int cus;                 // compute units the planner fills (xinv_options.cu_count, or the device's)
    int64_t srowf2;          // k_pipe3d: member stride of the record table (0: shared by the batch)
    bool bih_zbe;            // biharmonic one-pass kernel: B and E identically zero (terms left out)
    int bih_vm;              // ... where its coefficients come from: 0 per-row records (A..I constant along x), 1 A C D F
                             // as vector streams + the point-factor stream, 2 all nine, 3 as 1 with A == C and D == F
                             // everywhere (two streams less) (xinv_fusedbih.h); Q in ws->d_pfac
    bool aligned;
    unsigned umask;          // fused streams whose rows are constant along x (bit = stream index)
    unsigned um;             // the kernel variant's mask (subset of umask)
    bool even_split;         // rows split evenly over nrb row blocks (RY = average height)
    bool nine;               // 9-point form on the fused 4-colour kernel
    bool skip;               // masked-tile skipping: launches of K == Plan::K run the listed tiles only
    SkipNormArgs skipna;     // (the skipped tiles' geometry and list: k_skip_tiles in run_sweeps)
    int ntl, nskip;          // list entries per member (active, multiple of 4 / skipped)
    size_t trec_off;         // `pipe`: byte offset of k_pipe2d's tile records in ws->d_list (behind the lists, 32-byte aligned)
    int trec_ms;             // ... and their member stride in records (0: one set for every member -- no tile is skipped)
    int skip_pct;            // share of wave-tiles skipped, percent
    int skip_ppm;            // ... per million
    double lone = 1.6;       // planner: cost of a workgroup alone on its CU relative to one of a pair
    bool pipe;               // K == 4 passes run the wave-pipelined kernel (k_pipe2d): one tile per workgroup
    int tpw;                 // wave-tiles per workgroup of the planned kernel: 4, or 1 with `pipe`
    bool pipe_fr;            // `pipe`: the forcing rides the LDS ring (xinv_tiles.h: xinv_pipe_forcing_ring)
    int64_t xc;              // the problem's row length (the ring layout's strip width depends on it: xinv_tiles.h)
    bool fma;                // XINV_FLAG_FMA: the contracted-arithmetic kernel variants (per-row-coefficient forms only)
    bool alias_ac;           // `pq`: A and C hold the same numbers everywhere -- C is read out of A (FusedGen2DQA, kernel mask um | 2)
    bool pq;                 // general form with A, C varying along x: the point-factor stream Q (FusedGen2DQ: relaxation
                             // factor and update predicate of every point, evaluated once per coefficient stack);
                             // Q lives in ws->d_pfac (a plan's own buffer while it solves)
    KernelRef kern[XINV_KMAX + 1];   // the kernel of a pass of k sweeps, k = 1 .. K: the full pass, the shorter tail, the
                             // one-sweep redo and recovery (plan_kernels; resident plans copy them: process-lifetime addresses)
};

// kernel variants instantiated per model: mask of streams read as one scalar per row
static unsigned pick_um(int kind, unsigned umask)
{
    if (kind == KIND_STD2D) return ((umask & 3u) == 3u) ? 3u : 0u;            // A, C
    if (kind == KIND_STD2DT) return ((umask & 7u) == 7u) ? 7u : 0u;           // A, D, E
    if ((umask & 0x1fu) == 0x1fu) return 0x1fu;                                // A, C, D, E, F
    if ((umask & 0x1cu) == 0x1cu) return 0x1cu;                                // D, E, F
    return 0u;
}

// The streams of the 2-D 5-point kernels: stream q of FusedArgs (and bit q of umask / um above) reads Problem::c[c[q]].
// Standard form A C F, test form A D E F, general form A C D E F G (B is identically zero on these kernels).
struct StreamMap {
    int n, c[6];             // kernel streams; the coefficient each one reads
    int forcing;             // the stream that is the forcing: the last of every form
    int nuni;                // leading streams the x-uniform detection looks at (the forcing is not: no variant reads it per row)
};
static const StreamMap &stream_map(int kind)
{
    static const StreamMap std2d = {3, {0, 2, 3}, 2, 2}, std2dt = {4, {0, 3, 4, 5}, 3, 3}, gen2d = {6, {0, 2, 3, 4, 5, 6}, 5, 5};
    return kind == KIND_STD2D ? std2d : (kind == KIND_STD2DT ? std2dt : gen2d);
}

// Columns a tile of this plan owns at K sweeps per pass (`pipe`: of the wave-pipelined pass, which has K = XINV_PIPE_P).
// 5-point kernels: 128 minus the 2K halo columns a side; 9-point kernel: one halo column per colour and sweep; the
// odd-xc periodic seam variants own one pair less (the ring layout's strips, xinv_tiles.h); biharmonic kernel: fixed.
static inline int own_cols(const Problem &p, const Plan &pl, int K, bool pipe = false)
{
    if (p.kind == KIND_BIH2D) return XINV_BIH_OWN(p.BCx == XINV_BC_PERIODIC);
    if (pl.nine) return pl.seam ? xinv_ring_uw(pl.xc, 4 * K) : 128 - 8 * K;
    if (pl.seam) return xinv_ring_uw(pl.xc, pipe ? 2 * XINV_PIPE_P : 2 * K);
    return pipe ? XINV_PIPE_UW : 128 - 4 * K;
}

// k_row_factor's record of the two pipelined forms (xinv_pipe2d.h: PipeRec): doubles per record, the row predicate's word
struct PipeRecShape { int rw, irok; };
static inline PipeRecShape pipe_rec_shape(int kind)
{
    using G = PipeRec<FusedGen2D, 0x1fu>;
    using S = PipeRec<FusedStd2D, 3u>;
    return kind == KIND_GEN2D ? PipeRecShape{G::RW, G::NW - 1} : PipeRecShape{S::RW, S::NW - 1};
}

// k_pipe3d's launch shape (which tiles of a launch march the whole column, which are cut into the plan's k chunks) and the
// 'extend' variant's tiling offset: xinv_tiles.h (xinv_p3_whole_tiles, xinv_p3_extend_joff; checked on the CPU).
static int p3_extend_joff(int64_t yc)
{
    static_assert(XINV_P3_RR == 3 && XINV_P3_G * XINV_P3_RR - 8 > 0, "k_pipe3d: three rows per wavefront");
    return xinv_p3_extend_joff(yc, XINV_P3_G * XINV_P3_RR - 8, 4, XINV_P3_RR);
}

// ------------------------------------------------------------------ the sweep kernels: variant -> kernel, launch, occupancy
// The unit that holds a variant (xinv_dispatch.h); fn == nullptr where none does.
static KernelRef xinv_kernel(const SweepVariant &v)
{
    const bool gen = v.kind == KIND_GEN2D, test = v.kind == KIND_STD2DT;
    switch (v.family) {
    case FAM_FUSED2D:
        if (v.pq) return (!gen || v.seam || v.fma) ? KernelRef{} : xinv_kernel_fused2d<FUSED2D_GENQ, false>(v);
        if (v.fma) {                                     // contracted arithmetic (xinv_fused.h: FusedStd2DF / FusedGen2DF)
            if (v.seam || test) return KernelRef{};
            return gen ? xinv_kernel_fused2d<FUSED2D_GENF, false>(v) : xinv_kernel_fused2d<FUSED2D_STDF, false>(v);
        }
        if (v.seam)                                      // odd-xc periodic seam variants (xinv_fused.h: SEAM)
            return gen ? xinv_kernel_fused2d<FUSED2D_GEN, true>(v)
                       : (test ? xinv_kernel_fused2d<FUSED2D_STD2DT, true>(v) : xinv_kernel_fused2d<FUSED2D_STD, true>(v));
        return gen ? xinv_kernel_fused2d<FUSED2D_GEN, false>(v)
                   : (test ? xinv_kernel_fused2d<FUSED2D_STD2DT, false>(v) : xinv_kernel_fused2d<FUSED2D_STD, false>(v));
    case FAM_PIPE2D:
        if (v.fma) return v.seam ? KernelRef{} : xinv_kernel_pipe2d<PIPE2D_FMA, false>(v);
        if (v.seam) return gen ? xinv_kernel_pipe2d<PIPE2D_GEN, true>(v) : xinv_kernel_pipe2d<PIPE2D_STD, true>(v);
        return gen ? xinv_kernel_pipe2d<PIPE2D_GEN, false>(v) : xinv_kernel_pipe2d<PIPE2D_STD, false>(v);
    case FAM_FUSED9: return xinv_kernel_fused9(v);
    case FAM_FUSED3D: return v.seam ? xinv_kernel_fused3d_seam(v) : (v.fma ? xinv_kernel_fused3d_fma(v) : xinv_kernel_fused3d(v));
    case FAM_FUSED3DG: return v.seam ? xinv_kernel_fused3d_seam(v) : xinv_kernel_fused3d(v);
    case FAM_PIPE3D: return xinv_kernel_pipe3d(v);
    case FAM_BIH: return xinv_kernel_bih(v);
    }
    return KernelRef{};
}

// `args`: the kernel's one argument struct (FusedArgs, Fused3Args, Fused3GArgs, FusedBihArgs -- what its family takes)
template <class A>
static inline void kernel_launch(KernelRef k, dim3 grid, size_t lds, hipStream_t st, const A &args)
{
    void *argv[1] = {const_cast<A *>(&args)};
    (void)hipLaunchKernel(k.fn, grid, dim3(k.threads, 1, 1), argv, lds, st);     // (errors: the caller's hipGetLastError)
}

// Workgroups of a kernel that fit on a CU (register-limited), 1 where the runtime cannot say.  Asked of the runtime once
// per kernel and process (the planner asks in every solve: a few microseconds per query); several planner threads may ask.
static int kernel_occupancy(KernelRef k)
{
    static std::mutex mu;
    static std::unordered_map<const void *, int> known;
    std::lock_guard<std::mutex> lock(mu);
    int &n = known[k.fn];
    if (!n && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, (int)k.threads, 0) != hipSuccess || n < 1)) n = 1;
    return n;
}

// One sweep launch of a plan: k sweeps from src into dst (fused path; the colour path sweeps p.S in place) for members
// [member0, member0 + nmem).  force: also members that have stopped; no_ctl: no norm, no stop rule.
// Lagged norm (run_sweeps): the launch publishes with `lag_tag` into the partial buffer of its parity; its extra
// workgroup evaluates `lag_prev`; `lag_out` receives what the evaluation of THIS launch needs.
// prepass = false (biharmonic form, 'extend'): the source already carries this pass's pre-pass (launch_fusedbih).
struct SweepLaunch {
    int k;
    const double *src;
    double *dst;
    int64_t member0, nmem;
    int force = 0, no_ctl = 0;
    unsigned lag_tag = 0;
    NormLagArgs *lag_out = nullptr;
    const NormLagArgs *lag_prev = nullptr;
    bool prepass = true;
};

// The instantiation a pass of k sweeps of this plan runs: the wave-pipelined kernels for the full pass of a pipelined
// plan (2-D: k == pl.K; standard 3-D form: k == 2), the one-tile-per-wavefront kernels for every shorter one.
static SweepVariant plan_variant(const Problem &p, const Plan &pl, int k)
{
    SweepVariant v;
    memset(&v, 0, sizeof v);
    v.kind = p.kind; v.K = k;
    v.al = pl.aligned; v.ext = (p.BCy == XINV_BC_EXTEND); v.seam = pl.seam != 0; v.fma = pl.fma;
    if (p.kind == KIND_BIH2D) {
        v.family = FAM_BIH; v.per = (p.BCx == XINV_BC_PERIODIC); v.zbe = pl.bih_zbe; v.vm = pl.bih_vm;
    } else if (is3d(p.kind)) {
        v.family = p.kind == KIND_GEN3D ? FAM_FUSED3DG : (k == 2 ? FAM_PIPE3D : FAM_FUSED3D);
        v.NW = pl.RY; v.uni = (pl.um == 7u);
    } else if (pl.nine) {
        v.family = FAM_FUSED9;
    } else if (pl.pipe && k == pl.K) {
        v.family = FAM_PIPE2D; v.um = pl.um; v.pipe_fr = pl.pipe_fr;
    } else {
        v.family = FAM_FUSED2D; v.um = pl.um | (pl.alias_ac ? 2u : 0u); v.pq = pl.pq;      // (um | 2: the A == C variant)
    }
    return v;
}

static bool ptr_al16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }
// an array a kernel may read as vectors of two doubles: 16-byte aligned, members an even number of elements apart
static bool vec_aligned(const double *a, int64_t stride) { return ptr_al16(a) && !(stride & 1); }

// Members [member0, member0 + nmem) in launches of at most `chunk` members (grid.y and grid.z are limited to 65535):
// launch(first member, count) issues one; the first error ends the walk.
template <class F>
static int for_member_chunks(int64_t member0, int64_t nmem, F launch, int64_t chunk = XINV_MEMBER_CHUNK)
{
    for (int64_t m0 = 0; m0 < nmem; m0 += chunk) {
        const int rc = launch(member0 + m0, std::min<int64_t>(chunk, nmem - m0));
        if (rc) return rc;
    }
    return XINV_OK;
}

// BCy = 'extend': the pre-pass of a sweep (numbas.py:87-115) on S of members [member0, member0 + nm), nm <= 65535 --
// every interior plane of a volume; the biharmonic form has its own.  A no-op for a member that has stopped, unless `force`.
static void launch_extend(const Problem &p, const Workspace *ws, hipStream_t st, double *S, int force, int64_t member0, int64_t nm)
{
    ExtendArgs e;
    e.S = S; e.sS = p.sS; e.yc = p.yc; e.xc = p.xc;
    e.kfirst = is3d(p.kind) ? 1 : 0;
    e.nk = is3d(p.kind) ? p.zc - 2 : 1;
    // the standard 3-D kernel's second loop stays inside the row (numbas.py:104-108)
    e.per = (p.BCx == XINV_BC_PERIODIC); e.tall = (p.kind != KIND_STD3D) && (p.yc > p.xc); e.force = force;
    e.undef = p.sc_.undef; e.ctl = ws->ctl; e.member0 = member0;
    dim3 g(cdiv(p.xc, 256), (unsigned)e.nk, (unsigned)nm), b(256, 1, 1);
    if (p.kind == KIND_BIH2D) hipLaunchKernelGGL(k_extend_bih, g, b, 0, st, e);
    else                      hipLaunchKernelGGL(k_extend, g, b, 0, st, e);
}

// The buffer behind masked-tile skipping (ws->d_tsum) with `nskip` list slots per member: the skipped tiles' shares of the
// norm tsum / tcnt [nbatch][nskip], their sums per member xsum / xcnt [nbatch], k_skip_tiles' tickets [nbatch]; `bytes` in all.
struct TsumPtrs { double *tsum; long long *tcnt; double *xsum; long long *xcnt; unsigned *ticket; size_t bytes; };
static TsumPtrs tsum_layout(void *buf, int64_t nbatch, int nskip)
{
    const size_t nb = (size_t)nbatch, nt = nb * (size_t)nskip, pair = sizeof(double) + sizeof(long long);
    const uintptr_t base = (uintptr_t)buf;
    TsumPtrs t;
    t.tsum = (double *)base;
    t.tcnt = (long long *)(base + nt * sizeof(double));
    t.xsum = (double *)(base + nt * pair);
    t.xcnt = (long long *)(base + nt * pair + nb * sizeof(double));
    t.ticket = (unsigned *)(base + (nt + nb) * pair);
    t.bytes = (nt + nb) * pair + nb * sizeof(unsigned);
    return t;
}

// Fully masked tiles are left out (plan_tile_skip): the launch runs the listed tiles, `tpw` per workgroup, and takes the
// skipped tiles' constant share of the norm from xsum / xcnt.  `a` is a FusedArgs / FusedBihArgs.
template <class A>
static void set_skip(A &a, const Workspace *ws, const Problem &p, const Plan &pl, int tpw)
{
    a.tile_list = ws->d_list;
    a.ntl = pl.ntl;
    a.nwg = pl.ntl / tpw;
    const TsumPtrs t = tsum_layout(ws->d_tsum, p.nbatch, pl.nskip);
    a.xsum = t.xsum; a.xcnt = t.xcnt;
}

// The lagged norm of launch L (SweepLaunch): `a` is a FusedArgs / FusedBihArgs whose psum / xsum / xcnt / nwg are
// already final, K the sweeps of the pass.
template <class A>
static void set_lag(A &a, const Workspace *ws, const Problem &p, int K, const SweepLaunch &L)
{
    if (L.lag_tag) {
        a.lag = 1; a.tag = L.lag_tag;
        a.psum = (unsigned long long *)((char *)ws->partials + (size_t)((L.lag_tag - 1u) & 1u) * ws->partials_half);
        if (L.lag_prev && L.lag_prev->tag) {
            a.lagp_psum = L.lag_prev->psum; a.lagp_xsum = L.lag_prev->xsum; a.lagp_xcnt = L.lag_prev->xcnt;
            a.lagp_NB = L.lag_prev->NB; a.lagp_K = L.lag_prev->K; a.lagp_tag = L.lag_prev->tag;
        }
    }
    if (L.lag_out) {
        memset(L.lag_out, 0, sizeof *L.lag_out);
        L.lag_out->psum = a.psum; L.lag_out->ctl = ws->ctl; L.lag_out->stop = p.stop;
        L.lag_out->xsum = a.xsum; L.lag_out->xcnt = a.xcnt; L.lag_out->NB = a.nwg; L.lag_out->K = K; L.lag_out->tag = L.lag_tag;
    }
}

// What the 5-point and the 9-point launch fill alike: everything of FusedArgs but the coefficient streams, for strips of
// UW owned columns and four wave-tiles per workgroup.
static void fused_args(FusedArgs &a, const Problem &p, const Plan &pl, const Workspace *ws, const SweepLaunch &L, int UW)
{
    memset(&a, 0, sizeof a);
    a.src = L.src; a.dst = L.dst; a.sS = p.sS;
    a.yc = p.yc; a.xc = p.xc;
    a.per = (p.BCx == XINV_BC_PERIODIC);
    a.ext = (p.BCy == XINV_BC_EXTEND);
    a.tall = (p.yc > p.xc);
    a.RY = pl.even_split ? 0 : pl.RY;
    a.nstrip = (int)cdiv(p.xc, UW);
    a.nrb = pl.even_split ? pl.nrb : (int)cdiv(p.yc, pl.RY);
    a.nwg = (int)cdiv((int64_t)a.nstrip * a.nrb, 4);
    a.force = L.force; a.no_ctl = L.no_ctl;
    a.sc_ = p.sc_; a.ctl = ws->ctl; a.stop = p.stop;
    a.psum = (unsigned long long *)ws->partials;
}

static int launch_fused(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st, const SweepLaunch &L)
{
    FusedArgs a;
    const int K = L.k;
    const bool pipe = pl.pipe && K == pl.K;          // wave-pipelined pass: one tile per workgroup
    fused_args(a, p, pl, ws, L, own_cols(p, pl, K, pipe));
    const StreamMap &sm = stream_map(p.kind);
    for (int q = 0; q < sm.n; q++) { a.c[q] = p.c[sm.c[q]]; a.sc[q] = p.sc[sm.c[q]]; }
    if (pl.pq) {                                     // A, C, D, E, F, Q, G (FusedGen2DQ): Q in front of the forcing
        a.c[sm.forcing + 1] = a.c[sm.forcing]; a.sc[sm.forcing + 1] = a.sc[sm.forcing];
        a.c[sm.forcing] = (const double *)ws->d_pfac; a.sc[sm.forcing] = p.yc * p.xc;
    }
    if (pipe) {
        a.nwg = a.nstrip * a.nrb; a.rowf = ws->d_rowf; a.pmask = ws->d_pmask;
        a.trec = (const char *)ws->d_list + pl.trec_off; a.trec_ms = pl.trec_ms;    // (plan_tile_skip / plan_pipe_tile_recs)
    }
#if XINV_TEST_HOOKS
    a.dbg = (double *)t_hook_record;                 // (run_sweeps: XINV_HOOK_SKIP_PUBLISH; nullptr otherwise)
#endif
    if (pl.skip && K == pl.K) set_skip(a, ws, p, pl, pl.tpw);       // the lists were built for this K's strips
    set_lag(a, ws, p, K, L);
    for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) {
        a.member0 = m;
        dim3 grid((unsigned)a.nwg + (L.lag_tag ? 1u : 0u), (unsigned)nm, 1);
        // (XINV_PIPE_LDSPAD: unused dynamic LDS per workgroup of the pipelined pass, to cap the workgroups per CU in
        //  experiments; capping at the planned count changed nothing: the dispatcher already spreads them evenly)
        kernel_launch(pl.kern[K], grid, pipe ? (size_t)std::max(0, XINV_ENV_INT("XINV_PIPE_LDSPAD", 0)) : 0, st, a);
        return XINV_OK;
    });
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

// The update masks of the pipelined pass for members [member0, member0 + nmem): k_row_factor's records are complete on `st`
// and those members' forcing is in place.  make_plan builds the whole batch's; the rolling host batch, whose members'
// forcing arrives chunk by chunk, builds each chunk's when it joins (Problem::masks_by_chunk, roll_join).
static int launch_pipe_masks(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st, int64_t member0, int64_t nmem)
{
    if (!pl.pipe) return XINV_OK;
    const StreamMap &sm = stream_map(p.kind);
    PipeMaskArgs ma;
    memset(&ma, 0, sizeof ma);
    ma.f = p.c[sm.c[sm.forcing]]; ma.sf = p.sc[sm.c[sm.forcing]];
    ma.rowf = (const double *)ws->d_rowf; ma.rw = pipe_rec_shape(p.kind).rw; ma.irok = pipe_rec_shape(p.kind).irok;
    ma.yc = p.yc; ma.xc = p.xc;
    ma.per = (p.BCx == XINV_BC_PERIODIC); ma.al = pl.aligned; ma.seam = pl.seam != 0;
    ma.nstrip = (int)cdiv(p.xc, own_cols(p, pl, pl.K, true));
    ma.undef = p.sc_.undef; ma.mask = ws->d_pmask;
    const int rc = for_member_chunks(member0, nmem, [&](int64_t m, int64_t nm) {
        ma.member0 = m;
        hipLaunchKernelGGL(k_pipe_masks, dim3((unsigned)cdiv(p.yc, 4), (unsigned)ma.nstrip, (unsigned)nm), dim3(256), 0, st, ma);
        return XINV_OK;
    });
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

static int launch_fused9(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st, const SweepLaunch &L)
{
    FusedArgs a;
    fused_args(a, p, pl, ws, L, own_cols(p, pl, L.k));
    const int nc = (p.kind == KIND_GEN2D) ? 7 : 4;
    for (int q = 0; q < nc; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
    if (pl.skip && L.k == pl.K) set_skip(a, ws, p, pl, 4);
    set_lag(a, ws, p, L.k, L);
    for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) {
        a.member0 = m;
        kernel_launch(pl.kern[L.k], dim3((unsigned)a.nwg + (L.lag_tag ? 1u : 0u), (unsigned)nm, 1), 0, st, a);
        return XINV_OK;
    });
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

static int launch_fused3d(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st, const SweepLaunch &L)
{
    Fused3Args a;
    memset(&a, 0, sizeof a);
    a.src = L.src; a.dst = L.dst; a.sS = p.sS;
    for (int q = 0; q < 4; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
    a.zc = p.zc; a.yc = p.yc; a.xc = p.xc;
    a.per = (p.BCx == XINV_BC_PERIODIC);
    a.force = L.force; a.no_ctl = L.no_ctl;
    a.sc_ = p.sc_; a.ctl = ws->ctl; a.stop = p.stop;
    a.psum = (unsigned long long *)ws->partials;
    if (L.k == 2) {                                      // two sweeps per pass (k_pipe3d): its own tiling
        a.nstrip = pl.nsg2; a.njb = pl.nrb2; a.joff = pl.joff2;
        a.nkc = std::max(1, pl.nkc2); a.KC = pl.KC2;
        a.rowf = (const double *)ws->d_rowf; a.srowf = pl.srowf2;
        const int64_t NT2 = (int64_t)a.nstrip * a.njb;
        // a flat grid over the members of the launch (k_pipe3d); at most 2^30 workgroups per launch
        const int64_t mstep = std::max<int64_t>(1, std::min<int64_t>(XINV_MEMBER_CHUNK, ((int64_t)1 << 30) / (NT2 * a.nkc)));
        const bool ext2 = (p.BCy == XINV_BC_EXTEND);
        for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) {
            a.member0 = m;
            // 'extend': the pre-pass of the pass's first sweep, in place on the source (numbas.py:87-115; idempotent: a
            // pass redone from this source by the one-sweep kernel applies it again to the same effect); the second
            // sweep's is applied inside the kernel (xinv_pipe3d.h: EXT).  A no-op for a member that has stopped.
            if (ext2)
                for_member_chunks(m, nm, [&](int64_t q, int64_t nq) { launch_extend(p, ws, st, const_cast<double *>(L.src), L.force, q, nq); return XINV_OK; });
            // which tiles march the whole column, which are cut into the plan's k chunks (xinv_p3_whole_tiles)
            a.nfull = xinv_p3_whole_tiles(NT2 * nm, a.nkc, a.KC, p.zc, pl.cus);
            const int64_t nwg = a.nfull + (NT2 * nm - a.nfull) * a.nkc;
            kernel_launch(pl.kern[2], dim3((unsigned)nwg, 1, 1), 0, st, a);
            return XINV_OK;
        }, mstep);
    } else {
        a.nstrip = pl.nsg; a.njb = pl.nrb;
        a.nkc = std::max(1, pl.nkc); a.KC = pl.KC;
        const size_t NB = (size_t)pl.nsg * pl.nrb * a.nkc;
        for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) {
            a.member0 = m;
            kernel_launch(pl.kern[L.k], dim3((unsigned)NB, (unsigned)nm, 1), 0, st, a);
            return XINV_OK;
        });
    }
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

// ---- biharmonic one-pass launch (A..I x-uniform) ----------------------------------------------
static int launch_fusedbih(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st, const SweepLaunch &L)
{
    // (prepass = false: finalise() redoing a pass whose source already carries that pass's pre-pass -- the periodic
    //  pre-pass, r0 <- r1 then r1 <- r2, is not idempotent)
    if (p.BCy == XINV_BC_EXTEND && L.prepass)        // the kernel's own pre-pass, on the source buffer
        for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) { launch_extend(p, ws, st, const_cast<double *>(L.src), L.force, m, nm); return XINV_OK; });
    FusedBihArgs a;
    memset(&a, 0, sizeof a);
    a.src = L.src; a.dst = L.dst; a.sS = p.sS;
    for (int q = 0; q < 10; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
    a.yc = p.yc; a.xc = p.xc; a.per = (p.BCx == XINV_BC_PERIODIC);
    a.nstrip = (int)cdiv(p.xc, own_cols(p, pl, 1)); a.nrb = pl.nrb; a.RB = pl.RY;
    a.nwg = (int)cdiv((int64_t)a.nstrip * a.nrb, 4);
    a.force = L.force; a.no_ctl = L.no_ctl;
    a.sc_ = p.sc_; a.ctl = ws->ctl; a.stop = p.stop;
    a.rowf = (const double *)ws->d_rowf;
    a.q = pl.bih_vm ? (const double *)ws->d_pfac : nullptr;
    a.psum = (unsigned long long *)ws->partials;
    if (pl.skip) set_skip(a, ws, p, pl, 4);
    set_lag(a, ws, p, 1, L);
    for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) {
        a.member0 = m;
        kernel_launch(pl.kern[1], dim3((unsigned)a.nwg + (L.lag_tag ? 1u : 0u), (unsigned)nm, 1), 0, st, a);
        return XINV_OK;
    });
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

static int launch_fused3dg(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st, const SweepLaunch &L)
{
    Fused3GArgs a;
    memset(&a, 0, sizeof a);
    a.src = L.src; a.dst = L.dst; a.sS = p.sS;
    for (int q = 0; q < 8; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
    a.zc = p.zc; a.yc = p.yc; a.xc = p.xc;
    a.per = (p.BCx == XINV_BC_PERIODIC);
    a.nstrip = pl.nsg; a.njb = pl.nrb;
    a.nkc = std::max(1, pl.nkc); a.KC = pl.KC;
    a.force = L.force; a.no_ctl = L.no_ctl;
    a.sc_ = p.sc_; a.ctl = ws->ctl; a.stop = p.stop;
    const size_t NB = (size_t)pl.nsg * pl.nrb * a.nkc;
    a.psum = (unsigned long long *)ws->partials;
    for_member_chunks(L.member0, L.nmem, [&](int64_t m, int64_t nm) {
        a.member0 = m;
        kernel_launch(pl.kern[1], dim3((unsigned)NB, (unsigned)nm, 1), 0, st, a);
        return XINV_OK;
    });
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

// one full coloured sweep (+ norm + stop rule) in place on p.S
// Order of the colour launches of one sweep (the oracle's seq_colour): with the odd-xc periodic seam each seam colour
// (column xc-1, rows of one parity) runs right after the base colour its points would otherwise belong to.
static inline int seam_sequence(int pos, int base, int seam)
{
    static const int s2[4] = {0, 2, 1, 3}, s4[6] = {0, 4, 1, 2, 5, 3};
    if (!seam) return pos;
    return base == 2 ? s2[pos] : s4[pos];
}

static int launch_colour_chunk(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st,
                               int64_t m0, int64_t nm)
{
    const int per = (p.BCx == XINV_BC_PERIODIC);
    if (p.BCy == XINV_BC_EXTEND) launch_extend(p, ws, st, p.S, 0, m0, nm);
    if (p.kind == KIND_BIH2D) {
        ColourArgsBih a;
        memset(&a, 0, sizeof a);
        a.S = p.S; a.sS = p.sS;
        for (int q = 0; q < 10; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
        a.yc = p.yc; a.xc = p.xc; a.per = per; a.trail = pl.seam; a.force = 0; a.member0 = m0;
        a.sc_ = p.sc_; a.ctl = ws->ctl; a.umask = pl.umask;
        dim3 b(64, 4, 1);
        dim3 g(cdiv(cdiv(p.xc, 3) + 1, 64), cdiv(cdiv(p.yc, 3) + 1, 4), (unsigned)nm);
        if (!per || p.xc % 3 == 0) {
            // one launch per row class does its three column colours in registers (periodic x needs
            // xc % 3 == 0 so that the wrap keeps colour == column % 3; otherwise nine + trailing colours)
            dim3 gb(cdiv(cdiv(p.xc, 180), 4), cdiv(p.yc, 3) + 1, (unsigned)nm), bb(256, 1, 1);
            a.Y = ws->S2; a.sY = p.sS;                     // side buffer (allocated by solve_dev for this path)
            for (int cj = 0; cj < 3; cj++) {
                a.colour = cj;
                if (per) {
                    if (pl.umask) hipLaunchKernelGGL((k_bih_rowclass<true, true>), gb, bb, 0, st, a);
                    else          hipLaunchKernelGGL((k_bih_rowclass<false, true>), gb, bb, 0, st, a);
                } else {
                    if (pl.umask) hipLaunchKernelGGL((k_bih_rowclass<true, false>), gb, bb, 0, st, a);
                    else          hipLaunchKernelGGL((k_bih_rowclass<false, false>), gb, bb, 0, st, a);
                }
            }
            hipLaunchKernelGGL(k_rows_copy_back, dim3(256, (unsigned)nm, 1), dim3(256), 0, st,
                               (const double *)ws->S2, p.sS, p.S, p.sS, p.yc, p.xc,
                               (const XinvCtl *)ws->ctl, m0, 0);
        } else
        for (int cc = 0; cc < pl.ncol; cc++) {
            a.colour = cc;
            if (pl.umask) hipLaunchKernelGGL(k_colour_bih2d<true>, g, b, 0, st, a);
            else          hipLaunchKernelGGL(k_colour_bih2d<false>, g, b, 0, st, a);
        }
    } else if (is3d(p.kind)) {
        ColourArgs3D a;
        memset(&a, 0, sizeof a);
        a.S = p.S; a.sS = p.sS;
        for (int q = 0; q < p.ncoef; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
        a.zc = p.zc; a.yc = p.yc; a.xc = p.xc;
        a.per = per; a.seam = pl.seam; a.force = 0; a.sc_ = p.sc_; a.ctl = ws->ctl;
        a.nbatch = p.nbatch; a.member0 = m0;
        dim3 b(64, 4, 1);
        dim3 g(cdiv(cdiv(p.xc, 2) + 1, 64), cdiv(p.yc - 2, 4), (unsigned)(nm * (p.zc - 2)));
        for (int pos = 0; pos < pl.ncol; pos++) {
            a.colour = seam_sequence(pos, 2, pl.seam);
            if (p.kind == KIND_GEN3D) hipLaunchKernelGGL(k_colour_gen3d, g, b, 0, st, a);
            else                      hipLaunchKernelGGL(k_colour_std3d, g, b, 0, st, a);
        }
    } else {
        ColourArgs2D a;
        memset(&a, 0, sizeof a);
        a.S = p.S; a.sS = p.sS;
        for (int q = 0; q < p.ncoef; q++) { a.c[q] = p.c[q]; a.sc[q] = p.sc[q]; }
        a.yc = p.yc; a.xc = p.xc;
        a.per = per; a.base = pl.base; a.seam = pl.seam; a.force = 0;
        a.sc_ = p.sc_; a.ctl = ws->ctl; a.member0 = m0;
        dim3 b(64, 4, 1);
        dim3 g(cdiv(cdiv(p.xc, 2) + 1, 64), cdiv(p.yc - 2, 4), (unsigned)nm);
        const bool nine = (pl.base == 4);
        for (int pos = 0; pos < pl.ncol; pos++) {
            a.colour = seam_sequence(pos, pl.base, pl.seam);
            if (p.kind == KIND_STD2D) {
                if (nine) hipLaunchKernelGGL(k_colour_std2d<true>, g, b, 0, st, a);
                else      hipLaunchKernelGGL(k_colour_std2d<false>, g, b, 0, st, a);
            } else if (p.kind == KIND_STD2DT) {
                if (nine) hipLaunchKernelGGL(k_colour_std2dt<true>, g, b, 0, st, a);
                else      hipLaunchKernelGGL(k_colour_std2dt<false>, g, b, 0, st, a);
            } else {
                if (nine) hipLaunchKernelGGL(k_colour_gen2d<true>, g, b, 0, st, a);
                else      hipLaunchKernelGGL(k_colour_gen2d<false>, g, b, 0, st, a);
            }
        }
    }
    NormArgs n;
    n.S = p.S; n.sS = p.sS; n.n = p.zc * p.yc * p.xc; n.undef = p.sc_.undef;
    n.psum = (double *)ws->partials;
    n.pcnt = (long long *)((char *)ws->partials + p.nbatch * XINV_NORM_BLOCKS * sizeof(double));
    n.ctl = ws->ctl; n.stop = p.stop; n.force = 0; n.member0 = m0;
    int nblk = (int)std::min<int64_t>(XINV_NORM_BLOCKS, std::max<int64_t>(1, n.n / 2048));
    hipLaunchKernelGGL(k_norm_partial, dim3(nblk, (unsigned)nm, 1), dim3(256, 1, 1), 0, st, n);
    hipLaunchKernelGGL(k_norm_final, dim3((unsigned)nm, 1, 1), dim3(64, 1, 1), 0, st, n, nblk);
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

static int launch_colour_sweep(const Problem &p, const Plan &pl, Workspace *ws, hipStream_t st)
{
    // grid.z carries members (x planes in 3-D) and is limited to 65535
    int64_t chunk = XINV_MEMBER_CHUNK;
    if (is3d(p.kind)) chunk = std::max<int64_t>(1, 65535 / std::max<int64_t>(1, p.zc - 2));
    return for_member_chunks(0, p.nbatch, [&](int64_t m0, int64_t nm) { return launch_colour_chunk(p, pl, ws, st, m0, nm); }, chunk);
}

// The tiling cost model of the fused 2-D kernels -- xinv_tile_cost, and xinv_choose_row_blocks which minimises it: xinv_tiles.h,
// checked on the CPU -- with the kernels' constants: at most three workgroups of k_fused2d / k_fused9 per CU count; of the
// pipelined kernel up to XINV_PIPE_OCC workgroups -- one wavefront each per SIMD -- share a CU.  For the pipelined pass
// `rows` is the height of the split's TALLEST tile (tallest_tile below): its steps are the kernel's own count.
static int pipe_occ_cap()
{
    return std::max(1, XINV_ENV_INT("XINV_PIPE_OCC", 5));
}

static double tile_cost(int64_t wgs, int64_t rows, int K, int occ, double lone, bool pipe)
{
    return xinv_tile_cost(wgs, rows, K, occ, pipe ? pipe_occ_cap() : 3, lone, pipe ? XINV_PIPE_LAG : 0, pipe ? XINV_PIPE_B : 0,
                          XINV_PIPE_PF0 + 4, XINV_PIPE_PF + 4);
}

static int64_t choose_row_blocks(int64_t yc, int64_t nstrip, int64_t nbatch, int K, int occ, double lone, bool pipe)
{
    return xinv_choose_row_blocks(yc, nstrip, nbatch, K, occ, pipe ? pipe_occ_cap() : 3, lone, pipe ? XINV_PIPE_LAG : 0,
                                  pipe ? XINV_PIPE_B : 0, XINV_PIPE_PF0 + 4, XINV_PIPE_PF + 4);
}

// How many workgroups of the planned kernel variant fit on a CU at K sweeps per pass (2-D forms; the 3-D kernels fill a
// CU with one).  *have (when given): the variant exists; where it does not, the answer is the family's default.
static int plan_occ(const Problem &p, const Plan &pl, int K, bool *have = nullptr)
{
    SweepVariant v = plan_variant(p, pl, K);
    // (the biharmonic tiling has always been planned with the non-periodic kernel of the plan's stream mode, with the
    //  mixed terms unless that mode never has them: a plan's row split must not move with which one is asked)
    if (p.kind == KIND_BIH2D) v.per = v.zbe = false;
    const KernelRef k = xinv_kernel(v);
    if (have) *have = k.fn != nullptr;
    return k.fn ? kernel_occupancy(k) : (pl.nine ? 1 : 2);
}

// rows_per_tile > 0: tiles of that many rows (rounded up to even); < 0: exactly that many row blocks, split evenly; 0
// (returns false): the caller's cost model picks the number of row blocks, split_rows_evenly() then.
static void split_rows_evenly(const Problem &p, Plan &pl, int64_t nrb)
{
    pl.nrb = (int)nrb;
    pl.even_split = true;
    pl.RY = (int)cdiv(p.yc, pl.nrb);
}
static bool rows_per_tile_given(const Problem &p, const xinv_options &opt, Plan &pl)
{
    pl.even_split = false;
    if (opt.rows_per_tile > 0) {
        pl.RY = (opt.rows_per_tile + 1) & ~1;
        pl.nrb = (int)cdiv(p.yc, pl.RY);
    } else if (opt.rows_per_tile < 0)
        split_rows_evenly(p, pl, std::max<int64_t>(1, std::min<int64_t>(-opt.rows_per_tile, p.yc / 2)));
    return opt.rows_per_tile != 0;
}

// k_pipe2d's tile records (xinv_tiles.h: PipeTileRec): the kernel's constants they depend on
static inline PipeTileGeom pipe_tile_geom()
{
    return PipeTileGeom{2 * XINV_PIPE_P, XINV_PIPE_UW, XINV_PIPE_LAG, XINV_PIPE_B, XINV_PIPE_PF0 + 4, XINV_PIPE_PF + 4};
}
// ... of a pipelined plan that skips no tile: one set of nstrip x nrb records for every member, alone in ws->d_list.  A
// solve without a plan that finds the records of the same tiling in place uploads nothing (ws->trec_key).
// (With a tile list the records ride behind it: plan_tile_skip.)
static int plan_pipe_tile_recs(const Problem &p, Plan &pl, Workspace *ws, hipStream_t st)
{
    if (!pl.pipe || pl.skip) return XINV_OK;
    const int nstrip = (int)cdiv(p.xc, own_cols(p, pl, pl.K, true));
    const int RY = pl.even_split ? 0 : pl.RY, nrb = pl.even_split ? pl.nrb : (int)cdiv(p.yc, pl.RY);
    const bool per = p.BCx == XINV_BC_PERIODIC;
    pl.trec_off = 0; pl.trec_ms = 0;
    const Workspace::TrecKey key = {p.yc, p.xc, nstrip, nrb, RY, per ? 1 : 0, pl.seam ? 1 : 0, 1};
    const Workspace::TrecKey &k = ws->trec_key;
    if (ws->d_list && k.valid && k.yc == key.yc && k.xc == key.xc && k.nstrip == key.nstrip && k.nrb == key.nrb &&
        k.RY == key.RY && k.per == key.per && k.seam == key.seam)
        return XINV_OK;
    const size_t bytes = (size_t)nstrip * nrb * sizeof(PipeTileRec);
    ws->trec_key.valid = 0;
    int rc = ensure_dev(&ws->d_list, &ws->d_list_cap, bytes);
    if (rc) return rc;
    if ((rc = ensure_pinned(&ws->h_list, &ws->h_list_cap, bytes, hipHostMallocDefault))) return rc;
    xinv_pipe_identity_recs((PipeTileRec *)ws->h_list, nstrip, nrb, p.yc, RY, p.xc, per, pl.seam != 0, pipe_tile_geom());
    HIPCHK(hipMemcpyAsync(ws->d_list, ws->h_list, bytes, hipMemcpyHostToDevice, st));
    ws->trec_key = key;
    return XINV_OK;
}

// Masked-tile skipping for the 5-point fused kernels.  Wave-tiles whose forcing is undefined at
// every owned point (land, topography, polar caps) can never change (every mask predicate of the
// reference tests the forcing), so launches run the other tiles only; the row split is re-chosen
// so that the ACTIVE tiles fill the CUs evenly, and the skipped tiles' constant share of the norm
// is computed once.  Decided per solve from one pass over the forcing.
// `fixedRB` > 0 (biharmonic one-pass kernel): tiles are row blocks of exactly fixedRB rows x own_cols() owned
// columns and the split is kept; 0: the 5-point kernels' even split, re-planned for the active tiles.
// The activity map of the forcing for strips of UW owned columns: kernel + copy to the host, NOT synchronised.  The planner
// of the lat-lon forms issues it ahead of the x-uniform detection with the strip width those forms end up with, so that
// ONE host round trip brings both answers (25 us of a 4.6 ms headline solve); plan_tile_skip issues it itself otherwise.
static int issue_strip_active(const Problem &p, Workspace *ws, hipStream_t st, int UW, int fi)
{
    const int64_t yc = p.yc, nb = p.nbatch;
    const int nstrip = (int)cdiv(p.xc, UW);
    const int64_t cells = yc * nstrip;
    int rc = ensure_dev(&ws->d_act, &ws->d_act_cap, (size_t)(nb * cells));
    if (rc) return rc;
    if ((rc = ensure_pinned(&ws->h_act, &ws->h_act_cap, (size_t)(nb * cells), hipHostMallocDefault))) return rc;
    StripActArgs sa;
    sa.f = p.c[fi]; sa.sf = p.sc[fi]; sa.yc = yc; sa.xc = p.xc; sa.nstrip = nstrip; sa.UW = UW;
    sa.undef = p.sc_.undef; sa.act = ws->d_act;
    hipLaunchKernelGGL(k_strip_active, dim3(cdiv(cells, 4), (unsigned)nb, 1), dim3(256), 0, st, sa);
    HIPCHK(hipMemcpyAsync(ws->h_act, ws->d_act, (size_t)(nb * cells), hipMemcpyDeviceToHost, st));
    ws->act_ready = true; ws->act_uw = UW; ws->act_f = p.c[fi]; ws->act_synced = false;
    return XINV_OK;
}

static int plan_tile_skip(const Problem &p, Plan &pl, Workspace *ws, hipStream_t st,
                          const xinv_options &opt, int fixedRB = 0)
{
    pl.skip = false; pl.ntl = pl.nskip = 0; pl.skip_pct = 0; pl.skip_ppm = 0;
    const bool forced = (opt.flags & XINV_FLAG_FORCE_TILE_SKIP) != 0;
    const int tpw = pl.pipe ? 1 : 4;                              // wave-tiles per workgroup
    const int K = pl.K, UW = own_cols(p, pl, K, pl.pipe);
    const int nstrip = (int)cdiv(p.xc, UW);
    const int64_t wscale = 4 / tpw;                       // (thresholds in wavefronts: a pipelined tile has four)
    if (!forced && ((int64_t)nstrip * pl.nrb * p.nbatch * wscale < 1024 || (int64_t)nstrip * pl.nrb * wscale < 64 ||
                    p.nbatch > 64))
        return XINV_OK;                                   // small problems: nothing to balance
    const int64_t yc = p.yc, nb = p.nbatch;
    const int64_t cells = yc * nstrip;
    if (nb * nstrip * (yc + 1) > (int64_t)50000000) return XINV_OK;   // host-side prefix table would exceed 200 MB
    const StreamMap &sm = stream_map(p.kind);
    const int fi = (p.kind == KIND_BIH2D) ? 9 : sm.c[sm.forcing];      // the forcing (biharmonic form: J, the last of its ten arrays)

    int rc = XINV_OK;
    if (!(ws->act_ready && ws->act_uw == UW && ws->act_f == p.c[fi])) {     // (not already there: issue_strip_active below)
        rc = issue_strip_active(p, ws, st, UW, fi);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(st));
    } else if (!ws->act_synced)                           // (issued ahead, and no detection pass synchronised behind it)
        HIPCHK(hipStreamSynchronize(st));
    ws->act_ready = false;

    // prefix counts of active rows per (member, strip), laid out [member][row][strip]: building them and looking up the
    // two rows of a row block for every strip both run along contiguous memory (this planning is host time inside every
    // solve: 155 us of a 4.9 ms headline solve with the [member][strip][row] layout and per-tile id decoding)
    std::vector<int> &pre = ws->h_pre;
    pre.resize((size_t)(nb * nstrip * (yc + 1)));
    int64_t nact = 0;
    for (int64_t m = 0; m < nb; m++) {
        int *q = &pre[(size_t)(m * (yc + 1) * nstrip)];
        for (int s = 0; s < nstrip; s++) q[s] = 0;
        const unsigned char *ha = ws->h_act + m * yc * nstrip;
        for (int64_t r = 0; r < yc; r++, q += nstrip, ha += nstrip)
            for (int s = 0; s < nstrip; s++) q[nstrip + s] = q[s] + ha[s];
        for (int s = 0; s < nstrip; s++) nact += q[s];
    }
    if (!forced && (double)nact > 0.92 * (double)(nb * cells)) return XINV_OK;     // little to skip
    auto rows_active = [&](int64_t m, int strip, int64_t y0, int64_t y1) {
        const int *q = &pre[(size_t)(m * (yc + 1) * nstrip)];
        return q[y1 * nstrip + strip] - q[y0 * nstrip + strip] > 0;
    };

    const bool ext = (p.BCy == XINV_BC_EXTEND);
    // (tile ids and their rows: xinv_tile_rows -- with the odd-xc periodic seam the edge strips' row blocks are two tiles)
    auto ntile_ids = [&](int nrb) { return nstrip * nrb; };
    auto id_rb = [&](int, int id) { return id / nstrip; };
    auto tile_active = [&](int64_t m, int nrb, int id) {
        const int rb = id_rb(nrb, id);
        const TileRows t = xinv_tile_rows(id, nstrip, nrb, yc, fixedRB);
        if (t.y0 >= t.y1) return false;
        if (ext && (rb == 0 || rb >= nrb - (fixedRB ? 2 : 1))) return true;    // the boundary rows get their copy
                                                               // (a last block of one row: yc-2 sits in the one before)
        return rows_active(m, t.strip, t.y0, t.y1);
    };
    auto active_wgs = [&](int nrb, int64_t *maxact) {
        int64_t wgs = 0, mx = 0;
        for (int64_t m = 0; m < nb; m++) {
            int64_t c = 0;
            const int *q = &pre[(size_t)(m * (yc + 1) * nstrip)];                // (the rows of a block once, then its strips)
            for (int rb = 0; rb < nrb; rb++) {
                const TileRows t = xinv_tile_rows(rb * nstrip, nstrip, nrb, yc, fixedRB);
                if (t.y0 >= t.y1) continue;
                if (ext && (rb == 0 || rb >= nrb - (fixedRB ? 2 : 1))) { c += nstrip; continue; }
                const int *q0 = q + t.y0 * nstrip, *q1 = q + t.y1 * nstrip;
                for (int st_ = 0; st_ < nstrip; st_++) c += (q1[st_] - q0[st_]) > 0;
            }
            wgs += cdiv(c, tpw); mx = std::max(mx, c);
        }
        if (maxact) *maxact = mx;
        return wgs;
    };
    const int occ = fixedRB ? 2 : plan_occ(p, pl, K);
    const bool pp = pl.pipe;
    // the rows tile_cost is handed for a split into nrb blocks: the pipelined pass is costed by its tallest tile
    auto cost_rows = [&](int nrb) -> int64_t {
        if (!pp) return cdiv(yc, nrb);
        return pl.even_split ? xinv_even_split_tallest(yc, nrb) : std::min<int64_t>(pl.RY, yc);
    };
    const double cost0 = tile_cost((int64_t)cdiv((int64_t)nstrip * pl.nrb, tpw) * nb, cost_rows(pl.nrb), K, occ, pl.lone, pp);
    // candidates: the row split that brings the ACTIVE workgroups back to the default count sits
    // near nrb / (active share); search a window around it
    int best = pl.nrb; double best_cost = 1e300;
    int lo = pl.nrb, hi = pl.nrb;
    if (!forced && opt.rows_per_tile == 0 && !fixedRB) {
        const int64_t w0 = active_wgs(pl.nrb, nullptr);
        const double share = std::max(0.05, (double)w0 / (double)((int64_t)cdiv((int64_t)nstrip * pl.nrb, tpw) * nb));
        const double centre = (double)pl.nrb / share;
        const int64_t cap_rows = std::max<int64_t>(pl.nrb, yc / 4);
        lo = (int)std::min<int64_t>(cap_rows, std::max<int64_t>(pl.nrb, (int64_t)(centre * 0.85)));
        hi = (int)std::min<int64_t>(cap_rows, std::max<int64_t>(lo, (int64_t)(centre * 1.10) + 1));
    }
    best_cost = tile_cost(active_wgs(pl.nrb, nullptr), cost_rows(pl.nrb), K, occ, pl.lone, pp);   // keep the split, skip only
    for (int nrb = lo; nrb <= hi; nrb++) {
        const double c = tile_cost(active_wgs(nrb, nullptr), cost_rows(nrb), K, occ, pl.lone, pp);
        if (c < best_cost) { best_cost = c; best = nrb; }
    }
    if (!forced && best_cost > 0.95 * cost0) return XINV_OK;            // (fixed split: skipping must save 5 % of the workgroups)

    // lists for the chosen split
    int64_t maxact = 0;
    active_wgs(best, &maxact);
    const int64_t ntiles = (int64_t)ntile_ids(best);
    const int ntl = (int)(tpw * std::max<int64_t>(1, cdiv(maxact, tpw)));
    int64_t maxskip = 0, nskipped = 0;
    std::vector<std::vector<int>> act((size_t)nb), skp((size_t)nb);
    for (int64_t m = 0; m < nb; m++) {
        for (int id = 0; id < (int)ntiles; id++) {
            const TileRows t = xinv_tile_rows(id, nstrip, best, yc, fixedRB);
            if (t.y0 >= t.y1) continue;
            (tile_active(m, best, id) ? act[(size_t)m] : skp[(size_t)m]).push_back(id);
        }
        maxskip = std::max<int64_t>(maxskip, (int64_t)skp[(size_t)m].size());
        nskipped += (int64_t)skp[(size_t)m].size();
    }
    if (nskipped == 0) return XINV_OK;
    const int nskip = (int)maxskip;
    const size_t nints = (size_t)nb * ((size_t)ntl + nskip);
    // (the pipelined pass: one tile record per list entry behind the lists -- they travel in the same copy)
    const bool recs = pl.pipe && !fixedRB;
    const size_t rec_off = (nints * sizeof(int) + 31) & ~(size_t)31;
    const size_t list_bytes = recs ? rec_off + (size_t)nb * ntl * sizeof(PipeTileRec) : nints * sizeof(int);
    rc = ensure_dev(&ws->d_list, &ws->d_list_cap, list_bytes);
    if (rc) return rc;
    if ((rc = ensure_pinned(&ws->h_list, &ws->h_list_cap, list_bytes, hipHostMallocDefault))) return rc;
    ws->trec_key.valid = 0;
    int *hl = ws->h_list, *hs = ws->h_list + (size_t)nb * ntl;
    for (int64_t m = 0; m < nb; m++) {
        std::vector<int> &am = act[(size_t)m];
        if (pl.seam && !fixedRB) {
            // odd-xc periodic seam: the edge strips' tiles (two passes per half-sweep) are dispatched first, spread over
            // the XCDs (xinv_heavy_first; the kernels do the same arithmetic when there is no list)
            auto heavy = [&](int id) { const int s_ = id % nstrip; return s_ == 0 || s_ == nstrip - 1; };
            const int nh = (int)(std::stable_partition(am.begin(), am.end(), heavy) - am.begin());
            const int nwg = ntl / tpw, q = nwg >> 3, rem = nwg & 7;
            for (int L = 0; L < nwg; L++) {
                const int xcd = L & 7, T = xcd * q + std::min(xcd, rem) + (L >> 3);
                const int sq = xinv_heavy_first(L, nwg, nh / tpw);
                for (int w = 0; w < tpw; w++)
                    hl[m * ntl + T * tpw + w] = sq * tpw + w < (int)am.size() ? am[(size_t)(sq * tpw + w)] : -1;
            }
        } else
        for (int t = 0; t < ntl; t++) hl[m * ntl + t] = t < (int)am.size() ? am[(size_t)t] : -1;
        for (int t = 0; t < nskip; t++) hs[m * nskip + t] = t < (int)skp[(size_t)m].size() ? skp[(size_t)m][t] : -1;
    }
    if (recs) {
        PipeTileRec *hr = (PipeTileRec *)((char *)ws->h_list + rec_off);
        const PipeTileGeom g = pipe_tile_geom();
        const bool per = p.BCx == XINV_BC_PERIODIC;
        // (a tile's record is the same for every member: built once per tile id, copied per list entry)
        std::vector<PipeTileRec> &byid = ws->h_trec;
        byid.resize((size_t)ntiles + 1);
        for (int id = 0; id < (int)ntiles; id++) byid[(size_t)id] = xinv_pipe_tile_rec(id, nstrip, best, yc, 0, p.xc, per, pl.seam != 0, g);
        byid[(size_t)ntiles] = xinv_pipe_tile_rec(-1, nstrip, best, yc, 0, p.xc, per, pl.seam != 0, g);
        for (size_t e = 0; e < (size_t)nb * ntl; e++) hr[e] = byid[(size_t)(hl[e] < 0 ? ntiles : hl[e])];
        pl.trec_off = rec_off; pl.trec_ms = ntl;
    }
    HIPCHK(hipMemcpyAsync(ws->d_list, ws->h_list, list_bytes, hipMemcpyHostToDevice, st));
    rc = ensure_dev(&ws->d_tsum, &ws->d_tsum_cap, tsum_layout(nullptr, nb, nskip).bytes);
    if (rc) return rc;
    const TsumPtrs ts = tsum_layout(ws->d_tsum, nb, nskip);
    HIPCHK(hipMemsetAsync(ts.ticket, 0, (size_t)nb * sizeof(unsigned), st));   // k_skip_tiles' tickets
    SkipNormArgs na;
    na.S = p.S; na.sS = p.sS; na.yc = yc; na.xc = p.xc; na.nstrip = nstrip; na.nrb = best; na.UW = UW; na.RB = fixedRB;
    na.undef = p.sc_.undef; na.skip_list = ws->d_list + (size_t)nb * ntl; na.nskip_max = nskip;
    na.tsum = ts.tsum; na.tcnt = ts.tcnt; na.xsum = ts.xsum; na.xcnt = ts.xcnt; na.ticket = ts.ticket;
    pl.skipna = na;                                      // (the skipped tiles' norm share and their copies: run_sweeps)

    pl.skip = true; pl.ntl = ntl; pl.nskip = nskip;
    pl.skip_pct = (int)((100 * nskipped) / (ntiles * nb));
    pl.skip_ppm = (int)((1000000 * nskipped) / (ntiles * nb));
    if (!fixedRB) {
        split_rows_evenly(p, pl, best);
        pl.nsg = (int)cdiv((int64_t)cdiv(p.xc, 128 - (pl.nine ? 8 : 4) * XINV_KMAX - (pl.seam ? 4 : 0)) * pl.nrb, pl.pipe ? 4 : tpw) + 1;
        if (pl.pipe) pl.nsg = std::max(pl.nsg, (int)cdiv(p.xc, UW) * pl.nrb + 1);
    }
    return XINV_OK;
}

// Which of `nstream` arrays have rows (of xc elements, `rows` per member) that are bitwise constant
// along x?  One pass over each array on the device; *mask gets bit q set for uniform array q.
static int detect_xuniform(Workspace *ws, hipStream_t st, const double *const *arr,
                           const int64_t *stride, int nstream, int64_t nbatch, int64_t rows,
                           int64_t xc, unsigned *mask)
{
    XUniArgs xa;
    memset(&xa, 0, sizeof xa);
    xa.nstream = nstream;
    for (int q = 0; q < nstream; q++) { xa.c[q] = arr[q]; xa.stride[q] = stride[q]; }
    xa.nbatch = nbatch; xa.yc = rows; xa.xc = xc;
    if (!ws->dflags16) {
        HIPCHK(hipMalloc((void **)&ws->dflags16, 16 * sizeof(int)));
        HIPCHK(hipHostMalloc((void **)&ws->hflags16, 16 * sizeof(int), hipHostMallocDefault));
    }
    xa.flag = ws->dflags16;
    HIPCHK(hipMemsetAsync(ws->dflags16, 0, 16 * sizeof(int), st));
    hipLaunchKernelGGL(k_xuniform, dim3(512, (unsigned)nstream, 1), dim3(256), 0, st, xa);
    HIPCHK(hipMemcpyAsync(ws->hflags16, ws->dflags16, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ws->act_synced = true;                                // (an activity map issued ahead on this stream has landed too)
    *mask = 0;
    for (int q = 0; q < nstream; q++) if (!ws->hflags16[q]) *mask |= (1u << q);
    return XINV_OK;
}

static thread_local unsigned t_detected_um = 0;       // coefficient arrays (bit = coefficient index) the calling thread's last
                                                      // plan found constant along x (or knew to be): solve_host_one hands the
                                                      // shared ones to the later chunks of the same call
// The same over coefficient arrays idx[0..ns) of a problem; bit q of *mask = array idx[q].  Arrays the caller declared
// row-constant to a resident plan (Problem::known_um: the plan expanded them itself) are not read again.
static int detect_xuniform_of(const Problem &p, Workspace *ws, hipStream_t st, const int *idx, int ns, int64_t rows,
                              unsigned *mask)
{
    const double *arr[10]; int64_t strd[10]; int pos[10];
    int nu = 0;
    unsigned m = 0;
    for (int q = 0; q < ns; q++) {
        if ((p.known_um >> idx[q]) & 1u) { m |= 1u << q; continue; }
        arr[nu] = p.c[idx[q]]; strd[nu] = p.sc[idx[q]]; pos[nu] = q; nu++;
    }
    if (nu) {
        unsigned mm = 0;
        const int rc = detect_xuniform(ws, st, arr, strd, nu, p.nbatch, rows, p.xc, &mm);
        if (rc) return rc;
        for (int k = 0; k < nu; k++) if ((mm >> k) & 1u) m |= 1u << pos[k];
    }
    for (int q = 0; q < ns; q++) if ((m >> q) & 1u) t_detected_um |= 1u << idx[q];
    *mask = m;
    return XINV_OK;
}
