// xinv_plan.h -- the planner of libxinv_hip.so: colouring -> path -> tiling of the chosen kernel family, the once-per-solve
// detection passes, per-row records, point-factor streams and tile lists (everything a solve derives from the
// coefficient stack and the forcing's mask; nothing from S).  Included by xinv_hip.hip only, after xinv_launch.h.
#pragma once

// ------------------------------------------------------------------ planning
// solve_dev = plan (colouring -> path -> tiling of the chosen kernel family) -> sweep loop -> finalise.
// Every plan_* step fills `Plan`; the once-per-solve detection passes (is B zero? which arrays are
// constant along x? which tiles are fully masked?) run on the caller's stream and are synchronous.

// A flag pass: ws->dflag is cleared, `issue` launches the kernels that set bits in it, *flag gets what they left.
// Synchronises the stream.
template <class F>
static int flag_pass(Workspace *ws, hipStream_t st, int *flag, F issue)
{
    HIPCHK(hipMemsetAsync(ws->dflag, 0, sizeof(int), st));
    issue();
    HIPCHK(hipMemcpyAsync(ws->hflag, ws->dflag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *flag = *ws->hflag;
    return XINV_OK;
}

// ... over coefficient arrays: *nonzero = some element of one of them is not zero
static int any_nonzero(const Problem &p, Workspace *ws, hipStream_t st, std::initializer_list<int> arrays, int *nonzero)
{
    const int64_t n = p.zc * p.yc * p.xc;
    return flag_pass(ws, st, nonzero, [&] {
        for (int q : arrays) {
            const int64_t nb = (p.sc[q] == 0) ? n : (p.nbatch - 1) * p.sc[q] + n;
            hipLaunchKernelGGL(k_any_nonzero, dim3(1024), dim3(256), 0, st, p.c[q], nb, ws->dflag);
        }
    });
}

// red-black when the cross coefficient vanishes, else 4 colours; 9 for the biharmonic form; +seam colours
static int plan_colouring(const Problem &p, Workspace *ws, hipStream_t st, Plan &pl)
{
    if (is3d(p.kind)) {
        pl.base = 2;
    } else if (p.kind == KIND_BIH2D) {
        pl.base = 9;                                   // radius-2 stencil: (j%3, i%3)
    } else {
        bool bzero = (p.c[1] == nullptr);
        int nonzero = 0, rc = XINV_OK;
        if (p.kind == KIND_STD2DT && p.sc_.undef != 0.0) {          // cross coefficients B and C
            rc = any_nonzero(p, ws, st, {1, 2}, &nonzero);
            bzero = !nonzero;
        } else if (!bzero && p.sc_.undef != 0.0) {
            rc = any_nonzero(p, ws, st, {1}, &nonzero);
            bzero = !nonzero;
        }
        if (rc) return rc;
        pl.base = bzero ? 2 : 4;
    }
    if (p.kind == KIND_BIH2D) {
        pl.seam = (p.BCx == XINV_BC_PERIODIC) ? (int)(p.xc % 3) : 0;     // trailing columns
        pl.ncol = 9 + 3 * pl.seam;
    } else {
        pl.seam = (p.BCx == XINV_BC_PERIODIC) && (p.xc & 1);
        pl.xc = p.xc;
        pl.ncol = pl.base + (pl.seam ? 2 : 0);
    }
    return XINV_OK;
}

// biharmonic one-pass kernel: one pass per sweep; row blocks of RB rows (multiple of 3) x 180-column strips,
// four consecutive wave-tiles per workgroup; RB from the (workgroups per CU) x (steps) model
static int plan_fusedbih(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    pl.K = 1;
    pl.aligned = false;
    const int nstrip = (int)cdiv(p.xc, own_cols(p, pl, pl.K));
    int flag = 0;
    // no mixed derivatives (B == E == 0 everywhere)?  One flag pass over the two arrays.
    int rc = any_nonzero(p, ws, st, {1, 4}, &flag);
    if (rc) return rc;
    pl.bih_zbe = (flag == 0) && (p.sc_.undef != 0.0);
    // Where the coefficients come from (xinv_fusedbih.h): per-row records when A..I are constant along x; else the
    // vector-stream variants (round 6): A, C, D, F as streams when only they vary (A4(x, y), R(x, y) of
    // apps.py:1793-1836) and there are no mixed derivatives, all nine otherwise -- with the point-factor stream Q
    // (relaxation factor, 0 = the reference's predicate forbids the update), evaluated here, once per coefficient stack.
    pl.bih_vm = ((pl.umask & 0x1ffu) == 0x1ffu) ? 0 : ((pl.bih_zbe && (pl.umask & 0x1d2u) == 0x1d2u) ? 1 : 2);
    if (pl.bih_vm) {
        rc = ensure_dev(&ws->d_pfac, &ws->d_pfac_cap, (size_t)p.nbatch * p.yc * p.xc * sizeof(double));
        if (rc) return rc;
        PointFactorBihArgs fa;
        memset(&fa, 0, sizeof fa);
        for (int q = 0; q < 9; q++) { fa.c[q] = p.c[q]; fa.sc[q] = p.sc[q]; }
        fa.yc = p.yc; fa.xc = p.xc; fa.n = p.yc * p.xc; fa.sc_ = p.sc_; fa.q = ws->d_pfac; fa.flag = ws->dflag;
        rc = flag_pass(ws, st, &flag, [&] {
            hipLaunchKernelGGL(k_point_factor_bih, dim3((unsigned)std::min<int64_t>(2048, cdiv(fa.n, 256)), (unsigned)p.nbatch, 1),
                               dim3(256), 0, st, fa);
        });
        if (rc) return rc;
        if (pl.bih_vm == 1 && !(flag & 6)) pl.bih_vm = 3;      // A == C and D == F everywhere (bitwise): two streams less
        if (flag & 1) {                                  // (a factor of exactly zero somewhere: Q == 0 could not mean "skip")
            if (opt.path == XINV_PATH_FUSED)
                return fail_arg("biharmonic form: a relaxation factor of exactly zero on an updatable point -- the colour launches handle it");
            pl.path = XINV_PATH_COLOUR;
            return XINV_OK;
        }
    }
    const int occ = plan_occ(p, pl, pl.K);
    {   // per-row records (A..I, relaxation factor, row predicate), once per solve: xinv_fusedbih.h
        rc = ensure_dev(&ws->d_rowf, &ws->d_rowf_cap, (size_t)p.nbatch * p.yc * XINV_BIH_RW * sizeof(double));
        if (rc) return rc;
        RowFactorBihArgs ra;
        memset(&ra, 0, sizeof ra);
        for (int q = 0; q < 9; q++) { ra.c[q] = p.c[q]; ra.sc[q] = p.sc[q]; }
        ra.yc = p.yc; ra.xc = p.xc; ra.sc_ = p.sc_; ra.rowf = (double *)ws->d_rowf;
        hipLaunchKernelGGL(k_row_factor_bih, dim3((unsigned)cdiv(p.yc, 256), (unsigned)p.nbatch, 1), dim3(256), 0, st, ra);
    }
    // Time of a launch ~ (steps per tile) x f(workgroups per CU).  f measured on the round-3 kernel at 2000 x 2000
    // (profiles/r03_bih_rework.txt: rows 9 .. 33): one workgroup per CU 1.0; the second costs little (the
    // wavefronts fill each other's dependency stalls): 1.2 just above one per CU, 1.35 at two; a third 1.6 .. 1.75.
    // (the vector-stream variants, round 6, move 64 / 104 bytes per point and sweep and sit at what the fabric delivers
    //  -- 6.4 TB/s at 2000 x 2000 whatever the tile height: a second workgroup on a CU takes as long again, so the launch
    //  is planned in whole rounds of ONE workgroup per CU and what counts are the ten halo rows per tile: 15-row tiles
    //  67.5 us, 24-row tiles -- 273 workgroups -- 80 us, 27-row tiles 55 us, profiles/r06_bih_vector_streams.txt)
    const bool streams = pl.bih_vm != 0;
    auto wg_cost = [](double x) {
        if (x <= 1.0) return 1.0;
        if (x <= 2.0) return 1.15 + 0.10 * x;
        return 1.30 + 0.15 * x;
    };
    int bestRB = 3; double best = 1e300;
    for (int RB = 3; RB <= 192; RB += 3) {
        if (opt.rows_per_tile > 0 && RB != std::max(3, (opt.rows_per_tile / 3) * 3)) continue;
        const int64_t nrb = cdiv(p.yc, RB);
        const int64_t wgs = (int64_t)cdiv((int64_t)nstrip * nrb, 4) * p.nbatch;
        const int n = streams ? 1 : std::min(occ, 3);
        const int64_t cap = 256 * (int64_t)n;
        const int64_t rounds = cdiv(wgs, cap);
        const int64_t w_last = wgs - (rounds - 1) * cap;
        const double cost = ((double)(rounds - 1) * wg_cost((double)n) + wg_cost((double)w_last / 256.0)) * (double)(RB + 11 + 8);
        if (cost < best) { best = cost; bestRB = RB; }
    }
    pl.RY = bestRB;
    pl.nrb = (int)cdiv(p.yc, bestRB);
    pl.nsg = (int)cdiv((int64_t)nstrip * pl.nrb, 4) + 1;
    if (!(opt.flags & XINV_FLAG_NO_TILE_SKIP)) {
        rc = plan_tile_skip(p, pl, ws, st, opt, bestRB);
        if (rc) return rc;
    }
    return XINV_OK;
}

// 9-point forms: 4-colour fused kernel, all coefficient arrays streamed
static int plan_fused9(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    pl.um = pl.umask = 0;
    const int k9max = (p.kind == KIND_STD2D) ? 3 : 2;
    const int k9def = 2;      // bandwidth-bound: 2000x2000 general 0.74 -> 1.24e11, standard 1.07 -> 1.42e11 against K = 1
    pl.K = opt.sweeps_per_launch > 0 ? std::min(opt.sweeps_per_launch, k9max) : k9def;
    pl.aligned = !(p.xc & 1) && vec_aligned(p.S, p.sS);
    for (int q = 0; q < p.ncoef; q++) pl.aligned = pl.aligned && vec_aligned(p.c[q], p.sc[q]);
    if (!rows_per_tile_given(p, opt, pl)) {
        const int occ = plan_occ(p, pl, pl.K);
        // the 9-point kernels stream every coefficient array and sit at the fabric's bandwidth
        // (6+ TB/s): halo re-reads cost more than occupancy gives, so one workgroup per CU
        // (tall tiles) is the target -- measured +25 % (standard, K=1) / +21 % (general) at 2000x2000
        pl.lone = 1.0;
        split_rows_evenly(p, pl, choose_row_blocks(p.yc, cdiv(p.xc, own_cols(p, pl, pl.K)), p.nbatch, pl.K, occ, pl.lone, false));
    }
    pl.nsg = (int)cdiv((int64_t)cdiv(p.xc, own_cols(p, pl, XINV_KMAX)) * pl.nrb, 4) + 1;
    if (pl.even_split && !(opt.flags & XINV_FLAG_NO_TILE_SKIP))
        return plan_tile_skip(p, pl, ws, st, opt);
    return XINV_OK;
}

// 3-D forms: one sweep per launch; cross-sections of NW rows per workgroup (rows_per_tile = NW) marched through the
// planes, k chunks
static int plan_fused3d(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    int rc = XINV_OK;
    pl.K = 1;
    pl.RY = (opt.rows_per_tile == 8 || opt.rows_per_tile == 12 || opt.rows_per_tile == 16)
                ? opt.rows_per_tile : 0;     // 0: decided below, once the variant is known
    pl.nsg = (int)cdiv(p.xc, pl.seam ? xinv_ring_uw(p.xc, 2) : 124);   // x strips (seam: the ring layout's, xinv_tiles.h)
    // only S and the forcing are read as vectors when the coefficients are per-row scalars
    pl.aligned = !(p.xc & 1) && vec_aligned(p.S, p.sS) && vec_aligned(p.c[p.ncoef - 1], p.sc[p.ncoef - 1]);
    if (p.kind == KIND_STD3D) {
        for (int q = 0; q < 3; q++) pl.aligned = pl.aligned && vec_aligned(p.c[q], p.sc[q]);
        pl.umask = 0;
        if (!(opt.flags & XINV_FLAG_NO_XUNIFORM)) {
            const int idx3[3] = {0, 1, 2};
            rc = detect_xuniform_of(p, ws, st, idx3, 3, p.zc * p.yc, &pl.umask);
            if (rc) return rc;
        }
        pl.um = (pl.umask == 7u) ? 7u : 0u;
        // 16 waves x 64 lanes leaves 128 VGPRs per lane: enough only for the x-uniform variant (the others
        // spilled and are not instantiated: a request for sixteen gets twelve)
        const bool nw16_ok = (pl.um == 7u && p.BCy != XINV_BC_EXTEND);
        const bool nw16 = nw16_ok && !pl.seam;            // (seam variants: 8 or 12 wavefronts)
        if (pl.RY == 0) pl.RY = nw16 ? 16 : 12;
        if (pl.RY == 16 && !nw16) pl.RY = 12;
    } else {
        pl.um = pl.umask;                               // 0x7f: A..G are per-row scalars
        if (pl.RY == 0 || pl.RY == 16) pl.RY = 12;      // seven coefficient windows: 12 waves x 170 VGPRs
    }
    pl.nrb = (int)cdiv(p.yc, pl.RY - 4);
    // k chunks: one workgroup per CU is resident (16 / 12 waves); the chunk count that minimises (rounds of 256
    // workgroups) x (planes marched per workgroup): xinv_k_chunks_fused3d
    pl.nkc = xinv_k_chunks_fused3d(p.zc, (int64_t)pl.nsg * pl.nrb * p.nbatch);
    pl.KC = (int)xinv_k_chunk_planes(p.zc, pl.nkc);
    // Two sweeps per pass, x-uniform coefficients, no 'extend': k_pipe3d (the two sweeps pipelined across two
    // groups of eight wavefronts, xinv_pipe3d.h) -- the one-sweep kernel sits at what HBM delivers, so halving the
    // bytes per sweep pays: 15 volumes of 50 x 360 x 720: 2.83e11 against 1.88e11, 2 volumes 1.85 against 1.46,
    // 601 x 300 x 300 2.40 against 1.57 (profiles/r03_pipe3d_first.txt); sweeps_per_launch = 1 keeps the one-sweep
    // kernel.  (Round 2's k_fused3d2, both sweeps inside every wavefront, was bound by its own latency chain
    // -- 1.45e11 -- and is gone.)
    pl.K2 = false;
    const int k2_auto = XINV_ENV_INT("XINV_3D_K2", 1);
    const bool ext3 = (p.BCy == XINV_BC_EXTEND);      // ('extend': the EXT variant -- not with the seam or the contracted arithmetic)
    if (p.kind == KIND_STD3D && pl.um == 7u && !(ext3 && (pl.seam || pl.fma || p3_extend_joff(p.yc) < 0)) && !(pl.seam && (pl.fma || p.xc < 64)) &&
        (opt.sweeps_per_launch == 2 || (opt.sweeps_per_launch == 0 && k2_auto)) &&
        opt.rows_per_tile == 0 && p.stop.mxLoop >= 1 &&
        p.zc * p.yc * 64 < ((int64_t)1 << 31) &&                      // (32-bit offsets into the record table)
        p.zc * p.yc * p.xc * 8 < ((int64_t)1 << 31)) {                // (k_pipe3d addresses a volume through buffer resources: below 2 GiB)
        pl.K2 = true;
        pl.K = 2;
        pl.nsg2 = (int)cdiv(p.xc, pl.seam ? xinv_ring_uw(p.xc, 4) : 120);  // (odd-xc periodic seam: the ring variant's strips, xinv_tiles.h)
        pl.joff2 = ext3 ? p3_extend_joff(p.yc) : 0;
        pl.nrb2 = (int)cdiv(p.yc + pl.joff2, XINV_P3_G * XINV_P3_RR - 8);
        {
            // per-(plane, row) records of the x-uniform coefficients, relaxation factor and predicate: once per solve
            const bool shared = (p.sc[0] == 0 && p.sc[1] == 0 && p.sc[2] == 0);
            const int64_t tab = p.zc * p.yc * 8;
            rc = ensure_dev(&ws->d_rowf, &ws->d_rowf_cap, (size_t)(shared ? 1 : p.nbatch) * tab * sizeof(double));
            if (rc) return rc;
            RowFactor3Args ra;
            memset(&ra, 0, sizeof ra);
            for (int q = 0; q < 3; q++) { ra.c[q] = p.c[q]; ra.sc[q] = p.sc[q]; }
            ra.zc = p.zc; ra.yc = p.yc; ra.xc = p.xc; ra.sc_ = p.sc_;
            ra.rowf = (double *)ws->d_rowf; ra.srowf = shared ? 0 : tab;
            pl.srowf2 = ra.srowf;
            hipLaunchKernelGGL(k_row_factor3d, dim3((unsigned)cdiv(p.zc * p.yc, 256), (unsigned)(shared ? 1 : p.nbatch), 1),
                               dim3(256), 0, st, ra);
        }
        // the cut of the column into k chunks (xinv_p3_whole_tiles: which tiles of a launch are cut is decided per launch):
        // the count that makes the launch of the whole batch cheapest
        pl.nkc2 = xinv_k_chunks_pipe3d(p.zc, (int64_t)pl.nsg2 * pl.nrb2 * p.nbatch, pl.cus);
        pl.KC2 = (int)xinv_k_chunk_planes(p.zc, pl.nkc2);
    }
    return XINV_OK;
}

// ---- 2-D 5-point forms: the steps of plan_fused5, in the order they run ---------------------------------------------------
// which coefficient streams are constant along x (lat-lon grids: functions of latitude)
static int plan5_xuniform(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    const StreamMap &sm = stream_map(p.kind);
    pl.umask = 0;
    ws->act_ready = false;
    if (!(opt.flags & XINV_FLAG_NO_XUNIFORM)) {
        // (the activity map plan_tile_skip will ask for, with the pipelined pass's strips -- what a lat-lon problem
        //  of this size gets --, rides the same host round trip as the detection's flags)
        if (p.kind != KIND_STD2DT && opt.rows_per_tile == 0 && opt.sweeps_per_launch == 0 &&
            !(opt.flags & (XINV_FLAG_NO_TILE_SKIP | XINV_FLAG_NO_PIPE)) && p.nbatch <= 64 &&
            p.nbatch * p.yc * p.xc >= (int64_t)2000000) {
            const int uw_pipe = own_cols(p, pl, XINV_PIPE_P, true);
            if (p.xc >= uw_pipe && p.nbatch * cdiv(p.xc, uw_pipe) * (p.yc + 1) <= (int64_t)50000000) {
                const int rc = issue_strip_active(p, ws, st, uw_pipe, sm.c[sm.forcing]);
                if (rc) return rc;
            }
        }
        const int rc = detect_xuniform_of(p, ws, st, sm.c, sm.nuni, p.yc, &pl.umask);
        if (rc) return rc;
    }
    pl.um = pick_um(p.kind, pl.umask);
    return XINV_OK;
}

// sweeps per pass, and whether they run as the wave-pipelined pass
static int plan5_sweeps(const Problem &p, const xinv_options &opt, Workspace *, hipStream_t st, Plan &pl)
{
    if (opt.sweeps_per_launch > XINV_KMAX) return fail_arg("sweeps_per_launch must be 1 to 4");
    const StreamMap &sm = stream_map(p.kind);
    pl.aligned = !(p.xc & 1) && vec_aligned(p.S, p.sS);
    for (int q = 0; q < sm.n; q++) pl.aligned = pl.aligned && vec_aligned(p.c[sm.c[q]], p.sc[sm.c[q]]);
    // Sweeps per pass over HBM.  Each one costs two more window rows of registers and 2 more
    // halo rows/columns per side, and saves a pass and a launch.  Vector streams per row step
    // (S plus every coefficient array that is not x-uniform) tell the two regimes apart:
    //  - one or two (lat-lon Poisson, Gill-Matsuno): issue-bound, needs two wavefronts per
    //    SIMD.  The standard form still has them at K = 4 (3600x1800: 14.2 / 12.8 / 11.7 us
    //    per sweep for K = 2 / 3 / 4); the general form gains nothing from K = 3 (C4);
    //  - four or more (full coefficient arrays): bandwidth-bound, one workgroup per CU is as
    //    fast as two, so K = 3 pays even at one wavefront per SIMD (2000x2000 general form:
    //    2.20 -> 2.38e11 with A, C, G streamed, 1.53 -> 2.21e11 with all seven; standard form
    //    3600x1800: 2.65 -> 3.9e11), K = 4 does not (one wavefront per SIMD: 3.4e11).
    const int nvec = 1 + sm.n - __builtin_popcount(pl.um & ((1u << sm.n) - 1u));
    pl.lone = nvec <= 2 ? 1.6 : (nvec == 3 ? 1.3 : 1.0);
    // Four sweeps per pass pipelined across the four wavefronts of a workgroup (xinv_pipe2d.h) -- a quarter of
    // the tiles, four times as tall, half the recomputed halo -- for the forms whose coefficients are per-row
    // records: the standard form with per-row A and C (lat-lon Poisson) and the general form with per-row
    // A, C, D, E, F (lat-lon Gill-Matsuno).
    const int pipe_mode = XINV_ENV_INT("XINV_PIPE", 1);
    // (Only the variants whose relaxation factor is a per-row record.  With coefficient arrays that vary along
    // x every wavefront of the pipeline streams them and divides per point: built, bit-exact, and slower than
    // k_fused2d at three sweeps per pass -- C3 Stommel 2.09 against 2.56e11, C2 with every array streamed 2.95
    // against 4.06e11, profiles/r03_pipe_vector_streams.txt -- so those forms stay on k_fused2d.)
    const bool pipe_form = (p.kind == KIND_STD2D && pl.um == 3u) || (p.kind == KIND_GEN2D && pl.um == 0x1fu);
    // At every size (round 3, profiles/r03_pipe_size_crossover.txt).  Until the pass lost a quarter of its
    // instructions per step and the forcing rode the LDS ring, k_fused2d (VALU 96 % busy against ~75 %) won on
    // launches of several rounds of workgroups and the standard form switched at 1e7 points; re-measured on
    // 1 / 2 / 3 / 4 / 8 slices of 3600x1800: 6.17 / 6.76 / 7.25 / 7.21 / 7.72e11 pipelined (forcing through the
    // ring from two slices on) against 5.31 / 6.33 / 6.53 / 6.64 / 7.31e11.  The general form stops at two sweeps
    // per pass on k_fused2d (registers) and is bound by HBM at C4.  XINV_PIPE=3 restores the old crossover.
    const bool pipe_size_ok = pipe_mode != 3 || p.kind == KIND_GEN2D || p.nbatch * p.yc * p.xc <= (int64_t)10000000;
    // (k_pipe2d addresses a slice through buffer resources with signed 32-bit row offsets: slices below 2 GiB)
    const bool pipe_want = pipe_mode != 0 && pipe_form && pipe_size_ok && !(opt.flags & XINV_FLAG_NO_PIPE) &&
                           (opt.sweeps_per_launch == 0 || opt.sweeps_per_launch == XINV_PIPE_P) &&
                           (p.yc + 16) * p.xc * 8 < ((int64_t)1 << 31);
    const bool hoisted_gen = (p.kind == KIND_GEN2D && nvec <= 2);
    const int ksup = (p.kind == KIND_STD2D && nvec <= 2) ? XINV_KMAX : (hoisted_gen ? 2 : 3);
    const int occ_needed = nvec >= 4 ? 1 : 2;
    if (pipe_want)
        pl.K = XINV_PIPE_P;
    else if (opt.sweeps_per_launch > 0)
        pl.K = std::min(opt.sweeps_per_launch, (p.kind == KIND_STD2D) ? XINV_KMAX : 3);
    else {
        pl.K = 2;
        for (int k = ksup; k > 2; k--) {                 // (pl.pipe, pl.pq, pl.alias_ac are still unset: the plain k_fused2d variant)
            bool have = false;
            if (plan_occ(p, pl, k, &have) >= occ_needed && have) { pl.K = k; break; }
        }
    }
    pl.pipe = pipe_want && pl.K == XINV_PIPE_P;
    pl.tpw = pl.pipe ? 1 : 4;
    // the forcing through the LDS ring from the size on at which the later wavefronts' forcing requests cost more than
    // the ring does (xinv_tiles.h: xinv_pipe_forcing_ring; the headline's 155 MB is above it); XINV_PIPE_FR=0|1 forces
    const int fr_env = opt.pipe_fr ? (opt.pipe_fr > 0 ? 1 : 0) : XINV_ENV_INT("XINV_PIPE_FR", -1);
    const bool fr_size = xinv_pipe_forcing_ring(p.nbatch, p.yc, p.xc);
    pl.pipe_fr = pl.pipe && (fr_env < 0 ? fr_size : fr_env != 0);
    return XINV_OK;
}

// Round 5: the general form with A and C varying along x (Stommel with R(x, y), BASELINE configs[2]) reads the
// relaxation factor and the update predicate of every point from one more stream (FusedGen2DQ) instead of dividing
// and testing six operands whenever a row enters a window.  XINV_FLAG_NO_POINT_FACTOR keeps FusedGen2D.
static int plan5_point_factor(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    pl.pq = p.kind == KIND_GEN2D && (pl.um == 0x1cu || pl.um == 0u) && !pl.pipe && !pl.seam && !pl.fma &&
            !(opt.flags & XINV_FLAG_NO_POINT_FACTOR) && p.sc_.optArg != 0.0;
    if (!pl.pq) return XINV_OK;
    // the point-factor stream, once per coefficient stack
    int rc = ensure_dev(&ws->d_pfac, &ws->d_pfac_cap, (size_t)p.nbatch * p.yc * p.xc * sizeof(double));
    if (rc) return rc;
    const StreamMap &sm = stream_map(p.kind);
    PointFactorArgs fa;
    memset(&fa, 0, sizeof fa);
    for (int q = 0; q < sm.n; q++) { fa.c[q] = p.c[sm.c[q]]; fa.sc[q] = p.sc[sm.c[q]]; }
    fa.yc = p.yc; fa.xc = p.xc; fa.n = p.yc * p.xc; fa.sc_ = p.sc_; fa.q = ws->d_pfac; fa.flag = ws->dflag;
    int flag = 0;
    rc = flag_pass(ws, st, &flag, [&] {
        hipLaunchKernelGGL(k_point_factor, dim3((unsigned)std::min<int64_t>(2048, cdiv(fa.n, 256)), (unsigned)p.nbatch, 1),
                           dim3(256), 0, st, fa);
    });
    if (rc) return rc;
    if (flag & 1) pl.pq = false;                     // (a factor of exactly zero somewhere: Q == 0 could not mean "skip")
    pl.alias_ac = pl.pq && !(flag & 2);              // A and C bitwise equal everywhere: C is read out of A
    return XINV_OK;
}

// the pipelined pass's per-row records (the x-uniform streams, the relaxation factor, the row predicate) and its update masks
static int plan5_row_records(const Problem &p, const xinv_options &, Workspace *ws, hipStream_t st, Plan &pl)
{
    if (!pl.pipe) return XINV_OK;
    const StreamMap &sm = stream_map(p.kind);
    const int rw = pipe_rec_shape(p.kind).rw;
    const int rc = ensure_dev(&ws->d_rowf, &ws->d_rowf_cap, (size_t)p.nbatch * p.yc * rw * sizeof(double));
    if (rc) return rc;
    RowFactorArgs ra;
    memset(&ra, 0, sizeof ra);
    for (int q = 0; q < sm.nuni; q++) { ra.c[q] = p.c[sm.c[q]]; ra.sc[q] = p.sc[sm.c[q]]; }      // A, C (, D, E, F)
    ra.gen = p.kind == KIND_GEN2D; ra.um = pl.um; ra.rw = rw;
    ra.yc = p.yc; ra.xc = p.xc; ra.sc_ = p.sc_; ra.rowf = (double *)ws->d_rowf;
    hipLaunchKernelGGL(k_row_factor, dim3(cdiv(p.yc, 256), (unsigned)p.nbatch, 1), dim3(256), 0, st, ra);
    // the march's update masks: the row predicate just written, the launch's lane -> column map, the forcing's mask
    const int nstrip = (int)cdiv(p.xc, own_cols(p, pl, pl.K, true));
    const int rc2 = ensure_dev(&ws->d_pmask, &ws->d_pmask_cap,
                               (size_t)xinv_pipe_mask_count(p.nbatch, nstrip, p.yc) * sizeof(unsigned long long));
    if (rc2) return rc2;
    if (p.masks_by_chunk) return XINV_OK;                // (the forcing of the later chunks is not there yet: roll_join)
    return launch_pipe_masks(p, pl, ws, st, 0, p.nbatch);
}

// Rows per tile (the cost model: xinv_tiles.h).
static int plan5_row_split(const Problem &p, const xinv_options &opt, Workspace *, hipStream_t st, Plan &pl)
{
    if (rows_per_tile_given(p, opt, pl)) return XINV_OK;
    // Tall tiles amortise the 4K recomputed halo rows, but the launch should put the same
    // number of workgroups on every CU: with the K = 2 kernels two workgroups fit per CU
    // (register-limited), so the target is a multiple of 512 workgroups.  Pick the row-block
    // count that minimises (workgroups per CU) x (steps per tile); rows are then split
    // evenly (measured at 3600x1800: 64 blocks of ~28 rows beat 53 blocks of 34).
    const int occ = plan_occ(p, pl, pl.K);         // workgroups of the chosen variant per CU
    // (pl.lone, set with K above: with one or two vector streams a second workgroup per CU
    // fills idle issue slots; with four or more a pair runs no faster than one, and tall
    // tiles (less halo) win -- 2000x2000 general form, A C G streamed: 40-row tiles 38.3 us,
    // 17-row tiles 44.0 us)
    split_rows_evenly(p, pl, choose_row_blocks(p.yc, cdiv(p.xc, own_cols(p, pl, pl.K, pl.pipe)), p.nbatch, pl.K, occ, pl.lone, pl.pipe));
    return XINV_OK;
}

// workgroups per member with the narrowest strips any K uses: sizes the partials
// (the shorter tail / redo passes of a pipelined plan run k_fused2d: four 112-column tiles per workgroup)
static int plan5_partials(const Problem &p, const xinv_options &, Workspace *, hipStream_t, Plan &pl)
{
    pl.nsg = (int)cdiv((int64_t)cdiv(p.xc, own_cols(p, pl, XINV_KMAX, false)) * pl.nrb, 4) + 1;
    if (pl.pipe) pl.nsg = std::max(pl.nsg, (int)cdiv(p.xc, own_cols(p, pl, pl.K, true)) * pl.nrb + 1);
    return XINV_OK;
}

// 2-D 5-point forms: x-uniform streams, sweeps per pass, rows per tile, masked-tile skipping
static int plan_fused5(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    for (auto step : {plan5_xuniform, plan5_sweeps, plan5_point_factor, plan5_row_records, plan5_row_split, plan5_partials}) {
        const int rc = step(p, opt, ws, st, pl);
        if (rc) return rc;
    }
    if (pl.even_split && !(opt.flags & XINV_FLAG_NO_TILE_SKIP)) {
        const int rc = plan_tile_skip(p, pl, ws, st, opt);
        if (rc) return rc;
    }
    return plan_pipe_tile_recs(p, pl, ws, st);           // (no tile skipped: the pipelined pass's records of the final split)
}

// The kernel of every pass length the sweep loops can ask a fused plan for: k = 1 .. pl.K (plan_variant).  A variant no
// unit instantiates fails the plan here (the planner's own caps on K and the cross-section keep a planned solve away from it).
static int plan_kernels(const Problem &p, Plan &pl)
{
    for (int k = 1; k <= pl.K; k++) {
        pl.kern[k] = xinv_kernel(plan_variant(p, pl, k));
        if (pl.kern[k].fn) continue;
        return fail_arg(p.kind == KIND_GEN3D ? "internal: no general 3-D kernel variant for this cross-section"
                      : p.kind == KIND_STD3D ? "internal: no 3-D kernel variant for this cross-section"
                      : pl.nine              ? "unsupported sweeps_per_launch for the 9-point kernel"
                                             : "unsupported sweeps_per_launch for this kernel variant");
    }
    return XINV_OK;
}

// which path, then the tiling of its kernel family
static int plan_path(const Problem &p, const xinv_options &opt, Workspace *ws, hipStream_t st, Plan &pl)
{
    ws->act_ready = false;                               // (an activity map issued ahead belongs to ONE plan: issue_strip_active)
    int rc = XINV_OK;
    // ---- path ------------------------------------------------------------------------------
    // (the odd-xc periodic seam runs inside the 2-D 5-point streaming kernels -- xinv_fused.h: SEAM -- when a strip
    //  spans at most three wraps of the row: xc >= 64; the 3-D, 9-point and biharmonic forms keep the colour launches)
    const bool seam5_ok = !pl.seam || p.xc >= 64;        // (3-D forms: the SEAM variants of k_fused3d / k_fused3dg)
    const bool fused5_ok = pl.base == 2 && seam5_ok && p.kind != KIND_BIH2D && p.kind != KIND_GEN3D;
    const bool fused9_ok = pl.base == 4 && seam5_ok && p.c[1] &&      // (seam: k_fused9's SEAM variants)
                           (p.kind == KIND_STD2D || p.kind == KIND_GEN2D);
    // biharmonic: the one-pass kernel needs A..I as per-row scalars (and xc % 3 == 0 when periodic)
    bool fusedbih_ok = false;
    if (p.kind == KIND_BIH2D) {
        pl.umask = 0;
        if (!(opt.flags & XINV_FLAG_NO_XUNIFORM)) {
            const int idx10[10] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
            rc = detect_xuniform_of(p, ws, st, idx10, 10, p.yc, &pl.umask);
            if (rc) return rc;
        }
        pl.um = pl.umask;
        // (coefficients that vary along x: the vector-stream variants of the one-pass kernel, xinv_fusedbih.h)
        fusedbih_ok = (p.BCx != XINV_BC_PERIODIC || p.xc % 3 == 0) && !(opt.flags & XINV_FLAG_NO_XUNIFORM) &&
                      p.sc_.optArg != 0.0;
    }
    // general 3-D: the fused kernel exists for x-uniform coefficients only (every 3DOcean array)
    bool fused3g_ok = false;
    if (p.kind == KIND_GEN3D && seam5_ok && opt.path != XINV_PATH_COLOUR && !(opt.flags & XINV_FLAG_NO_XUNIFORM)) {
        const int idx7[7] = {0, 1, 2, 3, 4, 5, 6};
        rc = detect_xuniform_of(p, ws, st, idx7, 7, p.zc * p.yc, &pl.umask);
        if (rc) return rc;
        fused3g_ok = (pl.umask == 0x7fu);
    }
    const bool fused_ok = fused5_ok || fused9_ok || fused3g_ok || fusedbih_ok;
    pl.path = XINV_PATH_COLOUR;
    pl.nine = false;
    if (fused_ok && opt.path != XINV_PATH_COLOUR) { pl.path = XINV_PATH_FUSED; pl.nine = fused9_ok && !fused5_ok; }
    if (opt.path == XINV_PATH_FUSED && !fused_ok)
        return fail_arg("no fused kernel for this form (odd-xc periodic seam with xc < 64; 9-point test form; biharmonic with periodic x and xc % 3 != 0; general 3-D with coefficients that vary along x)");
    if (pl.path == XINV_PATH_COLOUR && !is3d(p.kind) && !p.c[1] && pl.base == 4)
        return fail_arg("internal: 9-point form without B");

    if (pl.path != XINV_PATH_FUSED) return XINV_OK;
    if (p.kind == KIND_BIH2D) return plan_fusedbih(p, opt, ws, st, pl);
    if (pl.nine) return plan_fused9(p, opt, ws, st, pl);
    if (is3d(p.kind)) return plan_fused3d(p, opt, ws, st, pl);
    return plan_fused5(p, opt, ws, st, pl);
}

