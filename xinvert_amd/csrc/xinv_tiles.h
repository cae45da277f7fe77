// xinv_tiles.h -- tile ids of the 2-D streaming kernels (k_fused2d / k_pipe2d), the dispatch order of seam launches and the
// planner's tiling cost models:
// integer arithmetic shared by the kernels and the planner (xinv_launch.h), and compiled on its own by the CPU suite
// (tests/test_tiles.py builds tests/csrc/tiles_check.cpp with g++ against this header; tests/test_pipe_tile_record.py the
// check of k_pipe2d's tile records and the lane -> column maps).
#pragma once
#include <cstdint>
#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

// Tile id -> strip and owned rows [y0, y1): row block rb = id / nstrip of strip id % nstrip (fixed height RY, or RY == 0:
// the yc rows split evenly, boundaries rounded to even rows).
struct TileRows { int strip; int64_t y0, y1; };
__host__ __device__ inline TileRows xinv_tile_rows(int wt, int nstrip, int nrb, int64_t yc, int RY)
{
    TileRows t;
    const int rb = wt / nstrip;
    t.strip = wt - rb * nstrip;
    if (RY > 0) { t.y0 = (int64_t)rb * RY; t.y1 = (t.y0 + RY < yc) ? t.y0 + RY : yc; }
    else {
        t.y0 = (((int64_t)rb * yc) / nrb) & ~(int64_t)1;
        t.y1 = (rb + 1 == nrb) ? yc : ((((int64_t)(rb + 1) * yc) / nrb) & ~(int64_t)1);
    }
    return t;
}

// Dispatch order of a seam launch (periodic x, odd xc).  The edge strips' tiles -- the ones that hold the seam: an extra pass
// in every other half-sweep -- are the slow ones and the launch ends with the last of them: they go FIRST, spread over the
// XCDs (round 4 cut their row blocks in pieces instead, whose ids at the end of the id space the chunk mapping handed to
// the one XCD dispatched last: profiles/r05_seam_rates.txt; whole row blocks, dispatched first, are faster).
// xinv_heavy_first: dispatch position L of `n` (blockIdx.x: XCD L & 7, round L >> 3) -> index in a sequence whose first
// `nh` entries are the heavy ones: rounds below nh / 8 take them eight at a time, the rest keeps the contiguous range per
// XCD of the plain mapping.  A bijection of [0, n).
__host__ __device__ inline int xinv_heavy_first(int L, int n, int nh)
{
    const int hq = (nh < n ? nh : n) >> 3, xcd = L & 7, idx = L >> 3;
    if (idx < hq) return idx * 8 + xcd;
    const int nr = n - 8 * hq, q = nr >> 3, rem = nr & 7;
    return 8 * hq + xcd * q + (xcd < rem ? xcd : rem) + (idx - hq);
}
// xinv_seam_tile: index in the heavy-first sequence -> tile id (heavy: the tiles of the last strip, then of strip 0, row
// block fastest; light: the other strips' tiles in id order).
__host__ __device__ inline int xinv_seam_tile(int s, int nstrip, int nrb)
{
    const int edges = nstrip == 1 ? 1 : 2, nh = edges * nrb;
    if (s < nh) {
        const int e = s / nrb, rb = s - e * nrb;
        return rb * nstrip + (e == 0 ? nstrip - 1 : 0);
    }
    const int k = s - nh, nl = nstrip > edges ? nstrip - edges : 1, rb = k / nl;
    return rb * nstrip + (k - rb * nl) + 1;
}

// Strips of the even-ring layout of the odd-xc periodic seam (xinv_fused.h: RING; H = halo columns a side the kernel needs
// without a seam).  A halo that holds the seam needs a column pair more: on the west because the phantom column takes a
// slot, on the east because information crosses the seam one pair faster.
//   symmetric:  every strip H + 2 | 128 - 2H - 4 owned | H + 2;
//   asymmetric: strip 0 -- its west halo wraps -- H + 2 | 128 - 2H - 2 | H, every other strip H | 128 - 2H - 2 | H + 2: valid
//               when no strip's halos hold the seam on both sides, i.e. strip 0's east halo -- H slots -- holds column xc-1
//               at most as its outermost slot (a column xc-1 further in is updated with the NEW column 0, which such a
//               halo does not hold: it would go stale two half-sweeps early): xc >= 128 - 2H - 2 + H; there are then at
//               least two strips.  3601 columns are then 33 strips of the pipelined pass, as 3600 are (34 symmetric).
// The kernels and the planner both call these with the kernel's H: no argument travels.
__host__ __device__ inline bool xinv_ring_asym(int64_t xc, int H) { return xc >= (int64_t)(128 - 2 * H - 2) + H; }
__host__ __device__ inline int xinv_ring_uw(int64_t xc, int H) { return 128 - 2 * H - (xinv_ring_asym(xc, H) ? 2 : 4); }
__host__ __device__ inline int xinv_ring_hw(int64_t xc, int H, int strip)      // west halo of a strip
{
    return xinv_ring_asym(xc, H) ? (strip == 0 ? H + 2 : H) : H + 2;
}

// ---- k_pipe3d (xinv_pipe3d.h): a FLAT grid over the members of a launch, one workgroup per CU -----------------------------
// Dispatch slot L of a launch -> which tile of which member, which planes.  With g the tile's index in the launch
// (member-major; a member has NT tiles), the slots below nfull march tile g = L through the WHOLE column; the tiles behind
// them are cut into nkc chunks: slot nfull + q marches chunk q % nkc of tile nfull + q / nkc.  `reducer`: the slot is the
// member's last in dispatch order (it adds the member's norm partials: every other slot of the member is resident or
// finished by then).  Whole-column slots take the member's tiles in an XCD-aware order: slot L lands on XCD L & 7, and the
// member's slots of one XCD take a contiguous band of its tiles -- Tj = rank of (L & 7, L) among the member's whole-column
// slots [L0, L0 + n) (with L0 a multiple of 8: xcd * (n / 8) + min(xcd, n % 8) + (L - L0) / 8).
// (Three pieces, so that the kernel can place them around its early exit; xinv_p3_slot puts them together.)
__host__ __device__ inline int xinv_p3_slot_tile(int L, int nfull, int nkc, int &kc)       // -> g; kc: the chunk (0 for a whole column)
{
    int g;                                               // tile index in the launch, member-major
    kc = 0;
    if (L < nfull) g = L;
    else { const int q = L - nfull; g = nfull + q / nkc; kc = q - (g - nfull) * nkc; }
    return g;
}
__host__ __device__ inline bool xinv_p3_slot_reduces(int L, int nfull, int nkc, int NT, int ml)
{
    const int gl = (ml + 1) * NT - 1;                    // the member's last tile
    return (gl < nfull) ? (L == gl) : (L == nfull + (gl - nfull) * nkc + nkc - 1);
}
__host__ __device__ inline int xinv_p3_slot_member_tile(int L, int nfull, int NT, int ml, int g)
{
    if (L < nfull) {
        const int L0 = ml * NT;
        const int n = (L0 + NT <= nfull) ? NT : (nfull - L0);                 // (the member's whole-column slots)
        const int xcd = L & 7;
        auto below = [](int e, int x) { return (e >> 3) * x + ((e & 7) < x ? (e & 7) : x); };       // v in [0, e): (v & 7) < x
        auto same = [](int e, int x) { return e <= x ? 0 : ((e - x + 7) >> 3); };                   // v in [0, e): (v & 7) == x
        return (below(L0 + n, xcd) - below(L0, xcd)) + (same(L, xcd) - same(L0, xcd));
    }
    return g - ml * NT;
}
struct P3Slot { int ml, Tj, kc; bool whole, reducer; };
__host__ __device__ inline P3Slot xinv_p3_slot(int L, int nfull, int nkc, int NT)
{
    P3Slot s;
    s.whole = L < nfull;
    const int g = xinv_p3_slot_tile(L, nfull, nkc, s.kc);
    s.ml = g / NT;
    s.reducer = xinv_p3_slot_reduces(L, nfull, nkc, NT, s.ml);
    s.Tj = xinv_p3_slot_member_tile(L, nfull, NT, s.ml, g);
    return s;
}

// How many tiles of a launch march the whole column (they come first).  One workgroup per CU: `tiles` tiles take
// ceil(tiles / cus) rounds of a whole march -- and when the last round holds only a few tiles (15 volumes of 50 x 360 x 720 on
// 256 CUs: 2070 tiles, 8.09 rounds) they march alone while the other CUs idle.  The plan fixes a cut of the column into nk
// chunks of KC planes; per launch: none of the tiles is cut, all are (small batches: more workgroups than tiles), or the
// remainder of the last round -- pieces that start together when the whole-column rounds end and finish in a fraction of a
// march.  Costs in pipeline steps: a whole march zc + 4, a chunk KC + 14 (four halo planes a side and the pipeline's fill).
// cus < 0: -cus compute units, never the remainder cut (xinv_options.cu_count = -1: A/B comparisons).
__host__ inline int64_t xinv_p3_whole_tiles(int64_t tiles, int nk, int64_t KC, int64_t zc, int cus_, double *cost_out = nullptr)
{
    const bool no_rem = cus_ < 0;
    const int64_t cus = cus_ < 0 ? -cus_ : cus_;
    auto cdiv64 = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    const double cf = (double)(zc + 4), cs = (double)(KC + 14);
    double best = (double)cdiv64(tiles, cus) * cf;
    int64_t nfull = tiles;
    if (nk > 1) {
        const double call = (double)cdiv64(tiles * nk, cus) * cs;
        if (call < best * 0.97) { best = call; nfull = 0; }
        const int64_t r = tiles % cus, R = tiles / cus;
        if (r && R && !no_rem) {
            const double crem = (double)R * cf + (double)cdiv64(r * nk, cus) * cs;
            if (crem < best * 0.985) { best = crem; nfull = tiles - r; }
        }
    }
    if (cost_out) *cost_out = best;
    return nfull;
}

// BCy = 'extend' on k_pipe3d (EXT): the second sweep's pre-pass is applied out of a wavefront's own registers, so rows 0 / 1
// and rows yc-2 / yc-1 each have to sit in ONE wavefront (RR adjacent rows each; the cross-section of row block jb starts at
// row jb * RJ - H - joff) -- the first pair in block 0, the second in the block that owns row yc-1 and in the block before
// it when that one owns row yc-2 or yc-3, whose second sweep reads row yc-1 through row yc-2.  xinv_p3_extend_joff: the
// shift of the row blocks that achieves it -- 0 for five row counts in eight, 2 for the others (-1: none; not reached).
__host__ __device__ inline bool xinv_p3_extend_ok(int64_t yc, int joff, int RJ, int H, int RR)
{
    if ((H + joff) % RR == RR - 1) return false;                   // row 0 would be a wavefront's last row
    const int64_t jbo = (yc - 1 + joff) / RJ;                      // the block that owns row yc-1
    auto together = [&](int64_t jb) { return ((yc - 2) - (jb * RJ - H - joff)) % RR != RR - 1; };   // row yc-2 is not a wavefront's last row
    if (!together(jbo)) return false;
    if (jbo > 0 && (yc - 1 + joff) - jbo * RJ <= 1 && !together(jbo - 1)) return false;
    return true;
}
__host__ __device__ inline int xinv_p3_extend_joff(int64_t yc, int RJ, int H, int RR)
{
    return xinv_p3_extend_ok(yc, 0, RJ, H, RR) ? 0 : (xinv_p3_extend_ok(yc, 2, RJ, H, RR) ? 2 : -1);
}

// ---- k_pipe2d (xinv_pipe2d.h): the schedule of the wave-pipelined pass ----------------------------------------------------
// The ONE definition of who marches which rows at which global step of the workgroup: the kernel, the planner's step count
// and the CPU simulation (tests/csrc/pipe_schedule_check.cpp) all call these.  Four wavefronts, wavefront pw applies sweep
// pw + 1 to a tile of ry owned rows [yu0, yu0 + ry); rows are relative to yu0, `lag` = steps wavefront pw + 1 runs behind
// wavefront pw, a barrier closes every b-th global step (step g is in barrier interval g / b), `period` = the unroll
// period of that wavefront's march (a march is whole periods).
//   needed rows     wavefront pw must enter the n = ry + 16 - 4 pw rows [-8 + 2 pw, ry + 7 - 2 pw], the first of them in
//                   global step lag * pw (a row enters wavefront pw + 1 `lag` steps after it entered wavefront pw);
//   padding         the march is rounded up to whole periods: pad = -n mod period extra rows.  Wavefront 0 cannot start
//                   before step 0 and is never the last to finish: its padding stays at the end.  Wavefronts 1..3 start
//                   EARLIER instead, in the pipeline's fill where their SIMD has nothing else to do: `front` rows above
//                   the first needed one -- the largest even count (the colour of a row is compile-time in the unrolled
//                   march) that the padding and the start allow -- and only pad - front <= 1 rows stay behind the last;
//   ring slots      a wavefront names the LDS ring slot of a row at compile time from the row's position in ITS march,
//                   (row - first row + 2 pw) mod 4, which is (row + 8 + front) mod 4: a wavefront whose front padding is
//                   2 mod 4 flips bit 1 of the slot (xinv_pipe_slot_flip; a second base address, no instruction), and
//                   every wavefront then finds row r in slot (r + 8) mod 4 whatever the others' padding.
// A padded step is a full step -- loads (clamped to the slice), ring read, two half-sweeps, ring write, barrier -- on rows
// nothing kept depends on (xinv_pipe2d.h: the header comment has the argument).
__host__ __device__ inline int xinv_pipe_rows(int ry, int pw) { return ry + 16 - 4 * pw; }
__host__ __device__ inline int xinv_pipe_pad(int ry, int pw, int period)
{
    return (period - xinv_pipe_rows(ry, pw) % period) % period;
}
__host__ __device__ inline int xinv_pipe_front(int ry, int pw, int lag, int period)
{
    const int pad = xinv_pipe_pad(ry, pw, period), room = lag * pw;
    return (pad < room ? pad : room) & ~1;
}
__host__ __device__ inline int xinv_pipe_end(int ry, int pw, int lag, int period)
{
    return xinv_pipe_pad(ry, pw, period) - xinv_pipe_front(ry, pw, lag, period);
}
// first row the wavefront marches (relative to yu0) and the global step in which it enters
__host__ __device__ inline int xinv_pipe_first_row(int ry, int pw, int lag, int period)
{
    return -8 + 2 * pw - xinv_pipe_front(ry, pw, lag, period);
}
__host__ __device__ inline int xinv_pipe_start(int ry, int pw, int lag, int period)
{
    return lag * pw - xinv_pipe_front(ry, pw, lag, period);
}
// Global step of the wavefront's first ring read (pw > 0).  Every row is taken out of the ring one step before it enters,
// the first marched row therefore in step start - 1, before the barrier that may close that step; -1: the wavefront starts
// in step 0 and its first read is row first + 1 in step 0 (the first marched row is then padding and stays zero).
__host__ __device__ inline int xinv_pipe_first_read(int ry, int pw, int lag, int period)
{
    return xinv_pipe_start(ry, pw, lag, period) - 1;
}
__host__ __device__ inline int xinv_pipe_slot_flip(int front) { return front & 2; }
// global steps every wavefront of the tile goes through: the longest of the four schedules, whole barrier periods
// (period0: wavefront 0's unroll period, period: the others')
__host__ __device__ inline int xinv_pipe_gtot(int ry, int lag, int b, int period0, int period)
{
    int gtot = 0;
    for (int pw = 0; pw < 4; pw++) {
        const int per = pw == 0 ? period0 : period;
        const int g = xinv_pipe_start(ry, pw, lag, per) + xinv_pipe_rows(ry, pw) + xinv_pipe_pad(ry, pw, per);
        gtot = g > gtot ? g : gtot;
    }
    return ((gtot + b - 1) / b) * b;
}

// The update masks of the pipelined pass (k_pipe_masks builds the table once per plan, the march reads it through the
// scalar unit): one record per member, strip and row, two 64-bit lane masks {mx, my} -- bit i: lane i's .x / .y point of
// that row may be updated (column, row and `forcing defined`).  Index in 64-bit words; rows 0 and yc-1 hold zero words.
#define XINV_PIPE_MASK_WORDS 2
__host__ __device__ inline int64_t xinv_pipe_mask_count(int64_t nbatch, int nstrip, int64_t yc)
{
    return nbatch * nstrip * yc * XINV_PIPE_MASK_WORDS;
}
__host__ __device__ inline int64_t xinv_pipe_mask_index(int64_t m, int nstrip, int strip, int64_t yc, int64_t row)
{
    return ((m * nstrip + strip) * yc + row) * XINV_PIPE_MASK_WORDS;
}

// ---- lane -> column maps of the 2-D streaming kernels (k_fused2d, k_pipe2d, k_pipe_masks) ---------------------------------
// Host-callable: the builder of k_pipe2d's tile records below is checked against them on the CPU
// (tests/csrc/pipe_tile_record_check.cpp).
#define XINV_HD_INLINE __host__ __device__ inline __attribute__((always_inline))
struct LaneCols {
    int64_t l0, l1;            // load columns of .x / .y (wrapped or clamped)
    bool ok_x, ok_y;           // column may be updated (interior, or any column when periodic)
    bool use_x, use_y;         // column is owned (stored / counted) by this lane
    int cls_x, cls_y;          // extend fix: 0 none, 1 straight copy, 2 column 0, 3 column xc-1
};

// Lane -> column map of one wavefront's strip: lane owns columns c0 = xu0 - H + 2*lane and c0+1.
template <bool AL>
XINV_HD_INLINE LaneCols make_lanecols(int64_t xu0, int H, int UW, int lane, int64_t xc, bool per)
{
    LaneCols lc;
    const int64_t c0 = xu0 - H + 2 * lane, c1 = c0 + 1;
    if (per) {
        int64_t w0 = c0 % xc; if (w0 < 0) w0 += xc;
        int64_t w1 = c1 % xc; if (w1 < 0) w1 += xc;
        lc.l0 = w0; lc.l1 = w1;
        lc.ok_x = lc.ok_y = true;
        lc.cls_x = lc.cls_y = 1;
    } else {
        if (AL) {
            int64_t p = c0 < 0 ? 0 : (c0 > xc - 2 ? xc - 2 : c0);
            lc.l0 = p; lc.l1 = p + 1;
        } else {
            lc.l0 = c0 < 0 ? 0 : (c0 > xc - 1 ? xc - 1 : c0);
            lc.l1 = c1 < 0 ? 0 : (c1 > xc - 1 ? xc - 1 : c1);
        }
        lc.ok_x = (c0 >= 1 && c0 <= xc - 2);
        lc.ok_y = (c1 >= 1 && c1 <= xc - 2);
        lc.cls_x = lc.ok_x ? 1 : (c0 == 0 ? 2 : (c0 == xc - 1 ? 3 : 0));
        lc.cls_y = lc.ok_y ? 1 : (c1 == xc - 1 ? 3 : 0);
    }
    lc.use_x = (c0 >= xu0 && c0 < xu0 + UW && c0 < xc);
    lc.use_y = (c1 >= xu0 && c1 < xu0 + UW && c1 < xc);
    return lc;
}

// The same for the even ring of the odd-xc periodic seam (xinv_fused.h: RING; make_lanecols_ring there adds the wave's
// mask of seam lanes).  seam_lane: the lane's .x slot holds column xc-1.
XINV_HD_INLINE LaneCols xinv_lanecols_ring(int64_t xu0, int HW, int UW, int lane, int64_t xc, bool &seam_lane)
{
    LaneCols lc;
    const int64_t c0 = xu0 - HW + 2 * lane, c1 = c0 + 1, xv = xc + 1;
    int64_t w0 = c0 % xv; if (w0 < 0) w0 += xv;              // (even: never P)
    int64_t w1 = c1 % xv; if (w1 < 0) w1 += xv;
    lc.l0 = w0; lc.l1 = (w1 == xc) ? xc - 1 : w1;
    lc.ok_x = true; lc.ok_y = (w1 != xc);
    lc.cls_x = lc.cls_y = 1;
    lc.use_x = (c0 >= xu0 && c0 < xu0 + UW && c0 < xc);
    lc.use_y = (c1 >= xu0 && c1 < xu0 + UW && c1 < xc);
    seam_lane = (w0 == xc - 1);
    return lc;
}

// ---- k_pipe2d: one record per tile, built with the plan ---------------------------------------------------------------------
// Tile -> (strip, rows), the steps of its march and the origin of its lane map are functions of the plan; the kernel used
// to derive them in every workgroup of every launch (an integer division for the strip, two 64-bit ones for the even row
// split, two 64-bit modulos per lane for the wrapped columns).  The planner builds them once, one
// 32-byte record per dispatch slot T of a member (the slot's entry of the tile list when fully masked tiles are skipped,
// the identity -- or the seam launch's heavy-first order -- otherwise), and the kernel takes its record with one scalar load.
struct PipeTileRec {
    int wt;                    // tile id (xinv_tile_rows); -1: an idle slot (the member has fewer active tiles than slots)
    int strip;
    int yu0, yu1;              // owned rows [yu0, yu1)
    int gtot;                  // global steps of the tile's march (xinv_pipe_gtot)
    int c0;                    // column of lane 0's .x slot, unwrapped: first owned column - west halo (negative in strip 0)
    int w0;                    // ... wrapped into the row [0, xc) (periodic x), into the even ring [0, xc + 1) (seam); else c0
    int xu0;                   // first owned column
};
static_assert(sizeof(PipeTileRec) == 32, "one s_load_dwordx8");
// the kernel's constants the records depend on (xinv_pipe2d.h: XINV_PIPE_*)
struct PipeTileGeom { int H, UW, lag, b, period0, period; };

// `seam`: the ring layout's strips (H + 2 / H west halo, xinv_ring_*); `per`: periodic x (always with seam).
// wt < 0: the idle record -- tile 0's geometry (every field a valid one: the kernel forms addresses from it before it looks
// at wt), wt = -1.
__host__ __device__ inline PipeTileRec xinv_pipe_tile_rec(int wt, int nstrip, int nrb, int64_t yc, int RY, int64_t xc, bool per,
                                                          bool seam, const PipeTileGeom &g)
{
    PipeTileRec r;
    const TileRows t = xinv_tile_rows(wt < 0 ? 0 : wt, nstrip, nrb, yc, RY);
    r.wt = wt < 0 ? -1 : wt;
    r.strip = t.strip;
    r.yu0 = (int)t.y0; r.yu1 = (int)t.y1;
    r.gtot = xinv_pipe_gtot(r.yu1 - r.yu0, g.lag, g.b, g.period0, g.period);
    const int UW = seam ? xinv_ring_uw(xc, g.H) : g.UW, HW = seam ? xinv_ring_hw(xc, g.H, t.strip) : g.H;
    const int64_t xu0 = (int64_t)t.strip * UW, c0 = xu0 - HW;
    r.xu0 = (int)xu0; r.c0 = (int)c0;
    if (seam || per) {
        const int64_t xv = seam ? xc + 1 : xc;
        int64_t w = c0 % xv; if (w < 0) w += xv;
        r.w0 = (int)w;
    } else r.w0 = (int)c0;
    return r;
}

// column `w0 + 2 lane` of a lane, wrapped into [0, n): w0 < n and 2 lane <= 126, so a row of 128 columns or more wraps
// once at the most (an add and a conditional subtract); shorter rows take the 32-bit remainder
XINV_HD_INLINE int xinv_wrap_lane_col(int w0, int lane, int n)
{
    int w = w0 + 2 * lane;
    if (n >= 128) return w >= n ? w - n : w;
    return (int)((unsigned)w % (unsigned)n);
}
// make_lanecols from the tile's record: the same map, field for field
template <bool AL>
XINV_HD_INLINE LaneCols xinv_lanecols_rec(const PipeTileRec &r, int UW, int lane, int xc, bool per)
{
    LaneCols lc;
    const int c0 = r.c0 + 2 * lane, c1 = c0 + 1;
    if (per) {
        const int w0 = xinv_wrap_lane_col(r.w0, lane, xc), w1 = (w0 + 1 == xc) ? 0 : w0 + 1;
        lc.l0 = w0; lc.l1 = w1;
        lc.ok_x = lc.ok_y = true;
        lc.cls_x = lc.cls_y = 1;
    } else {
        if (AL) {
            const int p = c0 < 0 ? 0 : (c0 > xc - 2 ? xc - 2 : c0);
            lc.l0 = p; lc.l1 = p + 1;
        } else {
            lc.l0 = c0 < 0 ? 0 : (c0 > xc - 1 ? xc - 1 : c0);
            lc.l1 = c1 < 0 ? 0 : (c1 > xc - 1 ? xc - 1 : c1);
        }
        lc.ok_x = (c0 >= 1 && c0 <= xc - 2);
        lc.ok_y = (c1 >= 1 && c1 <= xc - 2);
        lc.cls_x = lc.ok_x ? 1 : (c0 == 0 ? 2 : (c0 == xc - 1 ? 3 : 0));
        lc.cls_y = lc.ok_y ? 1 : (c1 == xc - 1 ? 3 : 0);
    }
    lc.use_x = (c0 >= r.xu0 && c0 < r.xu0 + UW && c0 < xc);
    lc.use_y = (c1 >= r.xu0 && c1 < r.xu0 + UW && c1 < xc);
    return lc;
}
// xinv_lanecols_ring from the tile's record
XINV_HD_INLINE LaneCols xinv_lanecols_ring_rec(const PipeTileRec &r, int UW, int lane, int xc, bool &seam_lane)
{
    LaneCols lc;
    const int c0 = r.c0 + 2 * lane, c1 = c0 + 1, xv = xc + 1;
    const int w0 = xinv_wrap_lane_col(r.w0, lane, xv), w1 = (w0 + 1 == xv) ? 0 : w0 + 1;
    lc.l0 = w0; lc.l1 = (w1 == xc) ? xc - 1 : w1;
    lc.ok_x = true; lc.ok_y = (w1 != xc);
    lc.cls_x = lc.cls_y = 1;
    lc.use_x = (c0 >= r.xu0 && c0 < r.xu0 + UW && c0 < xc);
    lc.use_y = (c1 >= r.xu0 && c1 < r.xu0 + UW && c1 < xc);
    seam_lane = (w0 == xc - 1);
    return lc;
}

// Dispatch slot T of a launch of NB workgroups <- blockIdx.x = L: workgroup L lands on XCD L & 7, and an XCD's workgroups
// take a contiguous range of slots (the kernel's arithmetic; a bijection of [0, NB))
__host__ __device__ inline int xinv_pipe_slot(int L, int NB)
{
    const int q = NB >> 3, rem = NB & 7, xcd = L & 7, idx = L >> 3;
    return xcd * q + (xcd < rem ? xcd : rem) + idx;
}
// The records of a launch WITHOUT a tile list: NB = nstrip * nrb slots, every tile active.  Slot T holds tile T -- or, in
// a seam launch, the tile of the heavy-first order (the edge strips' tiles dispatched first: xinv_heavy_first /
// xinv_seam_tile of the workgroup's dispatch position).
__host__ inline void xinv_pipe_identity_recs(PipeTileRec *out, int nstrip, int nrb, int64_t yc, int RY, int64_t xc, bool per,
                                             bool seam, const PipeTileGeom &g)
{
    const int NB = nstrip * nrb;
    for (int L = 0; L < NB; L++) {
        const int T = xinv_pipe_slot(L, NB);
        const int wt = seam ? xinv_seam_tile(xinv_heavy_first(L, NB, (nstrip == 1 ? 1 : 2) * nrb), nstrip, nrb) : T;
        out[T] = xinv_pipe_tile_rec(wt, nstrip, nrb, yc, RY, xc, per, seam, g);
    }
}

// ---- the planner's cost models (host only; pure integer / double arithmetic, checked on the CPU) --------------------------
__host__ inline int64_t xinv_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// k_pipe2d: does the forcing row ride the LDS ring behind S (FR: wavefront 0 reads it once, wavefronts 1..3 take it out
// of LDS), or does every wavefront ask the memory system for it?  Decided by the bytes the launch streams -- S read, S
// written and the forcing, 24 B per point of every member.  Beyond the caches the later wavefronts' requests go back to
// HBM, and FR wins by 10-20 % (profiles/r03_pipe_size_crossover.txt: the round-3 switch, 200 MB).  But their requests
// cost time when they HIT as well: with them compiled out the headline launch is 2.7 us shorter, and FR, which trades the
// three buffer loads of a workgroup's step for three LDS writes and reads, takes 0.4-1.0 us of that back at 155 MB, 3-5 %
// of the launch at 100-200 MB (four and eight Gill-Matsuno members); at 39 MB and below, where the tiles are short and
// few workgroups share a CU, the larger ring loses 0-2.5 % (profiles/pipe2d_norm_wave.txt).  The switch sits between
// the two measured sides.
#define XINV_PIPE_FR_BYTES 8.0e7
__host__ inline bool xinv_pipe_forcing_ring(int64_t nbatch, int64_t yc, int64_t xc)
{
    return (double)nbatch * (double)yc * (double)xc * 24.0 > XINV_PIPE_FR_BYTES;
}

// The tallest tile of the even split of yc rows into nrb blocks (xinv_tile_rows with RY == 0: boundaries at
// floor(k yc / nrb) rounded down to even rows, the last block ends at yc), in closed form: with yc = 2 nrb q + s the
// boundaries are 2 (k q + floor(k s / (2 nrb))); a block before the last has 2 q rows, or 2 q + 2 when the fraction
// carries somewhere below the last boundary; the last block takes what is left.
__host__ inline int64_t xinv_even_split_tallest(int64_t yc, int64_t nrb)
{
    const int64_t D = 2 * nrb, q = yc / D, s = yc - q * D;
    const int64_t last = 2 * (q + s / 2 - ((nrb - 1) * s) / D) + (s & 1);
    const int64_t inner = nrb > 1 ? 2 * (q + ((nrb - 1) * s >= D ? 1 : 0)) : 0;
    return last > inner ? last : inner;
}

// Cost of a fused 2-D launch of `wgs` workgroups whose tiles own `rows` rows, in (workgroups per CU) x (steps per tile)
// units: the model behind xinv_choose_row_blocks, shared with the masked-tile planner.  `occ` workgroups of the variant
// fit per CU (register-limited, queried from the runtime), of which the model counts at most `occ_cap`.
// `pipe_lag` > 0: the wave-pipelined pass (k_pipe2d: one tile per workgroup; pipe_lag = steps wavefront p+1 runs behind
// wavefront p -- the last wavefront starts 3 x pipe_lag steps late and enters rows + 4 rows); 0: k_fused2d / k_fused9 at K
// sweeps per pass.
// `pipe_b` > 0 (with pipe_lag > 0; the kernel's steps per barrier): `rows` is the height of the TALLEST tile of the split
// -- the launch ends with it -- and the steps are exactly the ones the kernel runs for it, xinv_pipe_gtot with the
// kernel's unroll periods (pipe_per0: wavefront 0's, pipe_per: the others'; rows in flight + 4).
// pipe_b == 0 keeps the estimate this model had before the schedule was shared -- `rows` the average height, one row added
// for the even rounding, rounded up to 8 in one go -- for the plans recorded from it (tests/csrc/tiles_check.cpp).
__host__ inline int64_t xinv_tile_steps(int64_t rows, int K, int pipe_lag, int pipe_b = 0, int pipe_per0 = 8, int pipe_per = 8)
{
    if (pipe_lag > 0 && pipe_b > 0) return xinv_pipe_gtot((int)rows, pipe_lag, pipe_b, pipe_per0, pipe_per);
    const int64_t period = 2 * K + 2;
    return pipe_lag > 0 ? xinv_cdiv(rows + 1 + 4 + 3 * pipe_lag, 8) * 8 : xinv_cdiv(rows + 1 + 4 * K, period) * period;
}
__host__ inline double xinv_tile_cost(int64_t wgs, int64_t rows, int K, int occ, int occ_cap, double lone, int pipe_lag,
                                      int pipe_b = 0, int pipe_per0 = 8, int pipe_per = 8)
{
    const bool pipe = pipe_lag > 0;
    occ = occ < occ_cap ? occ : occ_cap;
    occ = occ > 1 ? occ : 1;
    const int64_t cap = 256 * (int64_t)occ;
    const int64_t steps = xinv_tile_steps(rows, K, pipe_lag, pipe_b, pipe_per0, pipe_per);
    // rounds of `cap` resident workgroups; inside a round a CU holds ceil(w/256) of them,
    // and a lone workgroup on a CU leaves issue slots idle (charged like `lone`: 1.6 for the
    // issue-bound variants with one or two vector streams, ~1 for the bandwidth-bound ones)
    const int64_t r = xinv_cdiv(wgs, cap), rounds = r > 1 ? r : 1;
    const int64_t w_last = wgs - (rounds - 1) * cap;
    // (pipelined kernel, measured at 3600x1800: a step of n workgroups on a CU costs ~1.5 + n -- 2, 3, 4
    //  per CU: 0.346, 0.445, 0.543 us -- the wavefronts wait for each other at the step barriers, and more
    //  of them per SIMD fill the gaps)
    const double full = pipe ? 1.5 + occ : ((occ == 1) ? lone : (double)occ);
    const double last = pipe ? 1.5 + (double)xinv_cdiv(w_last, 256) : ((w_last <= 256) ? lone : (double)xinv_cdiv(w_last, 256));
    return ((double)(rounds - 1) * full + last) * (double)steps;
}

// Number of row blocks for the fused 2-D kernels.  Tall tiles amortise the 4K recomputed halo
// rows, but every CU should hold the same number of workgroups: `occ` of the chosen variant fit
// per CU.  Minimise (workgroups per CU, in rounds of 256*occ resident ones) x (steps per tile): xinv_tile_cost;
// rows are then split evenly over the blocks (pipe_b > 0: the pipelined pass is costed by its tallest tile's exact steps).
__host__ inline int64_t xinv_choose_row_blocks(int64_t yc, int64_t nstrip, int64_t nbatch, int K, int occ, int occ_cap,
                                               double lone, int pipe_lag, int pipe_b = 0, int pipe_per0 = 8, int pipe_per = 8)
{
    const bool pipe = pipe_lag > 0;
    int64_t best = 1; double best_cost = 1e300;
    const int64_t n0 = xinv_cdiv(yc, pipe ? 512 : 128), nmin = n0 > 1 ? n0 : 1, nmax = nmin > yc / 4 ? nmin : yc / 4;
    for (int64_t nr = nmin; nr <= nmax; nr++) {
        const int64_t wgs = xinv_cdiv(nstrip * nr, pipe ? 1 : 4) * nbatch;
        const int64_t rows = (pipe && pipe_b > 0) ? xinv_even_split_tallest(yc, nr) : xinv_cdiv(yc, nr);
        const double cost = xinv_tile_cost(wgs, rows, K, occ, occ_cap, lone, pipe_lag, pipe_b, pipe_per0, pipe_per);
        if (cost <= best_cost * 1.0001) { best_cost = cost < best_cost ? cost : best_cost; best = nr; }   // ties: more, shorter tiles
    }
    return best;
}

// The cut of a 3-D column of zc planes into k chunks: nk chunks of KC = xinv_k_chunk_planes(zc, nk) planes (a multiple of
// four, at least 16, no empty chunk), nk <= 16; the count whose launch cost(nk, KC) is lowest, more chunks only for a gain
// of 3 %.
__host__ inline int64_t xinv_k_chunk_planes(int64_t zc, int nk) { return xinv_cdiv(xinv_cdiv(zc, nk), 4) * 4; }
template <class Cost>
__host__ inline int xinv_choose_k_chunks(int64_t zc, Cost cost)
{
    int best = 1; double best_cost = 1e300;
    for (int nk = 1; nk <= 16; nk++) {
        const int64_t KC = xinv_k_chunk_planes(zc, nk);
        if (nk > 1 && (KC < 16 || (int64_t)(nk - 1) * KC >= zc)) break;
        const double c = cost(nk, KC);
        if (c < best_cost * 0.97) { best_cost = c; best = nk; }
    }
    return best;
}
// k_fused3d / k_fused3dg (`wgs` = strips x row blocks x members): one workgroup per CU is resident (16 / 12 waves); the
// chunk count that minimises (rounds of 256 workgroups) x (planes marched per workgroup, incl. 4 halo + 4 warm-up)
__host__ inline int xinv_k_chunks_fused3d(int64_t zc, int64_t wgs)
{
    return xinv_choose_k_chunks(zc, [&](int nk, int64_t KC) { return (double)xinv_cdiv(wgs * nk, 256) * (double)(KC + (nk > 1 ? 10 : 2)); });
}
// k_pipe3d (xinv_p3_whole_tiles: which tiles of a launch are cut is decided per launch): the count that makes the launch
// of the whole batch (`tiles` = strips x row blocks x members) cheapest
__host__ inline int xinv_k_chunks_pipe3d(int64_t zc, int64_t tiles, int cus)
{
    return xinv_choose_k_chunks(zc, [&](int nk, int64_t KC) { double c; xinv_p3_whole_tiles(tiles, nk, KC, zc, cus, &c); return c; });
}
