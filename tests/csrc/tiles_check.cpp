// CPU check of xinvert_amd/csrc/xinv_tiles.h (built and run by tests/test_tiles.py): for every geometry tried,
//  - the tiles of a strip partition the rows [0, yc), every tile starts on an even row;
//  - dispatch position -> xinv_heavy_first -> xinv_seam_tile visits every tile id exactly once, the edge strips' tiles in the
//    first rounds, eight consecutive positions (one per XCD) at a time;
//  - k_pipe3d's flat grid: dispatch slot -> (member, tile, chunk) covers every tile of every member once (whole column) or
//    once per chunk (cut tiles), each member has exactly one reducer and it is the member's last slot, the whole-column
//    slots of one XCD take a contiguous band of the member's tiles; the launch shape xinv_p3_whole_tiles picks is the
//    cheapest of the three it considers; the 'extend' tiling offset puts the row pairs 0 / 1 and yc-2 / yc-1 into one
//    wavefront in every row block whose second sweep reads them (checked by laying the rows out, for every row count).
//  - the planner's cost models: xinv_choose_row_blocks and the k-chunk searches return, for the shipped shapes, what the
//    planner returned before they moved into the header (recorded tables); every chunk count cuts the column into
//    non-empty chunks of a multiple of four planes that cover it.
#include "xinv_tiles.h"
#include <cstdio>
#include <vector>

static int fail(const char *what, int nstrip, int nrb, int parts, long yc)
{
    std::printf("FAIL %s nstrip %d nrb %d parts %d yc %ld\n", what, nstrip, nrb, parts, yc);
    return 1;
}

int main()
{
    long cases = 0;
    const int strips[] = {1, 2, 3, 4, 8, 31}, blocks[] = {1, 2, 3, 16, 31, 40};
    const long rows[] = {16, 17, 73, 180, 721};
    for (int nstrip : strips) for (int nrb : blocks) for (long yc : rows) {
        if (nrb * 2 > yc) continue;
        const int edges = nstrip == 1 ? 1 : 2, n = nstrip * nrb, nh = edges * nrb;
        for (int RY : {0, (int)((yc + nrb - 1) / nrb + 1) & ~1}) {
            if (RY && (long)RY * nrb < yc) continue;
            // rows of every strip covered once
            std::vector<std::vector<int>> cover((size_t)nstrip, std::vector<int>((size_t)yc, 0));
            for (int id = 0; id < n; id++) {
                const TileRows t = xinv_tile_rows(id, nstrip, nrb, yc, RY);
                if (t.strip < 0 || t.strip >= nstrip) return fail("strip", nstrip, nrb, 1, yc);
                if (t.y0 >= t.y1) continue;
                if (t.y0 & 1) return fail("odd first row", nstrip, nrb, 1, yc);
                if (t.y0 < 0 || t.y1 > yc) return fail("range", nstrip, nrb, 1, yc);
                for (long r = t.y0; r < t.y1; r++) cover[(size_t)t.strip][(size_t)r]++;
            }
            for (int s = 0; s < nstrip; s++) for (long r = 0; r < yc; r++)
                if (cover[(size_t)s][(size_t)r] != 1) return fail("cover", nstrip, nrb, 1, yc);
            cases++;
        }
        // dispatch order: a bijection, the edge strips' tiles in the first rounds
        std::vector<int> seen((size_t)n, 0);
        for (int L = 0; L < n; L++) {
            const int sq = xinv_heavy_first(L, n, nh);
            if (sq < 0 || sq >= n) return fail("sequence range", nstrip, nrb, 1, yc);
            const int id = xinv_seam_tile(sq, nstrip, nrb);
            if (id < 0 || id >= n || seen[(size_t)id]++) return fail("bijection", nstrip, nrb, 1, yc);
            const int strip = id % nstrip;
            const bool heavy = strip == 0 || strip == nstrip - 1;
            if ((L >> 3) < (nh >> 3) && !heavy) return fail("light tile in a heavy round", nstrip, nrb, 1, yc);
            if (heavy != (sq < nh)) return fail("heavy tiles first in the sequence", nstrip, nrb, 1, yc);
        }
        // workgroups of four tiles (k_fused2d, k_fused9): positions of workgroups, tiles sq * 4 + wave
        const int nwg = (n + 3) / 4;
        std::vector<int> seen4((size_t)(4 * nwg), 0);
        for (int L = 0; L < nwg; L++) {
            const int sq = xinv_heavy_first(L, nwg, nh >> 2);
            if (sq < 0 || sq >= nwg || seen4[(size_t)sq]++) return fail("workgroup bijection", nstrip, nrb, 1, yc);
        }
    }
    // the ring layout's strips (odd xc, periodic x): every strip has H halo columns a side, H + 2 on a side whose halo holds
    // the seam (west: the phantom column takes a slot; east: when column xc-1 sits in it anywhere but in the outermost slot)
    for (int H : {2, 4, 8, 12, 16})
        for (long xc = 65; xc < 1500; xc += 2) {
            const int uw = xinv_ring_uw(xc, H), nstrip = (int)((xc + uw - 1) / uw);
            if (uw != 128 - 2 * H - 2 && uw != 128 - 2 * H - 4) return fail("ring uw", nstrip, 0, H, xc);
            for (int s_ = 0; s_ < nstrip; s_++) {
                const int hw = xinv_ring_hw(xc, H, s_), he = 128 - hw - uw;
                const long lo = (long)s_ * uw - hw, hi = lo + 127;              // virtual columns of the strip's 128 slots
                if (hw < H || he < H) return fail("ring halo", nstrip, s_, H, xc);
                if (lo < 0 && hw < H + 2) return fail("ring west halo with the phantom column", nstrip, s_, H, xc);
                bool seam_east = false;                                         // column xc-1 (virtual xc-1 + n (xc+1)) in the east halo, not outermost
                for (long v = (long)s_ * uw + uw; v < hi; v++) seam_east = seam_east || ((v % (xc + 1)) == xc - 1);
                if (seam_east && he < H + 2) return fail("ring east halo with column xc-1", nstrip, s_, H, xc);
            }
            cases++;
        }
    // ---- k_pipe3d: slot -> (member, tile, chunk, reducer) ----
    for (int NT : {1, 3, 7, 8, 9, 16, 23, 138}) for (int nmem : {1, 2, 3, 5}) for (int nkc : {1, 2, 3, 4}) {
        const int tiles = NT * nmem;
        std::vector<int> cuts = {tiles, 0};                          // nfull: all whole, all cut, and remainders
        for (int cus : {4, 8, 13, 256}) if (tiles % cus && tiles / cus) cuts.push_back(tiles - tiles % cus);
        for (int r = 1; r < tiles; r += 5) cuts.push_back(tiles - r);
        for (int nfull : cuts) {
            if (nkc == 1 && nfull != tiles) continue;
            const int nslots = nfull + (tiles - nfull) * nkc;
            std::vector<int> seen((size_t)tiles * nkc, 0), last((size_t)nmem, -1), red((size_t)nmem, -1), nred((size_t)nmem, 0);
            std::vector<int> band_lo((size_t)nmem * 8, 1 << 30), band_hi((size_t)nmem * 8, -1), band_n((size_t)nmem * 8, 0), prev((size_t)nmem * 8, -1);
            for (int L = 0; L < nslots; L++) {
                const P3Slot sl = xinv_p3_slot(L, nfull, nkc, NT);
                if (sl.ml < 0 || sl.ml >= nmem || sl.Tj < 0 || sl.Tj >= NT || sl.kc < 0 || sl.kc >= nkc) return fail("p3 slot range", NT, nmem, nkc, nfull);
                if (sl.whole != (L < nfull) || (sl.whole && sl.kc)) return fail("p3 whole", NT, nmem, nkc, nfull);
                const size_t t = (size_t)(sl.ml * NT + sl.Tj) * nkc;
                if (sl.whole) { for (int c = 0; c < nkc; c++) if (seen[t + c]++) return fail("p3 tile twice", NT, nmem, nkc, nfull); }
                else if (seen[t + sl.kc]++) return fail("p3 chunk twice", NT, nmem, nkc, nfull);
                last[(size_t)sl.ml] = L;
                if (sl.reducer) { red[(size_t)sl.ml] = L; nred[(size_t)sl.ml]++; }
                if (sl.whole) {                                      // XCD bands: contiguous, ascending with the slot
                    const size_t b = (size_t)sl.ml * 8 + (L & 7);
                    if (sl.Tj <= prev[b]) return fail("p3 band order", NT, nmem, nkc, nfull);
                    prev[b] = sl.Tj;
                    band_lo[b] = sl.Tj < band_lo[b] ? sl.Tj : band_lo[b];
                    band_hi[b] = sl.Tj > band_hi[b] ? sl.Tj : band_hi[b];
                    band_n[b]++;
                }
            }
            for (size_t i = 0; i < seen.size(); i++) if (seen[i] != 1) return fail("p3 cover", NT, nmem, nkc, nfull);
            for (int m = 0; m < nmem; m++) {
                if (nred[(size_t)m] != 1 || red[(size_t)m] != last[(size_t)m]) return fail("p3 reducer is the member's last slot", NT, nmem, nkc, nfull);
                int next = 0;                                        // the bands follow each other in XCD order from tile 0
                for (int x = 0; x < 8; x++) {
                    const size_t b = (size_t)m * 8 + x;
                    if (!band_n[b]) continue;
                    if (band_lo[b] != next || band_hi[b] - band_lo[b] + 1 != band_n[b]) return fail("p3 band contiguous", NT, nmem, nkc, nfull);
                    next = band_hi[b] + 1;
                }
            }
            cases++;
        }
    }
    // ---- k_pipe3d: launch shape ----
    for (long tiles : {1L, 7L, 138L, 256L, 257L, 300L, 512L, 1104L, 2070L, 2208L}) for (int nk : {1, 2, 3, 4}) for (long zc : {10L, 50L, 120L})
        for (int cus : {256, -256, 64, 8}) {
            const long KC = (zc + nk - 1) / nk, c = cus < 0 ? -cus : cus;
            double cost = -1;
            const long nf = xinv_p3_whole_tiles(tiles, nk, KC, zc, cus, &cost);
            const double cf = (double)(zc + 4), cs = (double)(KC + 14);
            const double c_whole = (double)((tiles + c - 1) / c) * cf, c_all = (double)((tiles * nk + c - 1) / c) * cs;
            const long r = tiles % c;
            const double c_rem = (double)(tiles / c) * cf + (double)((r * nk + c - 1) / c) * cs;
            double want;
            if (nf == tiles) want = c_whole;
            else if (nf == 0) want = c_all;
            else if (nf == tiles - r && r && tiles / c && cus > 0) want = c_rem;
            else return fail("p3 launch shape is none of the three", (int)tiles, nk, cus, zc);
            if (nk == 1 && nf != tiles) return fail("p3 cut without chunks", (int)tiles, nk, cus, zc);
            if (cost != want) return fail("p3 launch shape cost", (int)tiles, nk, cus, zc);
            if (cost > c_whole) return fail("p3 launch shape dearer than whole columns", (int)tiles, nk, cus, zc);
            // a cut is taken only when it wins by its margin; never lose more than the margin against the cheapest
            double cheapest = c_whole;
            if (nk > 1) { cheapest = c_all < cheapest ? c_all : cheapest; if (r && tiles / c && cus > 0) cheapest = c_rem < cheapest ? c_rem : cheapest; }
            if (cost > cheapest / 0.97 + 1e-9) return fail("p3 launch shape far from the cheapest", (int)tiles, nk, cus, zc);
            cases++;
        }
    // ---- k_pipe3d, BCy = 'extend': the tiling offset, for every row count ----
    {
        const int G = 8, RR = 3, H = 4, NR = G * RR, RJ = NR - 2 * H;
        for (long yc = 4; yc <= 3000; yc++) {
            const int joff = xinv_p3_extend_joff(yc, RJ, H, RR);
            if (joff != 0 && joff != 2) return fail("p3 extend: no tiling offset", 0, 0, joff, yc);
            if (!xinv_p3_extend_ok(yc, joff, RJ, H, RR)) return fail("p3 extend: joff not ok", 0, 0, joff, yc);
            const long njb = (yc + joff + RJ - 1) / RJ;
            auto wave_of = [&](long jb, long j) { const long li = j - (jb * RJ - H - joff); return (li < 0 || li >= NR) ? -1L : li / RR; };
            for (long jb = 0; jb < njb; jb++) {
                const long own0 = jb * RJ - joff, own1 = own0 + RJ;
                // the second sweep of this block: first colour on rows [own0-1, own1+1), second on [own0, own1), rows 1..yc-2 only
                for (long j = own0 - 1; j < own1 + 1; j++) {
                    if (j < 1 || j > yc - 2) continue;
                    if (j == 1 && (wave_of(jb, 0) < 0 || wave_of(jb, 0) != wave_of(jb, 1)))
                        return fail("p3 extend: rows 0 / 1 in two wavefronts", (int)jb, 0, joff, yc);
                    if (j == yc - 2 && (wave_of(jb, yc - 1) < 0 || wave_of(jb, yc - 1) != wave_of(jb, yc - 2)))
                        return fail("p3 extend: rows yc-2 / yc-1 in two wavefronts", (int)jb, 0, joff, yc);
                }
            }
            cases++;
        }
    }
    // ---- the planner's cost models ----
    // Expected values recorded from commit 3ddae19 ("Split the host-pointer solve into named steps over one call state"): its
    // choose_row_blocks (xinv_launch.h) and the two k-chunk loops of plan_fused3d (xinv_plan.h), compiled unchanged into a
    // scratch harness.  Shapes: 1800x3600, 720x1440, 180x360, 73x144, 2000x2000 (strips of 128 - 4K owned columns, 112 for
    // the pipelined pass), batches of 1, 8, 64; per row the fifteen results for occ 1..5 x lone 1.0, 1.3, 1.6 (lone runs fastest).
    {
        const int occ_cap = 3, pipe_cap = 5, pipe_lag = 7;               // (xinv_launch.h: pipe_occ_cap(); XINV_PIPE_LAG)
        static const struct { long yc, nstrip, nbatch; int K, pipe; long nrb[15]; } rb[] = {
            {1800, 30,  1, 1, 0, {34, 34, 34, 34, 68, 68, 34, 68, 68, 34, 68, 68, 34, 68, 68}},
            {1800, 30,  1, 2, 0, {34, 34, 34, 34, 68, 68, 34, 68, 68, 34, 68, 68, 34, 68, 68}},
            {1800, 32,  1, 3, 0, {32, 32, 32, 32, 32, 64, 32, 32, 96, 32, 32, 96, 32, 32, 96}},
            {1800, 33,  1, 4, 0, {31, 31, 31, 31, 62, 62, 31, 62, 62, 31, 62, 62, 31, 62, 62}},
            {1800, 33,  1, 4, 1, {7, 7, 7, 15, 15, 15, 23, 23, 23, 31, 31, 31, 31, 31, 31}},
            {1800, 30,  8, 1, 0, {17, 17, 17, 17, 17, 17, 17, 21, 21, 17, 21, 21, 17, 21, 21}},
            {1800, 30,  8, 2, 0, {21, 21, 21, 21, 17, 17, 21, 21, 21, 21, 21, 21, 21, 21, 21}},
            {1800, 32,  8, 3, 0, {16, 16, 16, 16, 16, 16, 16, 20, 20, 16, 20, 20, 16, 20, 20}},
            {1800, 33,  8, 4, 0, {15, 15, 15, 15, 15, 15, 15, 23, 23, 15, 23, 23, 15, 23, 23}},
            {1800, 33,  8, 4, 1, {12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 9, 9, 9}},
            {1800, 30, 64, 1, 0, {17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17}},
            {1800, 30, 64, 2, 0, {24, 24, 24, 24, 16, 16, 24, 24, 24, 24, 24, 24, 24, 24, 24}},
            {1800, 32, 64, 3, 0, {17, 17, 17, 17, 17, 17, 17, 15, 15, 17, 15, 15, 17, 15, 15}},
            {1800, 33, 64, 4, 0, {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
            {1800, 33, 64, 4, 1, {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4}},
            { 720, 12,  1, 1, 0, {85, 85, 85, 85, 85, 170, 85, 85, 170, 85, 85, 170, 85, 85, 170}},
            { 720, 12,  1, 2, 0, {85, 85, 85, 85, 85, 85, 85, 85, 85, 85, 85, 85, 85, 85, 85}},
            { 720, 13,  1, 3, 0, {78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78}},
            { 720, 13,  1, 4, 0, {78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78}},
            { 720, 13,  1, 4, 1, {19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19}},
            { 720, 12,  8, 1, 0, {21, 21, 21, 21, 21, 21, 21, 21, 21, 21, 21, 21, 21, 21, 21}},
            { 720, 12,  8, 2, 0, {10, 10, 10, 10, 21, 21, 10, 21, 21, 10, 21, 21, 10, 21, 21}},
            { 720, 13,  8, 3, 0, {9, 9, 9, 9, 19, 19, 9, 19, 19, 9, 19, 19, 9, 19, 19}},
            { 720, 13,  8, 4, 0, {9, 9, 9, 9, 19, 19, 9, 19, 19, 9, 19, 19, 9, 19, 19}},
            { 720, 13,  8, 4, 1, {2, 2, 2, 4, 4, 4, 7, 7, 7, 7, 7, 7, 12, 12, 12}},
            { 720, 12, 64, 1, 0, {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8}},
            { 720, 12, 64, 2, 0, {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8}},
            { 720, 13, 64, 3, 0, {6, 6, 6, 6, 7, 7, 6, 6, 6, 6, 6, 6, 6, 6, 6}},
            { 720, 13, 64, 4, 0, {6, 6, 6, 6, 7, 7, 6, 6, 6, 6, 6, 6, 6, 6, 6}},
            { 720, 13, 64, 4, 1, {4, 4, 4, 3, 3, 3, 4, 4, 4, 2, 2, 2, 3, 3, 3}},
            { 180,  3,  1, 1, 0, {45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45}},
            { 180,  3,  1, 2, 0, {45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45}},
            { 180,  4,  1, 3, 0, {45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45}},
            { 180,  4,  1, 4, 0, {45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45}},
            { 180,  4,  1, 4, 1, {45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45, 45}},
            { 180,  3,  8, 1, 0, {42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42}},
            { 180,  3,  8, 2, 0, {42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42}},
            { 180,  4,  8, 3, 0, {32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32}},
            { 180,  4,  8, 4, 0, {32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32}},
            { 180,  4,  8, 4, 1, {8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
            { 180,  3, 64, 1, 0, {5, 5, 5, 5, 10, 10, 5, 10, 10, 5, 10, 10, 5, 10, 10}},
            { 180,  3, 64, 2, 0, {5, 5, 5, 5, 10, 10, 5, 10, 10, 5, 10, 10, 5, 10, 10}},
            { 180,  4, 64, 3, 0, {4, 4, 4, 4, 8, 8, 4, 8, 8, 4, 8, 8, 4, 8, 8}},
            { 180,  4, 64, 4, 0, {4, 4, 4, 4, 8, 8, 4, 8, 8, 4, 8, 8, 4, 8, 8}},
            { 180,  4, 64, 4, 1, {1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 4}},
    {  73,  2,  1, 1, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  1, 2, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  1, 3, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  1, 4, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  1, 4, 1, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  8, 1, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  8, 2, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  8, 3, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  8, 4, 0, {18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18}},
    {  73,  2,  8, 4, 1, {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
    {  73,  2, 64, 1, 0, {8, 8, 8, 8, 8, 16, 8, 8, 16, 8, 8, 16, 8, 8, 16}},
    {  73,  2, 64, 2, 0, {8, 8, 8, 8, 8, 16, 8, 8, 16, 8, 8, 16, 8, 8, 16}},
    {  73,  2, 64, 3, 0, {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8}},
    {  73,  2, 64, 4, 0, {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8}},
    {  73,  2, 64, 4, 1, {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}},
            {2000, 17,  1, 1, 0, {60, 60, 60, 60, 120, 120, 60, 120, 120, 60, 120, 120, 60, 120, 120}},
            {2000, 17,  1, 2, 0, {60, 60, 60, 60, 120, 120, 60, 120, 120, 60, 120, 120, 60, 120, 120}},
            {2000, 18,  1, 3, 0, {56, 56, 56, 56, 113, 113, 56, 113, 113, 56, 113, 113, 56, 113, 113}},
            {2000, 18,  1, 4, 0, {56, 56, 56, 56, 56, 113, 56, 56, 113, 56, 56, 113, 56, 56, 113}},
            {2000, 18,  1, 4, 1, {14, 14, 14, 28, 28, 28, 42, 42, 42, 56, 56, 56, 56, 56, 56}},
            {2000, 17,  8, 1, 0, {30, 30, 30, 30, 30, 30, 30, 22, 22, 30, 22, 22, 30, 22, 22}},
            {2000, 17,  8, 2, 0, {22, 22, 22, 22, 30, 30, 22, 22, 22, 22, 22, 22, 22, 22, 22}},
            {2000, 18,  8, 3, 0, {21, 21, 21, 21, 28, 28, 21, 21, 21, 21, 21, 21, 21, 21, 21}},
            {2000, 18,  8, 4, 0, {28, 28, 28, 28, 28, 28, 28, 21, 21, 28, 21, 21, 28, 21, 21}},
            {2000, 18,  8, 4, 1, {7, 7, 7, 7, 7, 7, 5, 5, 5, 7, 7, 7, 7, 7, 7}},
            {2000, 17, 64, 1, 0, {16, 16, 16, 16, 16, 30, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
            {2000, 17, 64, 2, 0, {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
            {2000, 18, 64, 3, 0, {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
            {2000, 18, 64, 4, 0, {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
            {2000, 18, 64, 4, 1, {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4}},
        };
        const double lones[3] = {1.0, 1.3, 1.6};
        for (const auto &r : rb) for (int occ = 1; occ <= 5; occ++) for (int l = 0; l < 3; l++) {
            const long got = (long)xinv_choose_row_blocks(r.yc, r.nstrip, r.nbatch, r.K, occ, r.pipe ? pipe_cap : occ_cap,
                                                          lones[l], r.pipe ? pipe_lag : 0);
            if (got != r.nrb[(occ - 1) * 3 + l]) return fail("row blocks differ from the recorded plan", (int)r.nstrip, (int)got, occ, r.yc);
            // ... and the cost it was chosen by is the one the masked-tile planner weighs its own splits against
            const long wgs = (r.nstrip * got + (r.pipe ? 0 : 3)) / (r.pipe ? 1 : 4) * r.nbatch;
            const double c = xinv_tile_cost(wgs, (r.yc + got - 1) / got, r.K, occ, r.pipe ? pipe_cap : occ_cap, lones[l], r.pipe ? pipe_lag : 0);
            for (long nr = got + 1; nr <= r.yc / 4; nr++) {              // (ties go to the larger count: none behind it is as cheap)
                const long w = (r.nstrip * nr + (r.pipe ? 0 : 3)) / (r.pipe ? 1 : 4) * r.nbatch;
                if (xinv_tile_cost(w, (r.yc + nr - 1) / nr, r.K, occ, r.pipe ? pipe_cap : occ_cap, lones[l], r.pipe ? pipe_lag : 0) <= c)
                    return fail("a larger row-block count is as cheap", (int)r.nstrip, (int)nr, occ, r.yc);
            }
            cases++;
        }
        // 50 x 360 x 720 and 601 x 300 x 300, batches of 1, 2, 8, 15, 64: workgroups of k_fused3d with 16 / 12 wavefronts
        // (wg16, wg12), tiles of k_pipe3d (tiles2) on `cus` compute units -> k chunks of the three
        static const struct { long zc, wg16, wg12, tiles2; int cus, nk16, nk12, nk2; } kc[] = {
            { 50,   180,   270,   138,  256, 1, 1, 1},
            { 50,   180,   270,   138, -256, 1, 1, 1},
            { 50,   180,   270,   138,   64, 1, 1, 3},
            { 50,   360,   540,   276,  256, 1, 1, 4},
            { 50,   360,   540,   276, -256, 1, 1, 1},
            { 50,   360,   540,   276,   64, 1, 1, 3},
            { 50,  1440,  2160,  1104,  256, 1, 1, 3},
            { 50,  1440,  2160,  1104, -256, 1, 1, 1},
            { 50,  1440,  2160,  1104,   64, 1, 1, 1},
            { 50,  2700,  4050,  2070,  256, 1, 1, 3},
            { 50,  2700,  4050,  2070, -256, 1, 1, 1},
            { 50,  2700,  4050,  2070,   64, 1, 1, 1},
            { 50, 11520, 17280,  8832,  256, 1, 1, 1},
            { 50, 11520, 17280,  8832, -256, 1, 1, 1},
            { 50, 11520, 17280,  8832,   64, 1, 1, 1},
            {601,    75,   114,    57,  256, 3, 2, 4},
            {601,    75,   114,    57, -256, 3, 2, 4},
            {601,    75,   114,    57,   64, 3, 2, 1},
            {601,   150,   228,   114,  256, 5, 1, 2},
            {601,   150,   228,   114, -256, 5, 1, 2},
            {601,   150,   228,   114,   64, 5, 1, 5},
            {601,   600,   912,   456,  256, 2, 1, 5},
            {601,   600,   912,   456, -256, 2, 1, 1},
            {601,   600,   912,   456,   64, 2, 1, 4},
            {601,  1125,  1710,   855,  256, 2, 1, 2},
            {601,  1125,  1710,   855, -256, 2, 1, 2},
            {601,  1125,  1710,   855,   64, 2, 1, 2},
            {601,  4800,  7296,  3648,  256, 1, 1, 2},
            {601,  4800,  7296,  3648, -256, 1, 1, 1},
            {601,  4800,  7296,  3648,   64, 1, 1, 1},
        };
        for (const auto &r : kc) {
            if (xinv_k_chunks_fused3d(r.zc, r.wg16) != r.nk16 || xinv_k_chunks_fused3d(r.zc, r.wg12) != r.nk12)
                return fail("k chunks (one sweep) differ from the recorded plan", (int)r.wg16, (int)r.wg12, r.cus, r.zc);
            if (xinv_k_chunks_pipe3d(r.zc, r.tiles2, r.cus) != r.nk2)
                return fail("k chunks (two sweeps) differ from the recorded plan", (int)r.tiles2, 0, r.cus, r.zc);
            cases++;
        }
        // every chunk count cuts the column into nk non-empty chunks of KC planes, KC a multiple of four, that cover it
        for (long zc = 3; zc <= 1500; zc++) for (long wgs : {1L, 57L, 138L, 256L, 300L, 2070L, 40000L}) for (int cus : {256, -256, 8}) {
            for (int which = 0; which < 2; which++) {
                const int nk = which ? xinv_k_chunks_pipe3d(zc, wgs, cus) : xinv_k_chunks_fused3d(zc, wgs);
                const long KC = (long)xinv_k_chunk_planes(zc, nk);
                if (nk < 1 || nk > 16 || KC % 4 != 0 || !((nk - 1) * KC < zc && zc <= nk * KC))
                    return fail("k chunks do not cut the column", nk, (int)KC, cus, zc);
            }
            cases++;
        }
    }
    std::printf("OK %ld geometries\n", cases);
    return 0;
}
