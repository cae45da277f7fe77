// CPU check of the wave-pipelined pass's schedule, xinv_pipe_* in xinvert_amd/csrc/xinv_tiles.h (built and run by
// tests/test_pipe_schedule.py).  For every tile height ry = 1..300 and B = 1, 2 steps per barrier (LAG = B + 5, unroll
// period 8) the four wavefronts are marched step by step the way xinv_pipe_wave does it -- barriers before the march, the
// first ring read, the unrolled march with its compile-time row colour, ring-slot names and barrier positions, barriers
// behind it -- from the shared functions alone, and
//  (a) every ring read of a row the reader needs falls in a barrier interval strictly after the one of the producer's write
//      of that row into that slot, and strictly before the one of the slot's next write (reads of padded rows are exempt,
//      and only those); every needed row enters its wavefront in step LAG pw + (row - first needed row), on its own colour;
//  (b) all four wavefronts pass gtot / B barriers, each at the end of a global step g with (g + 1) % B == 0;
//  (c) wavefront 3 has finished its last needed row after 3 LAG + ry + 4 steps and gtot <= roundup_B(3 LAG + ry + 4) + 2;
//  (d) the steps of the planner's cost model, xinv_tile_cost, are the simulated gtot -- for a tile height, and for the
//      tallest tile of an even split (xinv_even_split_tallest against xinv_tile_rows, every split of up to 400 rows).
//      (xinv_tile_steps calls xinv_pipe_gtot: what stands behind (d) is the simulation's own count -- gtot is the longest of
//      the four marches as simulated, rounded up to whole barrier periods.)
// The simulation restates the kernel's expressions -- the slot names RSLOT, the barrier positions, the loop before the
// march -- next to the shared functions: it proves the schedule those functions define, not that xinv_pipe_wave is written
// as simulated.  That the kernel computes the right bits with it is what tests/test_gpu_pipe_schedule.py checks on the GPU.
#include "xinv_tiles.h"
#include <cstdio>
#include <vector>

static int fail(const char *what, int ry, int B, int pw, long v)
{
    std::printf("FAIL %s ry %d B %d pw %d value %ld\n", what, ry, B, pw, v);
    return 1;
}

struct Ev { int step, row, slot; };

// marches the four wavefronts of a tile of ry rows; returns 0 and the steps the tile takes in *gtot_out
static int simulate(int ry, int B, int *gtot_out)
{
    const int LAG = B + 5, R = 8, NS = 4;
    const int gtot = xinv_pipe_gtot(ry, LAG, B, R, R);
    std::vector<Ev> writes[4], reads[4];                 // ring pw is written by wavefront pw, read by wavefront pw + 1
    int end_max = 0;
    for (int pw = 0; pw < 4; pw++) {
        const int n = xinv_pipe_rows(ry, pw), pad = xinv_pipe_pad(ry, pw, R);
        const int front = xinv_pipe_front(ry, pw, LAG, R), endp = xinv_pipe_end(ry, pw, LAG, R);
        const int first = xinv_pipe_first_row(ry, pw, LAG, R), start = xinv_pipe_start(ry, pw, LAG, R);
        const int gread = xinv_pipe_first_read(ry, pw, LAG, R), flip = pw > 0 ? xinv_pipe_slot_flip(front) : 0;
        const int need_lo = -8 + 2 * pw, need_hi = ry + 7 - 2 * pw;
        if (n != need_hi - need_lo + 1) return fail("rows needed", ry, B, pw, n);
        if (front < 0 || (front & 1) || endp < 0 || front + endp != pad || (n + pad) % R) return fail("padding", ry, B, pw, front);
        if (pw == 0 && front) return fail("wavefront 0 starts before step 0", ry, B, pw, front);
        if (start < 0 || first != need_lo - front || start != LAG * pw - front) return fail("start", ry, B, pw, start);
        if (flip != 0 && flip != 2) return fail("slot flip", ry, B, pw, flip);
        int g = 0, barriers = 0;
        // before the march: barriers, and the first marched row out of the ring in the step before the first
        for (; g < gread; g++) if ((g + 1) % B == 0) barriers++;
        if (pw > 0 && gread >= 0) {
            reads[pw].push_back({g, first, ((2 * pw) % NS) ^ flip});
            if ((g + 1) % B == 0) barriers++;
            g++;
        }
        if (g != start) return fail("the march does not start in its step", ry, B, pw, g);
        // the march: whole periods from the first row until the last needed one is in
        for (int rb = first; rb <= need_hi; rb += R) {
            for (int U = 0; U < R; U++) {
                const int r = rb + U;
                if (((r - U) & 1) != 0) return fail("row colour is not compile-time", ry, B, pw, r);
                if (r >= need_lo && r <= need_hi && g != LAG * pw + (r - need_lo)) return fail("a needed row enters off its step", ry, B, pw, r);
                if (pw > 0) reads[pw].push_back({g, r + 1, ((2 * pw + U + 1) % NS) ^ flip});
                if (pw < 3) writes[pw].push_back({g, r - 2, ((2 * pw + U - 2 + 16 * NS) % NS) ^ flip});
                const bool bar = (LAG * pw + U + 1) % B == 0;         // (compile-time in the kernel)
                if (bar != ((g + 1) % B == 0)) return fail("barrier off the global grid", ry, B, pw, g);
                barriers += bar;
                g++;
            }
        }
        if (g != start + n + pad) return fail("march length", ry, B, pw, g);
        if (g > gtot) return fail("march longer than gtot", ry, B, pw, g);
        end_max = g > end_max ? g : end_max;
        if (pw == 3) {                                               // (c)
            const int done = start + (need_hi - first) + 1;
            if (done != 3 * LAG + ry + 4) return fail("wavefront 3 finishes late", ry, B, pw, done);
        }
        for (; g < gtot; g++) if ((g + 1) % B == 0) barriers++;
        if (barriers * B != gtot) return fail("barrier count", ry, B, pw, barriers);                 // (b)
    }
    if (gtot != (end_max + B - 1) / B * B) return fail("gtot is not the longest schedule", ry, B, -1, gtot);
    const int need3 = (3 * LAG + ry + 4 + B - 1) / B * B;
    if (gtot < need3 || gtot > need3 + 2) return fail("gtot out of bound", ry, B, -1, gtot);          // (c)
    // (a) the hand-over: ring pw - 1 between its writer and wavefront pw
    for (int pw = 1; pw < 4; pw++) {
        const int need_lo = -8 + 2 * pw, need_hi = ry + 7 - 2 * pw;
        const std::vector<Ev> &w = writes[pw - 1];
        int checked = 0;
        for (const Ev &rd : reads[pw]) {
            if (rd.row < need_lo || rd.row > need_hi) continue;      // padding: may read anything
            int iw = -1;
            for (int k = 0; k < (int)w.size(); k++) if (w[k].row == rd.row) { if (iw >= 0) return fail("row written twice", ry, B, pw, rd.row); iw = k; }
            if (iw < 0) return fail("needed row never written", ry, B, pw, rd.row);
            if (w[iw].slot != rd.slot) return fail("reader and writer disagree on the slot", ry, B, pw, rd.row);
            if (!(w[iw].step / B < rd.step / B)) return fail("read not after the write's barrier interval", ry, B, pw, rd.row);
            for (int k = 0; k < (int)w.size(); k++) {
                if (k == iw || w[k].slot != rd.slot) continue;
                // every other write to the slot: before this row's (any interval), or in a later interval than the read
                const bool before = w[k].step < w[iw].step, after = w[k].step / B > rd.step / B;
                if (!before && !after) return fail("slot overwritten before it is read", ry, B, pw, rd.row);
            }
            checked++;
        }
        if (checked != need_hi - need_lo + 1) return fail("needed rows read", ry, B, pw, checked);
    }
    *gtot_out = gtot;
    return 0;
}

int main()
{
    long cases = 0;
    for (int B = 1; B <= 2; B++) for (int ry = 1; ry <= 300; ry++) {
        int gtot = 0;
        if (simulate(ry, B, &gtot)) return 1;
        // (d) the planner's steps: one workgroup on one CU costs (1.5 + 1) x steps
        if (xinv_tile_steps(ry, 4, B + 5, B) != gtot) return fail("xinv_tile_steps", ry, B, -1, (long)xinv_tile_steps(ry, 4, B + 5, B));
        if (xinv_tile_cost(1, ry, 4, 1, 5, 1.0, B + 5, B) != 2.5 * (double)gtot) return fail("xinv_tile_cost", ry, B, -1, gtot);
        cases++;
    }
    // the table of the schedule's design note: 3600 x 1800 in 40 row blocks has tiles of 44 and 46 rows
    {
        static const int tab[][2] = {{44, 70}, {46, 72}, {52, 78}, {54, 80}, {60, 86}};
        for (const auto &t : tab) if (xinv_pipe_gtot(t[0], 7, 2, 8, 8) != t[1]) return fail("steps of a known height", t[0], 2, -1, xinv_pipe_gtot(t[0], 7, 2, 8, 8));
    }
    // (d) the tallest tile of an even split, and the cost of the split by it
    for (long yc = 4; yc <= 400; yc++) for (long nrb = 1; nrb <= yc / 2; nrb++) {
        long tallest = 0;
        for (int rb = 0; rb < nrb; rb++) {
            const TileRows t = xinv_tile_rows(rb, 1, (int)nrb, yc, 0);
            tallest = (t.y1 - t.y0) > tallest ? (long)(t.y1 - t.y0) : tallest;
        }
        if ((long)xinv_even_split_tallest(yc, nrb) != tallest) return fail("tallest tile of the even split", (int)yc, 0, (int)nrb, tallest);
        if (tallest <= 300 && ((yc + nrb) % 7) == 0) {
            int gtot = 0;
            if (simulate((int)tallest, 2, &gtot)) return 1;
            if (xinv_tile_cost(nrb, xinv_even_split_tallest(yc, nrb), 4, 1, 5, 1.0, 7, 2) != 2.5 * (double)gtot) return fail("cost of a split", (int)yc, 2, (int)nrb, gtot);
        }
        cases++;
    }
    // the headline's split as the planner weighs it, and the choice made with the exact steps is a minimum of its own cost
    if (xinv_even_split_tallest(1800, 40) != 46) return fail("tallest of 1800 / 40", 1800, 2, 40, (long)xinv_even_split_tallest(1800, 40));
    for (long nbatch : {1L, 8L, 64L}) for (int occ = 1; occ <= 5; occ++) {
        const long yc = 1800, nstrip = 33;
        const long got = (long)xinv_choose_row_blocks(yc, nstrip, nbatch, 4, occ, 5, 1.0, 7, 2);
        const double c = xinv_tile_cost(nstrip * got * nbatch, xinv_even_split_tallest(yc, got), 4, occ, 5, 1.0, 7, 2);
        for (long nr = (yc + 511) / 512; nr <= yc / 4; nr++) {
            const double o = xinv_tile_cost(nstrip * nr * nbatch, xinv_even_split_tallest(yc, nr), 4, occ, 5, 1.0, 7, 2);
            if (o * 1.0001 < c || (nr > got && o <= c)) return fail("chosen split is not the cheapest", (int)yc, occ, (int)nr, got);
        }
        cases++;
    }
    std::printf("OK %ld cases\n", cases);
    return 0;
}
