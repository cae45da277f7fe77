// CPU check of k_pipe2d's tile records (xinvert_amd/csrc/xinv_tiles.h: PipeTileRec, xinv_pipe_tile_rec, xinv_lanecols_rec,
// xinv_lanecols_ring_rec, xinv_pipe_identity_recs), built and run by tests/test_pipe_tile_record.py.
// The kernel used to derive a tile's geometry at its entry, in every workgroup of every launch; `derive` below is that
// entry code, statement for statement (tile id -> row block and strip, xinv_tile_rows' split, xinv_pipe_gtot, the strip's
// lane map through make_lanecols / xinv_lanecols_ring, the unwrapped store column).  For every tile of every plan of the
// sweep -- yc in 4..300; row blocks from the even split and from a fixed RY; xc in {16, 112, 128, 224, 240, 3600, 3601}:
// 1, 1, 2, 2, 3, 33 and 33 strips; periodic and fixed x, the odd periodic row through the seam's ring layout; aligned
// and unaligned strips where the row length allows both -- every field of the record and, for all 64 lanes, every field
// of the lane map taken from the record (load columns, ok, use, classes, seam lane, store column) must equal it (the
// lanes of the tiles of the first and last row block; the map depends on the strip alone).
// Also: the records of a launch without a tile list put every tile into exactly one dispatch slot, tile T into slot T --
// in a seam launch the tile of the heavy-first order of the workgroup's dispatch position --, and the idle record
// (wt = -1) carries tile 0's geometry.
#include "xinv_tiles.h"
#include <cstdio>
#include <vector>

// the kernel's constants (xinv_pipe2d.h: XINV_PIPE_P = 4, _B = 2, _LAG = B + 5, _UW = 128 - 4 P, _PF0 = _PF = 4)
static const int P = 4, H = 2 * P, UWP = 128 - 4 * P, B = 2, LAG = B + 5, PER0 = 8, PER = 8;
static const PipeTileGeom G = {H, UWP, LAG, B, PER0, PER};

struct Derived { int strip, yu0, yu1, gtot, UW, HW; int64_t xu0; };
static Derived derive(int wt, int nstrip, int nrb, int64_t yc, int RY, int64_t xc, bool seam)
{
    Derived d;
    const int rb = wt / nstrip;
    d.strip = wt - rb * nstrip;
    if (RY > 0) {
        d.yu0 = rb * RY;
        d.yu1 = (d.yu0 + RY < (int)yc) ? d.yu0 + RY : (int)yc;
    } else {
        d.yu0 = (int)((((int64_t)rb * yc) / nrb) & ~(int64_t)1);
        d.yu1 = (rb + 1 == nrb) ? (int)yc : (int)((((int64_t)(rb + 1) * yc) / nrb) & ~(int64_t)1);
    }
    d.UW = seam ? xinv_ring_uw(xc, H) : UWP;
    d.HW = seam ? xinv_ring_hw(xc, H, d.strip) : H;
    d.xu0 = (int64_t)d.strip * d.UW;
    d.gtot = xinv_pipe_gtot(d.yu1 - d.yu0, LAG, B, PER0, PER);
    return d;
}

static int fail(const char *what, int64_t xc, int64_t yc, int nrb, int RY, int wt, int lane)
{
    std::printf("FAIL %s xc %ld yc %ld nrb %d RY %d tile %d lane %d\n", what, (long)xc, (long)yc, nrb, RY, wt, lane);
    return 1;
}

static bool same(const LaneCols &a, const LaneCols &b)
{
    return a.l0 == b.l0 && a.l1 == b.l1 && a.ok_x == b.ok_x && a.ok_y == b.ok_y && a.use_x == b.use_x && a.use_y == b.use_y &&
           a.cls_x == b.cls_x && a.cls_y == b.cls_y;
}

template <bool AL>
static int check_lanes(const PipeTileRec &r, const Derived &d, int64_t xc, bool per, bool seam, int64_t yc, int nrb, int RY)
{
    for (int lane = 0; lane < 64; lane++) {
        LaneCols want, got;
        bool ws = false, gs = false;
        if (seam) {
            want = xinv_lanecols_ring(d.xu0, d.HW, d.UW, lane, xc, ws);
            got = xinv_lanecols_ring_rec(r, d.UW, lane, (int)xc, gs);
        } else {
            want = make_lanecols<AL>(d.xu0, H, d.UW, lane, xc, per);
            got = xinv_lanecols_rec<AL>(r, d.UW, lane, (int)xc, per);
        }
        if (!same(want, got)) return fail(AL ? "lane map (aligned)" : "lane map", xc, yc, nrb, RY, r.wt, lane);
        if (ws != gs) return fail("seam lane", xc, yc, nrb, RY, r.wt, lane);
        if (d.xu0 - d.HW + 2 * lane != (int64_t)r.c0 + 2 * lane) return fail("store column", xc, yc, nrb, RY, r.wt, lane);
    }
    return 0;
}

int main()
{
    long tiles = 0, plans = 0;
    const int64_t xcs[] = {16, 112, 128, 224, 240, 3600, 3601};
    const int want_strips[] = {1, 1, 2, 2, 3, 33, 33};
    for (int xi = 0; xi < 7; xi++) for (int per = 0; per < 2; per++) {
        const int64_t xc = xcs[xi];
        const bool seam = per && (xc & 1);
        const int UW = seam ? xinv_ring_uw(xc, H) : UWP;
        const int nstrip = (int)((xc + UW - 1) / UW);
        if (nstrip != want_strips[xi]) return fail("strip count of the sweep", xc, 0, 0, 0, nstrip, 0);
        for (int64_t yc = 4; yc <= 300; yc++) {
            // the even split into 1, 2, 3 blocks and the most the planner allows (yc / 4); fixed heights 2, 12, 44, 46, yc
            std::vector<std::pair<int, int>> splits;      // (nrb, RY)
            for (int nrb : {1, 2, 3, (int)(yc / 4)}) if (nrb >= 1 && 2 * nrb <= yc) splits.push_back({nrb, 0});
            for (int RY : {2, 12, 44, 46, (int)yc}) if (RY <= yc) splits.push_back({(int)((yc + RY - 1) / RY), RY});
            for (const auto &sp : splits) {
                const int nrb = sp.first, RY = sp.second, NB = nstrip * nrb;
                plans++;
                for (int wt = 0; wt < NB; wt++) {
                    const Derived d = derive(wt, nstrip, nrb, yc, RY, xc, seam);
                    const PipeTileRec r = xinv_pipe_tile_rec(wt, nstrip, nrb, yc, RY, xc, per != 0, seam, G);
                    if (r.wt != wt || r.strip != d.strip || r.yu0 != d.yu0 || r.yu1 != d.yu1 || r.gtot != d.gtot ||
                        r.xu0 != d.xu0 || r.c0 != d.xu0 - d.HW)
                        return fail("record", xc, yc, nrb, RY, wt, -1);
                    const TileRows t = xinv_tile_rows(wt, nstrip, nrb, yc, RY);
                    if (t.strip != r.strip || t.y0 != r.yu0 || t.y1 != r.yu1) return fail("xinv_tile_rows", xc, yc, nrb, RY, wt, -1);
                    // (the lane map is a function of the strip: all 64 lanes for the tiles of the first and the last row
                    //  block; a tile between them carries the lane origin of the first block's tile of its strip)
                    if (wt < nstrip || wt >= NB - nstrip) {
                        if (check_lanes<false>(r, d, xc, per != 0, seam, yc, nrb, RY)) return 1;
                        if (!(xc & 1) && check_lanes<true>(r, d, xc, per != 0, seam, yc, nrb, RY)) return 1;
                    } else {
                        const PipeTileRec r0 = xinv_pipe_tile_rec(d.strip, nstrip, nrb, yc, RY, xc, per != 0, seam, G);
                        if (r.c0 != r0.c0 || r.w0 != r0.w0 || r.xu0 != r0.xu0) return fail("lane origin", xc, yc, nrb, RY, wt, -1);
                    }
                    tiles++;
                }
                // the idle record: tile 0's geometry, wt = -1
                {
                    const PipeTileRec i = xinv_pipe_tile_rec(-1, nstrip, nrb, yc, RY, xc, per != 0, seam, G);
                    const PipeTileRec z = xinv_pipe_tile_rec(0, nstrip, nrb, yc, RY, xc, per != 0, seam, G);
                    if (i.wt != -1 || i.strip != z.strip || i.yu0 != z.yu0 || i.yu1 != z.yu1 || i.gtot != z.gtot || i.c0 != z.c0 ||
                        i.w0 != z.w0 || i.xu0 != z.xu0)
                        return fail("idle record", xc, yc, nrb, RY, -1, -1);
                }
                // a launch without a tile list: slot T of dispatch position L holds the tile the kernel took there
                std::vector<PipeTileRec> recs((size_t)NB);
                for (auto &q : recs) q.wt = -2;
                xinv_pipe_identity_recs(recs.data(), nstrip, nrb, yc, RY, xc, per != 0, seam, G);
                std::vector<int> seen((size_t)NB, 0);
                for (int L = 0; L < NB; L++) {
                    const int q = NB >> 3, rem = NB & 7, xcd = L & 7, idx = L >> 3;
                    const int T = xcd * q + (xcd < rem ? xcd : rem) + idx;         // (the kernel's slot arithmetic)
                    if (T != xinv_pipe_slot(L, NB) || T < 0 || T >= NB) return fail("slot", xc, yc, nrb, RY, L, -1);
                    const int want = seam ? xinv_seam_tile(xinv_heavy_first(L, NB, (nstrip == 1 ? 1 : 2) * nrb), nstrip, nrb) : T;
                    if (recs[(size_t)T].wt != want) return fail("identity order", xc, yc, nrb, RY, L, -1);
                    if (seen[(size_t)want]++) return fail("identity bijection", xc, yc, nrb, RY, L, -1);
                }
            }
        }
    }
    std::printf("OK %ld tiles of %ld plans\n", tiles, plans);
    return 0;
}
