// CPU check of xinvert_amd/csrc/xinv_rotation.h (built and run by tests/test_rotation.py).  One member's buffers are
// labelled with the sweep count of the state they hold (-1: nothing valid) and the launches of a solve are simulated for
// two and three buffers, K = 1..4 sweeps per launch and budgets of 1..40 sweeps; for every stop sweep:
//  - with the lagged norm no launch overwrites the source of the previous launch unless the pending norm was flushed first;
//  - a solve that runs its whole budget with the lagged norm ends in buffer 0;
//  - the redo of finalise reads the state it expects, never writes the buffer it reads in the same step and returns the
//    buffer holding the stop sweep's state -- also where the biharmonic 'extend' pre-pass of the next launch has
//    scribbled on the stopped launch's output;
//  - the watchdog recovery (two-buffer redo from a launch's boundary) ends with the state of its stop sweep;
//  - the two-buffer rotation started in buffer j is the rolling batch's ping-pong with start parity j.
#include "xinv_rotation.h"
#include <cstdio>
#include <vector>

static int fail(const char *what, int nbuf, int K, int budget, long sw)
{
    std::printf("FAIL %s nbuf %d K %d budget %d stop %ld\n", what, nbuf, K, budget, sw);
    return 1;
}

struct Solve {                                           // the launches of one solve, as the sweep loop issues them
    std::vector<int64_t> bound;                          // bound[i] = sweeps before launch i; bound[n] = budget
    std::vector<signed char> srcb, dstb;
    std::vector<bool> flushed;                           // the pending norm was evaluated before launch i
};

static bool issue(Solve &s, int nbuf, int K, int budget, int start)
{
    const bool lag = nbuf == 3;
    const int64_t nl = (budget + K - 1) / K;
    const int64_t flip = xinv_flip_at(lag, nl);
    int64_t done = 0;
    for (int64_t i = 0; done < budget; i++) {
        const int src = i == 0 ? start : s.dstb[(size_t)i - 1];
        const int prev = i == 0 ? -1 : s.srcb[(size_t)i - 1];
        const XinvRot r = xinv_rot_dst(i, src, prev, nbuf, flip);
        if (r.dst == src || r.dst < 0 || r.dst >= nbuf) return false;
        s.srcb.push_back((signed char)src); s.dstb.push_back((signed char)r.dst); s.flushed.push_back(r.flush);
        s.bound.push_back(done);
        done += (K < budget - done) ? K : budget - done;
    }
    s.bound.push_back(done);
    return true;
}

int main()
{
    long cases = 0;
    for (int nbuf = 2; nbuf <= 3; nbuf++)
    for (int K = 1; K <= 4; K++)
    for (int budget = 1; budget <= 40; budget++) {
        const bool lag = nbuf == 3;
        if (lag && budget <= K) continue;                // (the sweep loop lags the norm only with more than one launch)
        Solve s;
        if (!issue(s, nbuf, K, budget, 0)) return fail("destination", nbuf, K, budget, -1);
        const int64_t nl = (int64_t)s.srcb.size();
        for (int64_t i = 1; lag && i < nl; i++)
            if (s.dstb[(size_t)i] == s.srcb[(size_t)i - 1] && !s.flushed[(size_t)i])
                return fail("overwrote the previous launch's source without a flush", nbuf, K, budget, -1);
        if (lag && s.dstb.back() != 0) return fail("whole budget does not end in buffer 0", nbuf, K, budget, -1);

        for (int extend = 0; extend <= (lag ? 1 : 0); extend++)
        for (long sw = 1; sw <= budget; sw++) {
            // run the launches: every launch up to the one holding sw writes its whole pass; with the lagged norm the next
            // one too unless it was flushed before (the decision arrives during it); everything later is a no-op
            std::vector<long> lab((size_t)nbuf, -1);
            lab[0] = 0;
            int64_t hold = -1;
            for (int64_t i = 0; i < nl; i++) {
                if (hold >= 0) {
                    if (i != hold + 1) continue;
                    if (extend) lab[(size_t)s.srcb[(size_t)i]] = -1;                 // (its in-place pre-pass)
                    if (lag && !s.flushed[(size_t)i]) lab[(size_t)s.dstb[(size_t)i]] = -2;   // (a state past the stop)
                    continue;
                }
                if (lab[(size_t)s.srcb[(size_t)i]] != s.bound[(size_t)i]) return fail("launch source", nbuf, K, budget, sw);
                lab[(size_t)s.dstb[(size_t)i]] = (long)s.bound[(size_t)i + 1];
                if (hold < 0 && s.bound[(size_t)i + 1] >= sw) hold = i;
            }
            const XinvWhere w = xinv_where(s.bound.data(), nl, s.srcb.data(), s.dstb.data(), nbuf, extend != 0, sw);
            if (w.launch != hold) return fail("launch of the stop sweep", nbuf, K, budget, sw);
            for (int64_t q = 0; q < w.f.redo; q++) {
                const int rd = xinv_redo_read(w.f.r, q), wr = xinv_redo_write(w.f.r, q);
                if (rd == wr) return fail("redo writes what it reads", nbuf, K, budget, sw);
                if (lab[(size_t)rd] != s.bound[(size_t)hold] + q) return fail("redo source", nbuf, K, budget, sw);
                lab[(size_t)wr] = lab[(size_t)rd] + 1;
            }
            if (lab[(size_t)w.f.where] != sw) return fail("final state", nbuf, K, budget, sw);
            cases++;
        }

        // watchdog recovery: the member stopped at the start of launch i (its source intact, later launches no-ops), then
        // swept one sweep at a time between that source and the launch's own output
        for (int64_t i = 0; i < nl; i++)
            for (long steps = 0; steps <= 6; steps++) {
                std::vector<long> lab((size_t)nbuf, -1);
                lab[(size_t)s.srcb[(size_t)i]] = (long)s.bound[(size_t)i];
                const XinvRedo r = xinv_redo(s.srcb[(size_t)i], s.dstb[(size_t)i], 2);
                for (long q = 0; q < steps; q++) {
                    const int rd = xinv_redo_read(r, q), wr = xinv_redo_write(r, q);
                    if (rd == wr || lab[(size_t)rd] != s.bound[(size_t)i] + q) return fail("recovery step", nbuf, K, budget, steps);
                    lab[(size_t)wr] = lab[(size_t)rd] + 1;
                }
                if (lab[(size_t)xinv_redo_result(r, steps)] != s.bound[(size_t)i] + steps)
                    return fail("recovery result", nbuf, K, budget, steps);
                cases++;
            }

        // the rolling batch: a member that joins at a launch whose source is buffer j ping-pongs from there
        if (nbuf == 2)
            for (int j = 0; j < 2; j++) {
                Solve t;
                if (!issue(t, 2, K, budget, j)) return fail("destination (start parity)", nbuf, K, budget, -1);
                for (int64_t r = 0; r < (int64_t)t.srcb.size(); r++)
                    if (t.srcb[(size_t)r] != xinv_pingpong_src(j, r) || t.dstb[(size_t)r] != xinv_pingpong_src(j, r + 1))
                        return fail("rolling batch parity", nbuf, K, budget, -1);
                cases++;
            }
    }
    std::printf("OK %ld cases\n", cases);
    return 0;
}
