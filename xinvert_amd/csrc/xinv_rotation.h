// xinv_rotation.h -- which buffer of S a sweep launch writes and where a member's final state lives: integer rules shared
// by the sweep loop (xinv_sweep.h) and the rolling host-pointer batch (xinv_hostptr.h), and compiled on its own by the
// CPU suite (tests/test_rotation.py builds tests/csrc/rotation_check.cpp with g++ against this header).
#pragma once
#include <algorithm>
#include <cstdint>

// Launch i sweeps buf[src] into buf[dst]; src is launch i-1's dst (buffer 0, the caller's S, for launch 0).  Two buffers:
// ping-pong.  Three (lagged norm): the decision about pass i-1 arrives while pass i runs, so pass i leaves pass i-1's
// source intact (a pass the stop rule fired in is redone from it) -- a rotation.  Evaluating the pending pass first
// (`flush`: pass i is then a no-op for a member that stopped in pass i-1) lets launch i write prev_src: the rotation
// reverses.  Forward for f launches and backward for the rest of nl ends in buffer (2 f - nl) mod 3, so one reversal at
// nl - 1 (nl mod 3 == 2) or nl - 2 (nl mod 3 == 1) brings a solve that runs its budget of nl launches home to buffer 0:
// no copy back into the caller's array (52 MB at 3600x1800: ~30 us of a 4.3 ms solve).
struct XinvRot { int dst; bool flush; };
inline int64_t xinv_flip_at(bool lag, int64_t nl) { return (!lag || nl % 3 == 0) ? -1 : (nl % 3 == 2 ? nl - 1 : nl - 2); }
inline XinvRot xinv_rot_dst(int64_t i, int src, int prev_src, int nbuf, int64_t flip_at)
{
    if (nbuf == 2) return {src ^ 1, false};
    if (i == 0) return {1, false};
    return i == flip_at ? XinvRot{prev_src, true} : XinvRot{3 - src - prev_src, false};
}// The two-buffer case from buffer `start` (the rolling batch: a member joins the ping-pong at any launch).
inline int xinv_pingpong_src(int64_t start, int64_t r) { return (int)((start + r) & 1); }

// A redo sweeps one sweep at a time from a launch's intact source into the launch's own output, then back and forth
// between that and `spare`: the third buffer with three (nothing after the first step writes src), src with two.
struct XinvRedo { int src, own, spare; };
inline XinvRedo xinv_redo(int src, int own, int nbuf) { return {src, own, nbuf == 3 ? 3 - src - own : src}; }
inline int xinv_redo_read(const XinvRedo &r, int64_t q) { return q == 0 ? r.src : (q & 1) ? r.own : r.spare; }
inline int xinv_redo_write(const XinvRedo &r, int64_t q) { return (q & 1) ? r.spare : r.own; }
inline int xinv_redo_result(const XinvRedo &r, int64_t steps) { return steps == 0 ? r.src : (steps & 1) ? r.own : r.spare; }
// The state after sweep sw, in a launch of sweeps (b0, b1] from buf[src] into buf[dst]: buf[dst] if the launch ended
// there and is not `hit`, else `redo` sweeps from b0 again, ending in buf[where].
struct XinvFinal { int where; int64_t redo; XinvRedo r; };
inline XinvFinal xinv_final_in(int64_t b0, int64_t b1, int src, int dst, int nbuf, bool hit, int64_t sw)
{
    const XinvRedo r = xinv_redo(src, dst, nbuf);
    const int64_t redo = (b1 == sw && !hit) ? 0 : sw - b0;
    return {redo ? xinv_redo_result(r, redo) : dst, redo, r};
}
// The launch i of nl holding sweep sw: bound[i] < sw <= bound[i+1], bound[] ascending (-1: none).
inline int64_t xinv_launch_of(const int64_t *bound, int64_t nl, int64_t sw)
{
    const int64_t i = std::lower_bound(bound, bound + nl + 1, sw) - bound - 1;
    return (i >= 0 && i < nl) ? i : -1;
}
// Where a member that stopped at sweep sw finds its state.  The biharmonic 'extend' pre-pass works IN PLACE on its
// launch's source: with the lagged norm (`extend_lag`) the launch after i has run it on pass i's OUTPUT before the
// decision about pass i arrived (rows 0, 1, yc-2, yc-1 of a tolerance stop, found by the fuzz) -- whenever a launch
// follows, pass i is redone (`hit`: without its own pre-pass, which already ran on the source and is not idempotent in
// the periodic form).
struct XinvWhere { int64_t launch; bool hit; XinvFinal f; };
inline XinvWhere xinv_where(const int64_t *bound, int64_t nl, const signed char *srcb, const signed char *dstb, int nbuf,
                            bool extend_lag, int64_t sw)
{
    const int64_t i = xinv_launch_of(bound, nl, sw);
    if (i < 0) return {-1, false, {0, 0, {0, 0, 0}}};
    const bool hit = extend_lag && i + 1 < nl;
    return {i, hit, xinv_final_in(bound[i], bound[i + 1], srcb[i], dstb[i], nbuf, hit, sw)};
}
