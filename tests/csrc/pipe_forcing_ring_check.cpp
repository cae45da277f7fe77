// CPU check of the planner's switch between the two forcing paths of k_pipe2d, xinv_pipe_forcing_ring in
// xinvert_amd/csrc/xinv_tiles.h (built and run by tests/test_pipe_forcing_ring.py).  The switch is a size: 24 bytes per
// point of every member against XINV_PIPE_FR_BYTES.  The cases are the launches the two paths were timed on
// (profiles/pipe2d_norm_wave.txt): every one the ring won must lie above the switch, every one it lost or tied below.
#include "xinv_tiles.h"
#include <cstdio>

struct Case { const char *name; long nbatch, yc, xc; bool ring; };

int main()
{
    static const Case cases[] = {
        {"C1 360x180", 1, 180, 360, false},
        {"Poisson 900x450", 1, 450, 900, false},
        {"Poisson 1800x900", 1, 900, 1800, false},                    // 39 MB: the ring 0-1.6 % slower
        {"Gill-Matsuno 1440x720 x 4", 4, 720, 1440, true},            // 99.5 MB: the ring 3 % faster
        {"headline 3600x1800", 1, 1800, 3600, true},                  // 155.5 MB: 1.2-2.7 % faster
        {"headline, odd 3601x1800", 1, 1800, 3601, true},
        {"Gill-Matsuno 1440x720 x 8", 8, 720, 1440, true},            // 199.1 MB: below the round-3 switch of 200 MB
        {"headline x 2", 2, 1800, 3600, true},
        {"Gill-Matsuno 1440x720 x 64", 64, 720, 1440, true},
    };
    int bad = 0;
    for (const Case &c : cases)
        if (xinv_pipe_forcing_ring(c.nbatch, c.yc, c.xc) != c.ring) {
            std::printf("FAIL %s: ring %d expected %d\n", c.name, (int)xinv_pipe_forcing_ring(c.nbatch, c.yc, c.xc), (int)c.ring);
            bad++;
        }
    // the switch is monotonic in every argument and sits between the two measured sides
    if (!(XINV_PIPE_FR_BYTES > 900.0 * 1800.0 * 24.0 && XINV_PIPE_FR_BYTES < 4.0 * 720.0 * 1440.0 * 24.0)) {
        std::printf("FAIL the switch %g left the measured bracket\n", (double)XINV_PIPE_FR_BYTES);
        bad++;
    }
    for (long n = 1; n <= 64; n *= 2)
        for (long yc = 64; yc <= 4096; yc *= 2)
            for (long xc = 64; xc <= 8192; xc *= 2)
                if (xinv_pipe_forcing_ring(n, yc, xc) && !(xinv_pipe_forcing_ring(2 * n, yc, xc) && xinv_pipe_forcing_ring(n, 2 * yc, xc) &&
                                                            xinv_pipe_forcing_ring(n, yc, 2 * xc))) {
                    std::printf("FAIL not monotonic at %ld x %ld x %ld\n", n, yc, xc);
                    bad++;
                }
    if (bad) return 1;
    std::printf("OK %d cases\n", (int)(sizeof(cases) / sizeof(cases[0])));
    return 0;
}
