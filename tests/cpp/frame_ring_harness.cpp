// TEST INFRASTRUCTURE: C entry points over restir-embree_amd/csrc/rs_frame_ring.h for tests/test_frame_ring.py, and
// (with -DFRAME_RING_MAIN) a stand-alone program that walks the same rings under a sanitizer.
#include "../../restir-embree_amd/csrc/rs_frame_ring.h"

#include <cstdio>

using namespace rs;

struct RingState {
    int r_last = 2;
    int rhist[kMaxAhead][3];
    int gcur = 0;
    uint64_t seq = 0;
    RingState() { for (auto& h : rhist) h[0] = h[1] = h[2] = -1; }   // as rs_context_create leaves them
};

extern "C" {
int fr_max_ahead() { return kMaxAhead; }
int fr_rring() { return kRRing; }
int fr_gring() { return kGRing; }
RingState* fr_new() { return new RingState(); }
void fr_free(RingState* s) { delete s; }
// begin one frame at depth D: out = {lane, ra, rb, last, gnew, gprev}
void fr_begin(RingState* s, int D, int fb_ring, int* out) {
    out[0] = ring::lane_of(s->seq++, D, fb_ring);
    out[3] = s->r_last;
    ring::pick_reservoirs(s->r_last, D, s->rhist, out[1], out[2]);
    out[5] = s->gcur;
    out[4] = s->gcur = ring::g_next(s->gcur);
}
// finish it: its final reservoirs are buffer `rcur` (one of its two)
void fr_finish(RingState* s, int rcur) { s->r_last = rcur; }
void fr_grid(int W, int ya, int yb, unsigned* out) {
    const ring::Grid r = ring::grid_rows(W, ya, yb), p = ring::grid_split(W, ya, yb);
    out[0] = r.x; out[1] = r.y; out[2] = p.x; out[3] = p.y;
}
unsigned long long fr_grid_waves(unsigned x, unsigned y, int wpb) { return ring::grid_waves({x, y}, wpb); }
unsigned long long fr_count_slot_need(int W, int gy0, int gy1, int y0, int y1, int split_waves, int passes,
                                      unsigned long long extra) {
    return ring::count_slot_need(W, gy0, gy1, y0, y1, split_waves, passes, (size_t)extra);
}
}

#ifdef FRAME_RING_MAIN
int main() {
    uint32_t rng = 12345u;
    auto rnd = [&](uint32_t n) { rng = rng * 1664525u + 1013904223u; return (rng >> 8) % n; };
    for (int D0 = 0; D0 <= kMaxAhead; ++D0) {
        RingState* s = fr_new();
        int D = D0, prev[kMaxAhead + 1][3], nprev = 0, final_prev = 2;
        for (int f = 0; f < 4000; ++f) {
            if (rnd(97) == 0) D = (int)rnd(kMaxAhead + 1);
            int o[6];
            fr_begin(s, D, 1 + (int)rnd(2), o);
            bool ok = o[1] != o[2] && o[1] >= 0 && o[2] >= 0 && o[1] < kRRing && o[2] < kRRing && o[3] == final_prev &&
                      o[1] != o[3] && o[2] != o[3] && o[0] >= 0 && o[0] < kLanes && o[4] != o[5] && o[4] < kGRing;
            for (int g = 0; g < D && g < nprev; ++g)
                for (int j = 0; j < 3; ++j) ok = ok && o[1] != prev[g][j] && o[2] != prev[g][j];
            if (!ok) { std::printf("frame %d depth %d: bad pick %d %d last %d\n", f, D, o[1], o[2], o[3]); return 1; }
            for (int g = kMaxAhead; g > 0; --g) for (int j = 0; j < 3; ++j) prev[g][j] = prev[g - 1][j];
            prev[0][0] = o[1]; prev[0][1] = o[2]; prev[0][2] = o[3];
            if (nprev < kMaxAhead + 1) ++nprev;
            final_prev = rnd(2) ? o[1] : o[2];
            fr_finish(s, final_prev);
        }
        fr_free(s);
    }
    unsigned g[4];
    fr_grid(1920, 0, 1080, g);
    std::printf("frame_ring: ok (1080p grid %ux%u, %llu slots)\n", g[0], g[1], fr_count_slot_need(1920, 0, 1080, 0, 1080, 0, 2, 0));
    return 0;
}
#endif
