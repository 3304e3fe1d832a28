// rs_frame_ring.h -- the ring bookkeeping of frames in flight (restir_capi.hip rs_context), as plain integer
// functions: no HIP, no context, so a CPU test drives the same code (tests/cpp/frame_ring_harness.cpp via
// tests/test_frame_ring.py).
//
// Frame pipelining ("run-ahead", depth D <= kMaxAhead): frames rotate over D+1 internal "lane"
// streams, frame f running entirely on lane f mod (D+1), so up to D+1 consecutive frames are in flight
// at once: one frame's G-buffer + initial pass (which reads nothing of earlier frames) overlaps the
// previous frames' later passes, halo exchanges and gathers, and the tails of their kernels.  Only the
// temporal pass depends on the previous frame (its final reservoirs and G-buffer): it waits for that
// frame's completion event.  Each lane owns its framebuffer, ray-count slots and counters; the G ring
// holds D+2 buffers (frames f-D-1..f: a frame writes the slot after the previous frame's), the reservoir
// ring 3D+2: a frame reads `last`, the previous frame's final buffer, and writes the two lowest-numbered
// buffers that are neither `last` nor among the three (its two and its `last`) each of the D frames before
// it touches -- those may still run.  The context's stream waits for every frame's completion, so
// its semantics are those of a sequential renderer.  D = 0 runs everything on the context's stream (lane 0;
// with a framebuffer ring of 2, lanes 0 and 1 in turn, for their framebuffers only).
// Work enqueued on the context's stream between frames (geometry updates, MIS frames, sky changes)
// makes the next frame's lane wait for it.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef RS_MAX_AHEAD
#define RS_MAX_AHEAD 2
#endif

namespace rs {
constexpr int kMaxAhead = RS_MAX_AHEAD, kLanes = kMaxAhead + 1, kGRing = kMaxAhead + 2, kRRing = 3 * kMaxAhead + 2;
namespace ring {

// the lane of frame number `seq` at depth D (fb_ring: rs_context_set_frame_ring)
inline int lane_of(uint64_t seq, int D, int fb_ring) {
    return D > 0 ? (int)(seq % (uint64_t)(D + 1)) : (fb_ring == 2 ? (int)(seq & 1) : 0);
}

// Reservoir ring: `last` = the previous frame's final buffer (reservoirsLastFrame, a pointer swap,
// pg/simpleguidx11.cpp:477); this frame writes two buffers (ra < rb) none of the D frames before it touches.
// rhist = {ra, rb, last} of the previous frames, most recent first; the pick is shifted in.
inline void pick_reservoirs(int last, int D, int (&rhist)[kMaxAhead][3], int& ra, int& rb) {
    auto used = [&](int i) {
        if (i == last) return true;
        for (int g = 0; g < D; ++g)
            if (i == rhist[g][0] || i == rhist[g][1] || i == rhist[g][2]) return true;
        return false;
    };
    ra = 0;
    while (used(ra)) ++ra;
    rb = ra + 1;
    while (used(rb)) ++rb;                      // < kRRing: D frames touch <= 3D buffers, `last` among them
    for (int g = kMaxAhead - 1; g > 0; --g)
        for (int j = 0; j < 3; ++j) rhist[g][j] = rhist[g - 1][j];
    rhist[0][0] = ra; rhist[0][1] = rb; rhist[0][2] = last;
}

// G-buffer ring (replaces gBufferLastFrame.setDataFrom, pg/simpleguidx11.cpp:480): a frame writes the slot
// after the current one, which becomes the previous frame's
inline int g_next(int gcur) { return (gcur + 1) % kGRing; }

// launch grids (16x16-px workgroups of four 8x8 waves; the candidate-split pass one workgroup per 8x8 tile) and
// their waves
struct Grid { unsigned x, y; };
inline Grid grid_rows(int W, int ya, int yb) { return {(unsigned)((W + 15) / 16), (unsigned)((yb - ya + 15) / 16)}; }
inline Grid grid_split(int W, int ya, int yb) { return {(unsigned)((W + 7) / 8), (unsigned)((yb - ya + 7) / 8)}; }
inline size_t grid_waves(Grid g, int waves_per_block = 4) { return (size_t)g.x * g.y * waves_per_block; }

// ray-count slots for every launch of a frame: initial (rows gy0..gy1; `split_waves` per tile when candidate-split,
// else 0) + visibility + temporal + shade + spare (rows y0..y1, four launches' worth) + the spatial passes + extra
inline size_t count_slot_need(int W, int gy0, int gy1, int y0, int y1, int split_waves, int spatial_passes, size_t extra) {
    const size_t band = grid_waves(grid_rows(W, y0, y1));
    const size_t initial = split_waves ? grid_waves(grid_split(W, gy0, gy1), split_waves) : grid_waves(grid_rows(W, gy0, gy1));
    return initial + band * 4 + band * (size_t)(spatial_passes > 0 ? spatial_passes : 0) + extra;
}

}  // namespace ring
}  // namespace rs
