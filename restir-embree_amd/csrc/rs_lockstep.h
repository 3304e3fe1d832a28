// rs_lockstep.h -- the successor rule of the lockstep walks (rs_scene.h occluded_wave_multi, occluded_wave,
// closest_wave): which node the wave steps to after node m, without a cross-lane minimum.  Plain C++ (no HIP
// types), so tests/cpp/lockstep_successor.cpp runs the same function on the host.
//
// The wave's step is m = the exact minimum of the live cursors (a cursor = a ray's next node in the preorder with
// skip pointers; a finished ray's cursor is "done", above every node).  After the step every ray that stood on m
// has moved to m + 1 (entered an interior node), to skip(m) (missed the box, or left a leaf) or to done (an any-hit
// ray that found its occluder in the leaf).
//
// Lemma.  Every cursor c != m satisfies c >= skip(m).
// Proof.  A cursor is 0, x + 1 for an entered interior node x, or skip(x), for some x stepped earlier; steps
// increase, so x < m.  Suppose m < c < skip(m).  c = x + 1 would need x >= m.  c = skip(x) with x < m: preorder
// subtrees are nested or disjoint, so either m lies in subtree(x) and skip(x) >= skip(m), or subtree(x) ends
// before m and skip(x) <= m.  Neither lies in (m, skip(m)).  []
//
// Hence the next minimum is
//   m + 1     if any ray entered the interior node m (the entering rays stand there, everything else is >= it);
//   skip(m)   at an interior node nobody entered: the rays on m move there and the rest are already >= it;
//   skip(m)   (= m + 1) after a leaf, if at least one ray on m goes on;
//   unknown   only when every ray on a leaf ended there: the rule answers kLockstepReduce and the caller takes
//             the minimum over the wave (wave_min_full / wave_min_partial).
// A closest-hit walk never ends a ray at a leaf, so it never reduces; the first step is node 0 if any ray is live.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_LOCKSTEP_HD __host__ __device__
#else
#define RS_LOCKSTEP_HD
#endif

namespace rs {

constexpr uint32_t kLockstepDone = 0xffffffffu;     // a finished (or never started) ray's cursor
constexpr uint32_t kLockstepReduce = 0xfffffffeu;   // "take the minimum of the cursors": no node has this index

// leaf: node m is a leaf; any_descended: some ray on m entered it (interior m only); any_survivor: some ray on m
// goes on to skip(m) (leaf m only; a ray on m that missed the leaf's box counts).  All arguments wave-uniform.
RS_LOCKSTEP_HD inline uint32_t lockstep_next(bool leaf, bool any_descended, bool any_survivor, uint32_t m,
                                             uint32_t skip) {
    if (!leaf) return any_descended ? m + 1u : skip;
    return any_survivor ? skip : kLockstepReduce;
}
// the first step: every live cursor starts at node 0
RS_LOCKSTEP_HD inline uint32_t lockstep_first(bool any_live) { return any_live ? 0u : kLockstepDone; }

}  // namespace rs
