// TEST INFRASTRUCTURE (tests/test_lockstep_successor.py): the lockstep walks' wave automaton on random preorder
// skip trees, run twice per case -- with the exact minimum of the cursors at every step, and with the successor
// rule of restir-embree_amd/csrc/rs_lockstep.h (the function the GPU walks call).  Both runs must visit the same
// nodes in the same order and end every ray the same way, and the rule may ask for a reduction only after a leaf
// step on which every ray on the node ended.  Stand-alone: g++ -std=c++17 lockstep_successor.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../restir-embree_amd/csrc/rs_lockstep.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

// preorder tree: skip[i] = index after i's subtree, leaf[i]; an interior node's first child is i + 1
struct Tree {
    std::vector<uint32_t> skip;
    std::vector<uint8_t> leaf;
};
enum Shape { RANDOM, CHAIN, FULL };

void grow(Tree& t, Rng& r, uint32_t count, Shape shape) {   // a subtree of exactly `count` nodes
    const uint32_t i = (uint32_t)t.skip.size();
    t.skip.push_back(i + count);
    t.leaf.push_back(count == 1);
    uint32_t rest = count - 1;
    if (rest == 0) return;
    if (shape == CHAIN) { grow(t, r, rest, shape); return; }
    if (shape == FULL) {
        if (rest == 1) { grow(t, r, 1, shape); return; }
        grow(t, r, rest - rest / 2, shape);
        grow(t, r, rest / 2, shape);
        return;
    }
    uint32_t kids = 1 + r.below(3);                          // 1..3 children
    if (kids > rest) kids = rest;
    for (uint32_t k = 0; k < kids; ++k) {
        const uint32_t left = kids - 1 - k;                  // children still to come, one node each at least
        const uint32_t c = left == 0 ? rest : 1 + r.below(rest - left);
        grow(t, r, c, shape);
        rest -= c;
    }
}

uint32_t hash3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA6Bu ^ (c + 0x165667B1u) * 0xC2B2AE35u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}

struct Case {
    Tree t;
    uint32_t rays, seed;
    std::vector<uint8_t> active;
    uint32_t p_hit, p_end;                                   // of 256
};
struct Run {
    std::vector<uint32_t> visited;                           // the wave's steps
    std::vector<uint32_t> ended_at;                          // per ray: the leaf it ended in, or kLockstepDone
    uint32_t reductions = 0;
};
struct Counts { long cases = 0, steps = 0, descend = 0, interior_skip = 0, leaf = 0, reductions = 0; };

uint32_t exact_min(const std::vector<uint32_t>& cur) {
    uint32_t m = rs::kLockstepDone;
    for (uint32_t c : cur) m = c < m ? c : m;
    return m;
}

// rule = false: the minimum at every step; true: rs::lockstep_next, the minimum only when it says so
bool run(const Case& c, bool rule, Run& out, Counts* cnt, char* msg, size_t msg_n) {
    const uint32_t n = (uint32_t)c.t.skip.size();
    std::vector<uint32_t> cur(c.rays);
    bool any = false;
    for (uint32_t r = 0; r < c.rays; ++r) {
        cur[r] = c.active[r] ? 0u : rs::kLockstepDone;
        any |= c.active[r] != 0;
    }
    out.ended_at.assign(c.rays, rs::kLockstepDone);
    uint32_t m = rule ? rs::lockstep_first(any) : exact_min(cur);
    while (m < n) {
        if (out.visited.size() > n) { snprintf(msg, msg_n, "more steps than nodes"); return false; }
        out.visited.push_back(m);
        const bool leaf = c.t.leaf[m] != 0;
        const uint32_t skip = c.t.skip[m];
        uint32_t on = 0, ended = 0, descended = 0;
        for (uint32_t r = 0; r < c.rays; ++r) {
            if (cur[r] != m) continue;
            ++on;
            const uint32_t h = hash3(r, m, c.seed);
            const bool hit = (h & 0xffu) < c.p_hit;
            if (!leaf) {
                cur[r] = hit ? m + 1 : skip;
                descended += hit;
            } else if (hit && ((h >> 8) & 0xffu) < c.p_end) {
                cur[r] = rs::kLockstepDone;
                out.ended_at[r] = m;
                ++ended;
            } else {
                cur[r] = skip;
            }
        }
        const uint32_t want = exact_min(cur);
        if (!rule) { m = want; continue; }
        if (on == 0) { snprintf(msg, msg_n, "step %u with no ray on it", m); return false; }
        uint32_t next = rs::lockstep_next(leaf, descended != 0, ended < on, m, skip);
        const bool all_ended_leaf = leaf && ended == on;
        if ((next == rs::kLockstepReduce) != all_ended_leaf) {
            snprintf(msg, msg_n, "node %u (leaf %d, %u on it, %u ended): reduce sentinel %s", m, (int)leaf, on, ended,
                     all_ended_leaf ? "missing" : "returned");
            return false;
        }
        if (next == rs::kLockstepReduce) { next = want; ++out.reductions; }
        if (next != want && !(next >= n && want >= n)) {
            snprintf(msg, msg_n, "after node %u: rule says %u, the minimum is %u", m, next, want);
            return false;
        }
        if (cnt) {
            ++cnt->steps;
            if (leaf) ++cnt->leaf; else if (descended) ++cnt->descend; else ++cnt->interior_skip;
        }
        m = next;
    }
    return true;
}

bool check(const Case& c, Counts& cnt, const char* what) {
    Run a, b;
    char msg[200] = "";
    if (!run(c, false, a, nullptr, msg, sizeof msg) || !run(c, true, b, &cnt, msg, sizeof msg)) {
        fprintf(stderr, "FAIL %s: %u nodes, %u rays, seed %u, p_hit %u p_end %u: %s\n", what, (unsigned)c.t.skip.size(),
                c.rays, c.seed, c.p_hit, c.p_end, msg);
        return false;
    }
    if (a.visited != b.visited || a.ended_at != b.ended_at) {
        fprintf(stderr, "FAIL %s: %u nodes, %u rays, seed %u: visited sequences or outcomes differ (%zu / %zu steps)\n", what,
                (unsigned)c.t.skip.size(), c.rays, c.seed, a.visited.size(), b.visited.size());
        return false;
    }
    ++cnt.cases;
    cnt.reductions += b.reductions;
    return true;
}

}  // namespace

int main() {
    Rng r{12345};
    Counts cnt;
    const uint32_t p_ends[3] = {0, 128, 256};
    const uint32_t p_hits[4] = {0, 96, 192, 256};
    uint32_t seed = 1;
    for (int shape = RANDOM; shape <= FULL; ++shape) {
        for (int rep = 0; rep < 40; ++rep) {
            // sizes: 1 (a single-leaf root), 2, 3, then random up to 300, 300 itself
            const uint32_t nodes = rep == 0 ? 1 : rep == 1 ? 2 : rep == 2 ? 3 : rep == 3 ? 300 : 1 + r.below(300);
            Case c;
            grow(c.t, r, nodes, (Shape)shape);
            if (c.t.skip.size() != nodes || c.t.skip[0] != nodes) { fprintf(stderr, "FAIL: tree generator\n"); return 2; }
            for (uint32_t pe : p_ends) {
                for (uint32_t ph : p_hits) {
                    for (int inact = 0; inact < 3; ++inact) {   // all rays live; some inactive; none live
                        c.rays = rep % 5 == 0 ? 1 : rep % 5 == 1 ? 128 : rep % 5 == 2 ? 64 : 1 + r.below(128);
                        c.seed = seed++;
                        c.p_hit = ph; c.p_end = pe;
                        c.active.assign(c.rays, 1);
                        if (inact == 1) for (auto& x : c.active) x = r.below(3) != 0;
                        if (inact == 2) for (auto& x : c.active) x = 0;
                        if (!check(c, cnt, shape == RANDOM ? "random" : shape == CHAIN ? "chain" : "full")) return 1;
                    }
                }
            }
        }
    }
    printf("ok cases=%ld steps=%ld descend=%ld interior_skip=%ld leaf=%ld reductions=%ld\n", cnt.cases, cnt.steps,
           cnt.descend, cnt.interior_skip, cnt.leaf, cnt.reductions);
    return 0;
}
