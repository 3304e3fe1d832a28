// TEST INFRASTRUCTURE: the strip rule and the strip gather plan of a multi-rank ground truth
// (restir-embree_amd/csrc/rs_mgpu_core.h strip_rows_of, strip_gather_plan) behind a C interface, for
// tests/test_gt_strips.py.  Host code only.
#include "../../restir-embree_amd/csrc/rs_mgpu_core.h"

#include <cstdio>
#include <cstring>

using namespace rs::mgpu;

extern "C" {

// rank r's strips as y0, y1 pairs into out (cap pairs); returns their number
int strips_of(int H, int world, int r, int32_t* out, int cap) {
    const std::vector<RowSpan> v = strip_rows_of(H, world, r);
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) { out[2 * i] = v[i].y0; out[2 * i + 1] = v[i].y1; }
    return (int)v.size();
}

// The plans of every rank of `world`: check_plans' message into msg ("" when consistent).  recv0 = the bytes rank
// 0 receives.  Returns 0, or 1 when check_plans objects, 2 when a peer's transfers are not in ascending offset order
// on some rank, 3 when a transfer is no kFrameRows transfer with rank 0 on one side, 4 when the pairing in issue
// order (what RCCL does with the sends and receives between two ranks) joins transfers of different size or place.
int strip_plan_check(int world, int H, int row_bytes, unsigned long long* recv0, char* msg, int cap) {
    std::vector<std::vector<Xfer>> plans;
    for (int r = 0; r < world; ++r) plans.push_back(strip_gather_plan(r, world, H, (size_t)row_bytes));
    const std::string e = check_plans(plans);
    std::snprintf(msg, (size_t)cap, "%s", e.c_str());
    *recv0 = plan_bytes(plans[0], false);
    if (!e.empty()) return 1;
    for (int r = 0; r < world; ++r) {
        std::vector<long long> last(world, -1);
        for (const Xfer& x : plans[r]) {
            if (x.slot != kFrameRows || (r == 0) == x.send || (r != 0 && x.peer != 0)) return 3;
            if ((long long)x.offset <= last[x.peer]) return 2;
            last[x.peer] = (long long)x.offset;
        }
    }
    for (int q = 1; q < world; ++q) {                       // k-th send of q to 0 <-> k-th recv of 0 from q
        std::vector<Xfer> rx;
        for (const Xfer& x : plans[0]) if (x.peer == q) rx.push_back(x);
        if (rx.size() != plans[q].size()) return 4;
        for (size_t k = 0; k < rx.size(); ++k)
            if (rx[k].bytes != plans[q][k].bytes || rx[k].offset != plans[q][k].offset) return 4;
    }
    return 0;
}

}  // extern "C"
