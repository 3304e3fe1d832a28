// TEST INFRASTRUCTURE: runs the RCCL branch of rs_mgpu_render_ground_truth (csrc/rs_mgpu.hip: every rank's strips on
// its context's stream, then one ncclSend / ncclRecv group per rank with one transfer per strip) with `world` ranks as
// threads of one process on one GPU, linked against tests/cpp/rccl_stub.cpp instead of librccl (as
// mgpu_rccl_driver.cpp does for the ReSTIR frames), and checks every gathered frame bit for bit against one context
// rendering the same frames.  The stub pairs the sends and receives between two ranks in issue order and counts a
// pair of unequal sizes as a mismatch: the strips' order on both sides is under test.
//   mgpu_gt_rccl_driver <scene.obj> W H world frames spp bounces eye(3) at(3) fov
// Estimators: the reference's path tracer and the unbiased one, `frames` frames each.  Prints one JSON line; exit 0
// iff every frame is identical and the stub saw no unpaired / mismatched transfer.
#include "../../include/restir.hpp"

#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

extern "C" void rccl_stub_stats(long* pairs, long* bytes, long* mismatches, long* unpaired, long* allreduces);

int main(int argc, char** argv) {
    if (argc < 15) { std::fprintf(stderr, "usage: %s obj W H world frames spp bounces ex ey ez ax ay az fov\n", argv[0]); return 2; }
    const char* obj = argv[1];
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), world = std::atoi(argv[4]), frames = std::atoi(argv[5]);
    const uint32_t spp = (uint32_t)std::atoi(argv[6]);
    const rs_path_params pp{std::atoi(argv[7]), 1, 1, 1};
    restir::Camera cam(std::atof(argv[8]), std::atof(argv[9]), std::atof(argv[10]), std::atof(argv[11]), std::atof(argv[12]),
                       std::atof(argv[13]), std::atof(argv[14]));
    restir::Params P;
    const int estimators[2] = {RS_GT_PATH, RS_GT_PATH_UNBIASED};
    const size_t px = (size_t)W * H * 3;
    std::vector<std::vector<float>> ref;                    // [estimator * frames + frame]
    try {
        restir::Renderer r(W, H);
        r.LoadScene(obj);
        r.camera_ = cam;
        r.params = P;
        r.pathParams = pp;
        r.samplesPerPixel = spp;
        r.timePasses = false;
        for (int e = 0; e < 2; ++e) {
            r.unbiasedEstimator = estimators[e] == RS_GT_PATH_UNBIASED;
            r.frameCtr = 0;
            for (int k = 0; k < frames; ++k) {
                r.produceStandard();
                ref.emplace_back(r.frame_data(), r.frame_data() + px);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "reference: %s\n", e.what());
        return 1;
    }
    std::vector<restir::Renderer*> rk;
    for (int i = 0; i < world; ++i) {
        rk.push_back(new restir::Renderer(W, H));
        rk.back()->LoadScene(obj);
    }
    uint8_t id[RS_MGPU_ID_BYTES];
    if (rs_mgpu_unique_id(id) != RS_OK) { std::fprintf(stderr, "unique id\n"); return 1; }
    std::vector<int> fail(world, 0);
    std::vector<std::string> msg(world);
    int bad_frames = 0;
    unsigned long long gather_bytes = 0;
    std::barrier sync(world);
    auto run = [&](int i) {
        rs_mgpu* m = nullptr;
        auto chk = [&](int rc, const char* what) {
            if (rc != RS_OK && !fail[i]) { fail[i] = rc; msg[i] = std::string(what) + ": " + rs_last_error(rk[i]->handle()); }
            return rc == RS_OK;
        };
        if (!chk(rs_mgpu_create(rk[i]->handle(), i, world, id, &m), "rs_mgpu_create")) { sync.arrive_and_drop(); return; }
        const rs_scene* s = rk[i]->scene_handle();
        std::vector<float> host(i == 0 ? px : 0);
        for (int e = 0; e < 2 && !fail[i]; ++e)
            for (int k = 0; k < frames; ++k) {
                if (!chk(rs_mgpu_render_ground_truth(m, &s, &cam, &P, estimators[e], &pp, (uint32_t)k, spp, 1,
                                                     i == 0 ? host.data() : nullptr, nullptr), "render_ground_truth"))
                    break;
                if (i == 0 && std::memcmp(host.data(), ref[(size_t)e * frames + k].data(), px * sizeof(float)) != 0) ++bad_frames;
            }
        rs_mgpu_stats st{};
        chk(rs_mgpu_get_stats(m, &st, 0), "stats");
        if (i == 0) gather_bytes = st.gather_bytes;
        sync.arrive_and_wait();                 // nobody tears down a communicator a peer still uses
        rs_mgpu_destroy(m);
    };
    std::vector<std::thread> th;
    for (int i = 0; i < world; ++i) th.emplace_back(run, i);
    for (auto& t : th) t.join();
    long pairs, bytes, mism, unp, ar;
    rccl_stub_stats(&pairs, &bytes, &mism, &unp, &ar);
    int nfail = 0;
    for (int i = 0; i < world; ++i) if (fail[i]) { ++nfail; std::fprintf(stderr, "rank %d: %s\n", i, msg[i].c_str()); }
    std::printf("{\"world\": %d, \"frames\": %d, \"bad_frames\": %d, \"rank_errors\": %d, \"pairs\": %ld, \"bytes\": %ld, "
                "\"mismatches\": %ld, \"unpaired\": %ld, \"gather_bytes\": %llu}\n",
                world, 2 * frames, bad_frames, nfail, pairs, bytes, mism, unp, gather_bytes);
    for (auto* r : rk) delete r;
    return (bad_frames || nfail || mism || unp || pairs == 0) ? 1 : 0;
}
