// MsckfBackend::single_object_initialization_lite / single_levenberg_marquardt_lite / levenberg_marquardt_lite
// (orcvio_amd/csrc/host/orcvio_msckf_host.hpp) as ObjectInitNode's bbox-only branch would call them: reads the cases
// tests/test_gpu_object_lite_host.py wrote (plain text), runs each alone, all in one launch, and all in one launch with the start
// found on the device; prints the results with 17 digits for the test to compare with the Python binding's.
//   file: n_objects, then per object: F left new_bbox | w[2] | mean_shape 3 | pose 16 | wTc 16F | bbox 4F
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../orcvio_amd/csrc/host/orcvio_msckf_host.hpp"

using namespace orcvio_amd;

static double next(FILE* f) {
    char buf[64];
    if (std::fscanf(f, "%63s", buf) != 1) { std::fprintf(stderr, "short file\n"); std::exit(2); }
    return std::strtod(buf, nullptr);
}

static void print(const char* tag, int k, const MsckfBackend::ObjectState& o, bool ok) {
    std::printf("%s %d ok %d lm_status %d iterations %d evaluations %d cost0 %.17g cost %.17g state", tag, k, ok ? 1 : 0, o.lm_status,
                o.iterations, o.evaluations, o.cost0, o.cost);
    for (double v : o.object_pose) std::printf(" %.17g", v);
    for (double v : o.ellipsoid_shape) std::printf(" %.17g", v);
    std::printf(" kps %d\n", (int)o.object_keypoints.size());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    const int n = (int)next(f);
    MsckfBackend be(0, 8, 64, 256);
    be.object_lm_max_iter = 400;
    std::vector<MsckfBackend::ObjectFeatureTrack> feats(n);
    std::vector<MsckfBackend::ObjectState> starts(n);
    int left = 1, new_bbox = 0;
    for (int k = 0; k < n; ++k) {
        const int F = (int)next(f);
        left = (int)next(f); new_bbox = (int)next(f);
        for (int i = 0; i < 2; ++i) be.residual_weights[i] = next(f);
        be.object_mean_shape.assign(3, 0.0);
        for (double& v : be.object_mean_shape) v = next(f);
        for (double& v : starts[k].object_pose) v = next(f);
        feats[k].n_keypoints = 0;
        feats[k].frame_wTc.assign((size_t)16 * F, 0.0);
        for (double& v : feats[k].frame_wTc) v = next(f);
        feats[k].frame_bbox.assign((size_t)4 * F, 0.0);
        for (double& v : feats[k].frame_bbox) v = next(f);
    }
    std::fclose(f);
    // (the objects of one file share the prior and the flags: the backend's members are the initializer's)
    for (int k = 0; k < n; ++k) {
        MsckfBackend::ObjectState o = starts[k];
        const bool ok = be.single_levenberg_marquardt_lite(feats[k], o, left != 0, new_bbox);
        if (o.status != ORCVIO_OK) { std::fprintf(stderr, "object_lm_lite: %s\n", orcvio_msckf_last_error()); return 1; }
        print("single", k, o, ok);
        MsckfBackend::ObjectInitLite init;
        auto [iok, wTq] = be.single_object_initialization_lite(feats[k], &init);
        if (init.status != ORCVIO_OK) { std::fprintf(stderr, "object_init_lite: %s\n", orcvio_msckf_last_error()); return 1; }
        std::printf("init %d ok %d status %d d %.17g pose", k, iok ? 1 : 0, init.init_status, init.d);
        for (double v : wTq) std::printf(" %.17g", v);
        std::printf("\n");
    }
    std::vector<const MsckfBackend::ObjectFeatureTrack*> ptrs;
    for (auto& ft : feats) ptrs.push_back(&ft);
    std::vector<MsckfBackend::ObjectState> all = starts;
    if (be.levenberg_marquardt_lite(ptrs, all, left != 0, new_bbox) != ORCVIO_OK) { std::fprintf(stderr, "object_lm_lite: %s\n", orcvio_msckf_last_error()); return 1; }
    for (int k = 0; k < n; ++k) print("batch", k, all[k], all[k].lm_status == 1);
    std::vector<MsckfBackend::ObjectState> dev(n);
    std::vector<MsckfBackend::ObjectInitLite> inits;
    if (be.levenberg_marquardt_lite(ptrs, dev, left != 0, new_bbox, true, &inits) != ORCVIO_OK) { std::fprintf(stderr, "object_init_lm_lite: %s\n", orcvio_msckf_last_error()); return 1; }
    for (int k = 0; k < n; ++k) { print("chain", k, dev[k], dev[k].lm_status == 1); std::printf("chaininit %d status %d d %.17g\n", k, inits[k].init_status, inits[k].d); }
    // a start that is not a number is refused by the call, the state untouched
    MsckfBackend::ObjectState bad = starts[0];
    bad.object_pose[3] = std::nan("");
    const bool ok = be.single_levenberg_marquardt_lite(feats[0], bad, left != 0, new_bbox);
    std::printf("refused %d status %d\n", ok ? 0 : 1, bad.status);
    // a bbox vector that is not four numbers per frame is refused by the wrapper itself (it would silently drop a frame otherwise)
    MsckfBackend::ObjectFeatureTrack cut = feats[0];
    cut.frame_bbox.pop_back();
    MsckfBackend::ObjectState st = starts[0];
    const bool ok2 = be.single_levenberg_marquardt_lite(cut, st, left != 0, new_bbox);
    std::printf("short bbox refused %d status %d\n", ok2 ? 0 : 1, st.status);
    std::printf("host object lite ok\n");
    return 0;
}
