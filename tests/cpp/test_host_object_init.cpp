// MsckfBackend::single_object_initialization / object_initialization / levenberg_marquardt(.., initialize_on_device)
// (orcvio_amd/csrc/host/orcvio_msckf_host.hpp) as ObjectInitNode would call them: reads the cases tests/test_gpu_object_init.py wrote
// (plain text), runs each alone, all in one launch, and the one call with the optimiser behind; prints the results with 17 digits
// for the test to compare with the Python binding's.
//   file: pose_form n_objects, then per object: K F | w[4] | mean_shape 3 | mean_kps 3K | wTc 16F | zs 2KF ("nan" allowed) | bbox 4F
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

static void print(const char* tag, int k, const MsckfBackend::ObjectInit& o, bool ok) {
    std::printf("%s %d ok %d init_status %d n_used %d scale %.17g values", tag, k, ok ? 1 : 0, o.init_status, o.n_used, o.scale);
    for (double v : o.wTq) std::printf(" %.17g", v);
    for (double v : o.R_kabsch) std::printf(" %.17g", v);
    for (double v : o.t_kabsch) std::printf(" %.17g", v);
    for (double v : o.sigma) std::printf(" %.17g", v);
    for (double v : o.valid_shape_global_frame) std::printf(" %.17g", v);
    for (double v : o.kp_cond) std::printf(" %.17g", v);
    for (int v : o.kp_used) std::printf(" %d", v);
    for (int v : o.kp_obs) std::printf(" %d", v);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    MsckfBackend be(0, 8, 64, 256);
    be.object_init_pose_form = (int)next(f);
    const int n = (int)next(f);
    std::vector<MsckfBackend::ObjectFeatureTrack> feats(n);
    for (int k = 0; k < n; ++k) {
        const int K = (int)next(f), F = (int)next(f);
        for (int i = 0; i < 4; ++i) be.residual_weights[i] = next(f);
        be.object_mean_shape.assign(3, 0.0);
        for (double& v : be.object_mean_shape) v = next(f);
        be.object_keypoints_mean.assign((size_t)3 * K, 0.0);
        for (double& v : be.object_keypoints_mean) v = next(f);
        feats[k].n_keypoints = K;
        feats[k].frame_wTc.assign((size_t)16 * F, 0.0);
        for (double& v : feats[k].frame_wTc) v = next(f);
        feats[k].frame_zs.assign((size_t)2 * K * F, 0.0);
        for (double& v : feats[k].frame_zs) v = next(f);
        feats[k].frame_bbox.assign((size_t)4 * F, 0.0);
        for (double& v : feats[k].frame_bbox) v = next(f);
    }
    std::fclose(f);
    // (the objects of one file share K and the priors: the backend's members are the initializer's)
    for (int k = 0; k < n; ++k) {
        MsckfBackend::ObjectInit o;
        bool ok;
        std::array<double, 16> wTq;
        std::tie(ok, wTq) = be.single_object_initialization(feats[k], &o);
        if (o.status != ORCVIO_OK) { std::fprintf(stderr, "object_init: %s\n", orcvio_msckf_last_error()); return 1; }
        for (int i = 0; i < 16; ++i)
            if (wTq[i] != o.wTq[i]) return 1;
        print("single", k, o, ok);
    }
    std::vector<const MsckfBackend::ObjectFeatureTrack*> ptrs;
    for (auto& ft : feats) ptrs.push_back(&ft);
    std::vector<MsckfBackend::ObjectInit> all;
    if (be.object_initialization(ptrs, all) != ORCVIO_OK) { std::fprintf(stderr, "object_init: %s\n", orcvio_msckf_last_error()); return 1; }
    for (int k = 0; k < n; ++k) print("batch", k, all[k], all[k].init_status == 1);
    // the one call: the start found on the device, the optimum written back where the initialisation succeeded
    std::vector<MsckfBackend::ObjectState> states(n);
    std::vector<MsckfBackend::ObjectInit> inits;
    if (be.levenberg_marquardt(ptrs, states, true, 0, true, &inits) != ORCVIO_OK) { std::fprintf(stderr, "object_init_lm: %s\n", orcvio_msckf_last_error()); return 1; }
    for (int k = 0; k < n; ++k) {
        print("chain_init", k, inits[k], inits[k].init_status == 1);
        const MsckfBackend::ObjectState& o = states[k];
        std::printf("chain_lm %d lm_status %d iterations %d evaluations %d cost0 %.17g cost %.17g state", k, o.lm_status, o.iterations, o.evaluations, o.cost0, o.cost);
        for (double v : o.object_pose) std::printf(" %.17g", v);
        for (double v : o.ellipsoid_shape) std::printf(" %.17g", v);
        for (double v : o.object_keypoints) std::printf(" %.17g", v);
        std::printf("\n");
    }
    // a camera pose that is not a number is refused by the call
    MsckfBackend::ObjectFeatureTrack bad = feats[0];
    bad.frame_wTc[3] = std::nan("");
    MsckfBackend::ObjectInit ob;
    const bool okb = std::get<0>(be.single_object_initialization(bad, &ob));
    std::printf("refused %d status %d\n", okb ? 0 : 1, ob.status);
    // a detection vector that is not 2K numbers per frame is refused by the wrapper itself
    MsckfBackend::ObjectFeatureTrack cut = feats[0];
    cut.frame_zs.pop_back();
    const bool okc = std::get<0>(be.single_object_initialization(cut, &ob));
    std::printf("short zs refused %d status %d\n", okc ? 0 : 1, ob.status);
    std::printf("host object init ok\n");
    return 0;
}
