// imu_model_main.cpp -- the host build of orcvio_amd/csrc/host/imu_model.hpp as a stand-alone program (tests/test_imu_model_host.py
// builds it under AddressSanitizer + UndefinedBehaviorSanitizer and compares its output with tests/mirror_imu.py).
//   imu_model_main CASE          reads a case, prints the batch info, the propagated state, per-sample Phi_k / Q_k and the accumulated pair
//   imu_model_main CASE REPS     prints the median wall time (ns) of mean propagation + accumulation over REPS repetitions
// CASE (text, whitespace separated): use_larvio use_left use_closed_form if_fej | gravity 3 | imu_img_timeTh | Q_c diagonal 12 |
//   time R 9 v 3 p 3 b_g 3 b_a 3 v_fej 3 p_fej 3 | prev_meas 6 | time_bound | n | n rows of t gyro 3 acc 3
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orcvio_amd/csrc/host/imu_model.hpp"

using namespace orcvio_amd;

static bool rd(FILE* f, double* x, int n) {
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%lf", x + i) != 1) return false;
    return true;
}
static void pr(const char* tag, const double* x, size_t n) {
    printf("%s", tag);
    for (size_t i = 0; i < n; ++i) printf(" %.17g", x[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: imu_model_main CASE [REPS]\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    double fl[4], Qc[12], st0[28], prev0[6], tb, nn;
    ImuModelConfig c{};
    bool ok = rd(f, fl, 4) && rd(f, c.gravity, 3) && rd(f, &c.imu_img_time_th, 1) && rd(f, Qc, 12) && rd(f, st0, 28) && rd(f, prev0, 6) &&
              rd(f, &tb, 1) && rd(f, &nn, 1);
    const int n = ok ? (int)nn : 0;
    std::vector<double> samples((size_t)n * 7);
    ok = ok && rd(f, samples.data(), n * 7);
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    c.flags = ImuFlags{(int)fl[0], (int)fl[1], (int)fl[2], (int)fl[3]};
    auto load_state = [&](ImuMeanState* s) {
        const double* p = st0;
        s->time = *p++;
        for (int i = 0; i < 9; ++i) s->R[i] = *p++;
        for (int i = 0; i < 3; ++i) s->v[i] = *p++;
        for (int i = 0; i < 3; ++i) s->p[i] = *p++;
        for (int i = 0; i < 3; ++i) s->bg[i] = *p++;
        for (int i = 0; i < 3; ++i) s->ba[i] = *p++;
        for (int i = 0; i < 3; ++i) s->v_fej[i] = *p++;
        for (int i = 0; i < 3; ++i) s->p_fej[i] = *p++;
    };
    std::vector<double> recs((size_t)IMU_MAX_SAMPLES * IMU_REC);
    std::vector<double> Phi(IMU_LEG * IMU_LEG), Q(IMU_LEG * IMU_LEG);
    ImuMeanState st;
    ImuBatchInfo info{};
    double prev[6];
    if (argc > 2) {
        const int reps = std::max(1, atoi(argv[2]));
        std::vector<double> ns;
        for (int r = 0; r < reps; ++r) {
            load_state(&st);
            for (int i = 0; i < 6; ++i) prev[i] = prev0[i];
            const auto t0 = std::chrono::steady_clock::now();
            if (!imu_propagate_mean(c, &st, prev, samples.data(), n, tb, recs.data(), IMU_MAX_SAMPLES, &info)) return 3;
            imu_accumulate_host(recs.data(), info.n_propagated, c.flags, c.gravity, Qc, Phi.data(), Q.data());
            const auto t1 = std::chrono::steady_clock::now();
            ns.push_back(std::chrono::duration<double, std::nano>(t1 - t0).count());
        }
        std::sort(ns.begin(), ns.end());
        printf("median_ns %.1f samples %d checksum %.17g\n", ns[ns.size() / 2], info.n_propagated, Phi[3 * IMU_LEG] + Q[0]);
        return 0;
    }
    load_state(&st);
    for (int i = 0; i < 6; ++i) prev[i] = prev0[i];
    if (!imu_propagate_mean(c, &st, prev, samples.data(), n, tb, recs.data(), IMU_MAX_SAMPLES, &info)) {
        printf("capacity %d %d\n", info.n_used, info.n_propagated);
        return 0;
    }
    const int S = info.n_propagated;
    std::vector<double> Pk((size_t)S * IMU_DIM * IMU_DIM), Qk((size_t)S * IMU_DIM * IMU_DIM);
    imu_accumulate_host(recs.data(), S, c.flags, c.gravity, Qc, Phi.data(), Q.data(), Pk.data(), Qk.data());
    printf("info %d %d %.17g %.17g %.17g %.17g\n", info.n_used, info.n_propagated, info.dt, info.mean_sforce[0], info.mean_sforce[1], info.mean_sforce[2]);
    printf("time %.17g\n", st.time);
    pr("R", st.R, 9); pr("v", st.v, 3); pr("p", st.p, 3); pr("v_fej", st.v_fej, 3); pr("p_fej", st.p_fej, 3); pr("prev", prev, 6);
    for (int k = 0; k < S; ++k) {
        pr("rec", recs.data() + (size_t)k * IMU_REC, IMU_REC);
        pr("phik", Pk.data() + (size_t)k * IMU_DIM * IMU_DIM, IMU_DIM * IMU_DIM);
        pr("qk", Qk.data() + (size_t)k * IMU_DIM * IMU_DIM, IMU_DIM * IMU_DIM);
    }
    pr("Phi", Phi.data(), Phi.size());
    pr("Q", Q.data(), Q.size());
    printf("imu model ok\n");
    return 0;
}
