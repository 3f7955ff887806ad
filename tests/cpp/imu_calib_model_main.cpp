// imu_calib_model_main.cpp -- the leg_dim = 46 host build of orcvio_amd/csrc/host/imu_model.hpp as a stand-alone program
// (tests/test_imu_calib_model_host.py builds it under AddressSanitizer + UndefinedBehaviorSanitizer and compares its output with
// tests/mirror_imu_calib.py).
//   imu_calib_model_main CASE    reads a case, prints the batch info, the propagated state, the per-sample records and the accumulated pair
// CASE (text, whitespace separated): intrinsics 24 (T1 T2 T3 A1 A2 A3 M1 M2) | then as imu_model_main.cpp:
//   use_larvio use_left use_closed_form if_fej | gravity 3 | imu_img_timeTh | Q_c diagonal 12 |
//   time R 9 v 3 p 3 b_g 3 b_a 3 v_fej 3 p_fej 3 | prev_meas 6 | time_bound | n | n rows of t gyro 3 acc 3
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
    if (argc < 2) { fprintf(stderr, "usage: imu_calib_model_main CASE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    double x[IMU_NI], fl[4], Qc[12], st0[28], prev[6], tb, nn;
    ImuModelConfig c{};
    bool ok = rd(f, x, IMU_NI) && rd(f, fl, 4) && rd(f, c.gravity, 3) && rd(f, &c.imu_img_time_th, 1) && rd(f, Qc, 12) && rd(f, st0, 28) &&
              rd(f, prev, 6) && rd(f, &tb, 1) && rd(f, &nn, 1);
    const int n = ok ? (int)nn : 0;
    std::vector<double> samples((size_t)n * 7);
    ok = ok && rd(f, samples.data(), n * 7);
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    c.flags = ImuFlags{(int)fl[0], (int)fl[1], (int)fl[2], (int)fl[3]};
    ImuMeanState st;
    {
        const double* p = st0;
        st.time = *p++;
        for (int i = 0; i < 9; ++i) st.R[i] = *p++;
        for (int i = 0; i < 3; ++i) st.v[i] = *p++;
        for (int i = 0; i < 3; ++i) st.p[i] = *p++;
        for (int i = 0; i < 3; ++i) st.bg[i] = *p++;
        for (int i = 0; i < 3; ++i) st.ba[i] = *p++;
        for (int i = 0; i < 3; ++i) st.v_fej[i] = *p++;
        for (int i = 0; i < 3; ++i) st.p_fej[i] = *p++;
    }
    ImuIntrinsicMx mx;
    imu_intrinsic_mx(x, &mx);
    pr("Tg", mx.Tg, 9); pr("As", mx.As, 9); pr("Ma", mx.Ma, 9);
    std::vector<double> recs((size_t)IMU_MAX_SAMPLES * IMU_REC46);
    std::vector<double> Phi(IMU_LEG46 * IMU_LEG46), Q(IMU_LEG46 * IMU_LEG46);
    ImuBatchInfo info{};
    if (!imu_propagate_mean46(c, mx, &st, prev, samples.data(), n, tb, recs.data(), IMU_MAX_SAMPLES, &info)) {
        printf("capacity %d %d\n", info.n_used, info.n_propagated);
        return 0;
    }
    const int S = info.n_propagated;
    imu_accumulate_host46(recs.data(), S, c.flags, c.gravity, Qc, mx, Phi.data(), Q.data());
    printf("info %d %d %.17g %.17g %.17g %.17g\n", info.n_used, info.n_propagated, info.dt, info.mean_sforce[0], info.mean_sforce[1], info.mean_sforce[2]);
    printf("time %.17g\n", st.time);
    pr("R", st.R, 9); pr("v", st.v, 3); pr("p", st.p, 3); pr("v_fej", st.v_fej, 3); pr("p_fej", st.p_fej, 3); pr("prev", prev, 6);
    for (int k = 0; k < S; ++k) pr("rec", recs.data() + (size_t)k * IMU_REC46, IMU_REC46);
    pr("Phi", Phi.data(), Phi.size());
    pr("Q", Q.data(), Q.size());
    printf("imu calib model ok\n");
    return 0;
}
