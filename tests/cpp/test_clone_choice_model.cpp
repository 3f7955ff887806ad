// Stand-alone program over host/clone_choice_model.hpp (the arithmetic k_clone_choice runs), built by tests/test_clone_choice_mirror.py
// with -fsanitize=address,undefined.
//   no argument     edge inputs: the four result sets at N = 6 (the smallest window), identical records, a half turn (the quaternion's
//                   trace <= 0 branches), the possible-set predicate; prints "clone choice model ok"
//   <file>          a case: N rot_thr trans_thr tracking_ok pred0 pred1 from_body, then either cam records [N][12] (from_body = 0) or
//                   body poses [N][12] (R_b2w 9 | t_b_w 3) followed by the extrinsic R 9 | t 3 (from_body = 1: clone_choice_cam_pose);
//                   prints evaluated agree chosen[2] compared[2] taken[2] angle[2] distance[2]
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "../../orcvio_amd/csrc/host/clone_choice_model.hpp"

using namespace orcvio_amd;

static int fail(const char* what) { std::printf("FAILED: %s\n", what); return 1; }

static void rot_z(double a, double* R) {
    const double c = std::cos(a), s = std::sin(a);
    const double M[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) R[i] = M[i];
}

static int edge_inputs() {
    const int N = CLONE_CHOICE_MIN_N;
    std::vector<double> cam((size_t)N * CLONE_CHOICE_CAM);
    // clone c: a turn of 0.1 c about z, 1 m per clone along x
    for (int c = 0; c < N; ++c) { rot_z(0.1 * c, &cam[(size_t)c * 12]); cam[(size_t)c * 12 + 9] = c; cam[(size_t)c * 12 + 10] = 0; cam[(size_t)c * 12 + 11] = 0; }
    struct { double rt, tt; int ok, want[2], cmp[2]; } T[] = {
        {0.5, 5.0, 1, {N - 3, N - 2}, {N - 3, N - 2}},   // both taken
        {0.15, 5.0, 1, {0, N - 3}, {N - 3, N - 2}},      // N-2 is two steps from the key: 0.2 rad
        {0.05, 5.0, 1, {0, 1}, {N - 3, N - 5}},          // nothing taken: the compared clone moves back by two
        {0.5, 5.0, 0, {0, 1}, {N - 3, N - 5}},           // tracking lost
    };
    for (auto& t : T) {
        CloneChoice o{};
        clone_choice_on_records(N, cam.data(), t.rt, t.tt, t.ok, t.want, &o);
        if (!o.evaluated || !o.agree || o.chosen[0] != t.want[0] || o.chosen[1] != t.want[1] || o.compared[0] != t.cmp[0] || o.compared[1] != t.cmp[1]) return fail("result set");
        if (std::fabs(o.angle[0] - 0.1) > 1e-15 || std::fabs(o.distance[0] - 1.0) > 1e-15) return fail("angle / distance");
    }
    {   // {0, N-5}: the first not taken, the clone behind the key taken -- N-5 turned back onto the key
        std::vector<double> c2 = cam;
        for (int i = 0; i < 12; ++i) c2[(size_t)(N - 5) * 12 + i] = cam[(size_t)(N - 4) * 12 + i];
        const int want[2] = {0, N - 5}, other[2] = {0, N - 3};
        CloneChoice o{};
        clone_choice_on_records(N, c2.data(), 0.05, 5.0, 1, other, &o);
        if (o.agree || o.chosen[0] != want[0] || o.chosen[1] != want[1] || o.angle[1] != 0.0 || o.distance[1] != 0.0 || !o.taken[1] || o.taken[0]) return fail("{0, N-5}");
    }
    {   // half turns: trace <= 0, each of the three branches
        for (int ax = 0; ax < 3; ++ax) {
            double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, H[9] = {-1, 0, 0, 0, -1, 0, 0, 0, -1};
            H[ax * 4] = 1.0;
            const double a = clone_choice_angle(I, H);
            if (std::fabs(a - M_PI) > 1e-15) return fail("half turn");
        }
        double A[9], B[9];
        rot_z(0.3, A); rot_z(0.3 + 3.0, B);
        if (std::fabs(clone_choice_angle(A, B) - 3.0) > 1e-14) return fail("a turn of 3 rad");
        rot_z(0.3 + 1e-9, B);
        if (std::fabs(clone_choice_angle(A, B) - 1e-9) > 1e-15) return fail("a turn of 1e-9 rad");   // (the entries' own rounding; acos would give 0 or 2e-8 here)
    }
    for (int n = 6; n < 24; ++n) {
        int count = 0;
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) count += clone_choice_possible(n, a, b) ? 1 : 0;
        if (count != (n == 6 ? 3 : 4)) return fail("possible sets");   // (at N = 6 the sets {0, N-5} and {0, 1} are one)
    }
    if (clone_choice_possible(5, 0, 1)) return fail("N = 5");
    std::printf("clone choice model ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return edge_inputs();
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the case");
    double head[7];
    for (double& v : head) if (std::fscanf(f, "%lf", &v) != 1) return fail("short case");
    const int N = (int)head[0], from_body = (int)head[6];
    if (N < CLONE_CHOICE_MIN_N || N > 4096) return fail("N");
    std::vector<double> rec((size_t)N * 12), cam((size_t)N * 12);
    for (double& v : rec) if (std::fscanf(f, "%lf", &v) != 1) return fail("short case");
    if (from_body) {
        double ext[12];
        for (double& v : ext) if (std::fscanf(f, "%lf", &v) != 1) return fail("short case");
        for (int c = 0; c < N; ++c) clone_choice_cam_pose(&rec[(size_t)c * 12], &rec[(size_t)c * 12 + 9], ext, ext + 9, &cam[(size_t)c * 12]);
    } else cam = rec;
    std::fclose(f);
    const int pred[2] = {(int)head[4], (int)head[5]};
    CloneChoice o{};
    clone_choice_on_records(N, cam.data(), head[1], head[2], (int)head[3], pred, &o);
    std::printf("%d %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g\n", o.evaluated, o.agree, o.chosen[0], o.chosen[1], o.compared[0], o.compared[1], o.taken[0],
                o.taken[1], o.angle[0], o.angle[1], o.distance[0], o.distance[1]);
    return 0;
}
