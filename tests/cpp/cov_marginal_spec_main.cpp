// The HIP-free half of the marginal read (orcvio_amd/csrc/host/cov_marginal_spec.hpp) as a stand-alone program, for
// tests/test_cov_marginal_cases.py: built with -fsanitize=address,undefined and run directly.  Every array is exactly as long as
// the contract says, on the heap, so a read or a write past it is reported: marginal_refusal on every refusal of the C-ABI's list and
// on the largest acceptable request, odometry_marginal_spec / _split on the rotation given on the command line (nine doubles).
// Prints "idx ..." and "T ..." of the spec, then "cov marginal spec ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/host/cov_marginal_spec.hpp"

using namespace orcvio_amd;

static int fails = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++fails; }
}
static bool refused(const char* why, const char* word) { return why && std::strstr(why, word); }

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    std::unique_ptr<double[]> R(new double[9]);
    for (int i = 0; i < 9; ++i) R[i] = std::atof(argv[1 + i]);

    // ---- the validation
    const int n = 34;
    for (int k : {1, 2, 9, 63, 64})
        for (int m : {0, 1, 9, 64}) {
            std::unique_ptr<int32_t[]> idx(new int32_t[k]);
            for (int i = 0; i < k; ++i) idx[i] = (i * 7 + n - 1) % n;   // (repeats once k > n; n - 1 and 0 among them)
            std::unique_ptr<double[]> T(m ? new double[(size_t)m * k] : nullptr);
            for (int i = 0; i < m * k; ++i) T[i] = 0.25 * i - 3.0;
            expect(marginal_refusal(k, idx.get(), m, T.get(), n) == nullptr, "an acceptable request");
            expect(refused(marginal_refusal(k, idx.get(), m, T.get(), 0), "no resident"), "no resident covariance");
            expect(refused(marginal_refusal(k, nullptr, m, T.get(), n), "idx is NULL"), "idx NULL");
            idx[k - 1] = n;
            expect(refused(marginal_refusal(k, idx.get(), m, T.get(), n), "index outside"), "index == n");
            idx[k - 1] = -1;
            expect(refused(marginal_refusal(k, idx.get(), m, T.get(), n), "index outside"), "index < 0");
            idx[k - 1] = 0;
            if (m) {
                expect(refused(marginal_refusal(k, idx.get(), m, nullptr, n), "T is NULL"), "T NULL with m > 0");
                expect(refused(marginal_refusal(k, idx.get(), 0, T.get(), n), "m == 0"), "T given with m == 0");
                T[(size_t)m * k - 1] = std::numeric_limits<double>::quiet_NaN();
                expect(refused(marginal_refusal(k, idx.get(), m, T.get(), n), "non-finite"), "NaN in the last entry of T");
                T[(size_t)m * k - 1] = 1.0;
                T[0] = -std::numeric_limits<double>::infinity();
                expect(refused(marginal_refusal(k, idx.get(), m, T.get(), n), "non-finite"), "Inf in the first entry of T");
            }
        }
    {
        int32_t one = 0;
        double t = 1.0;
        expect(refused(marginal_refusal(0, &one, 0, nullptr, n), "n_idx"), "n_idx == 0");
        expect(refused(marginal_refusal(-3, &one, 0, nullptr, n), "n_idx"), "n_idx < 0");
        expect(refused(marginal_refusal(MARGINAL_MAX + 1, &one, 0, nullptr, n), "n_idx"), "n_idx == 65 (refused before idx is read)");
        expect(refused(marginal_refusal(1, &one, -1, &t, n), "m outside"), "m < 0");
        expect(refused(marginal_refusal(1, &one, MARGINAL_MAX + 1, &t, n), "m outside"), "m == 65 (refused before T is read)");
    }

    // ---- the odometry spec
    std::unique_ptr<int32_t[]> idx(new int32_t[9]);
    std::unique_ptr<double[]> T(new double[81]);
    odometry_marginal_spec(R.get(), idx.get(), T.get());
    expect(marginal_refusal(ODOMETRY_MARGINAL_DIM, idx.get(), ODOMETRY_MARGINAL_DIM, T.get(), 22) == nullptr, "the spec is acceptable at the smallest state");
    std::printf("idx");
    for (int i = 0; i < 9; ++i) std::printf(" %d", idx[i]);
    std::printf("\nT");
    for (int i = 0; i < 81; ++i) std::printf(" %.17g", T[i]);
    std::printf("\n");
    std::unique_ptr<double[]> out(new double[81]), pose(new double[36]), vel(new double[9]);
    for (int i = 0; i < 81; ++i) out[i] = 100.0 + i;
    odometry_marginal_split(out.get(), pose.get(), vel.get());
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) expect(pose[6 * i + j] == 100.0 + 9 * i + j, "the leading 6 x 6");
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) expect(vel[3 * i + j] == 100.0 + 9 * (6 + i) + 6 + j, "the trailing 3 x 3");
    if (fails) return 1;
    std::printf("cov marginal spec ok\n");
    return 0;
}
