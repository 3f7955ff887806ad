// The HIP-free half of the zero-velocity check (orcvio_amd/csrc/host/zupt_check_model.hpp) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_zupt_check_mirror.py:
//   no argument    edge inputs of the packing and of the Woodbury fall-back: one row block, the capacity, intervals that are zero,
//                  negative or NaN, a NaN in the marginal and one elsewhere in P, a negative diagonal, an indefinite marginal
//   <case file>    a case as the test writes it (left | sigma_w2 sigma_a2 sigma_wb sigma_ab | R | ba | g | n | P | S | samples):
//                  prints "status chi2 c dt_sum" for the test to compare with the dense form
//   <case file> dense <reps>   the reference's LITERAL form on the same case in plain C++ -- H, R, S = H P_m H^T + R of order 6 (S - 1),
//                  its Cholesky factorisation, r . S^-1 r: prints "chi2 median_us" (scripts/gpu_zupt_check_timing.py: what a caller
//                  paid on the host before the check had a device form; it stands in for the reference's Eigen, which this tree
//                  does not build)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../orcvio_amd/csrc/host/zupt_check_model.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static ZuptCheckConsts consts(int left) { return ZuptCheckConsts{1.6968e-04 * 1.6968e-04, 2.0e-3 * 2.0e-3, 1.9393e-05, 3.0e-03, left}; }

static std::vector<double> make_samples(int S, double rate) {
    std::vector<double> s((size_t)S * 7);
    for (int i = 0; i < S; ++i) {
        s[(size_t)i * 7] = 10.0 + (i + 1) / rate;
        for (int k = 0; k < 3; ++k) s[(size_t)i * 7 + 1 + k] = 1e-3 * (k + 1);
        s[(size_t)i * 7 + 4] = 0.02 * std::sin(0.7 * i); s[(size_t)i * 7 + 5] = -0.03 * std::cos(0.3 * i); s[(size_t)i * 7 + 6] = 9.81 + 0.01 * std::sin(1.3 * i);
    }
    return s;
}

// checkZUPTIMU :3165-3274 as written, dense.  rows [m][4], Pm with Q_bias added inside.
static double dense_chi2(const double* P, int n, const double* rows, int m, const double* R, const double* ba, const double* g, const ZuptCheckConsts& k) {
    const int M = 6 * m;
    std::vector<double> H((size_t)M * 9, 0.0), r((size_t)M, 0.0), Rd((size_t)M, 1.0), HP((size_t)M * 9), S((size_t)M * M);
    double dts = 0.0;
    for (int i = 0; i < m; ++i) {
        const double dt = rows[i * 4];
        const double a[3] = {rows[i * 4 + 1] - ba[0], rows[i * 4 + 2] - ba[1], rows[i * 4 + 3] - ba[2]};
        double Ra[3];
        for (int q = 0; q < 3; ++q) Ra[q] = R[q * 3] * a[0] + R[q * 3 + 1] * a[1] + R[q * 3 + 2] * a[2];
        const double sRa[9] = {0, -Ra[2], Ra[1], Ra[2], 0, -Ra[0], -Ra[1], Ra[0], 0}, sa[9] = {0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0};
        for (int q = 0; q < 3; ++q) {
            H[(size_t)(6 * i + q) * 9 + 3 + q] = 1.0;
            r[6 * i + 3 + q] = -Ra[q] - g[q];
            for (int c = 0; c < 3; ++c) {
                H[(size_t)(6 * i + 3 + q) * 9 + c] = k.left ? sRa[q * 3 + c] : R[q * 3] * sa[c] + R[q * 3 + 1] * sa[3 + c] + R[q * 3 + 2] * sa[6 + c];
                H[(size_t)(6 * i + 3 + q) * 9 + 6 + c] = R[q * 3 + c];
            }
            Rd[6 * i + q] = k.sigma_w2 / dt;
            Rd[6 * i + 3 + q] = k.sigma_a2 / dt;
        }
        dts += dt;
    }
    double Pm[81];
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) Pm[i * 9 + j] = P[(size_t)zupt_check_state(i) * n + zupt_check_state(j)];
    for (int q = 0; q < 3; ++q) { Pm[(3 + q) * 10] += dts * k.sigma_wb; Pm[(6 + q) * 10] += dts * k.sigma_ab; }
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < 9; ++j) {
            double s = 0.0;
            for (int q = 0; q < 9; ++q) s += H[(size_t)i * 9 + q] * Pm[q * 9 + j];
            HP[(size_t)i * 9 + j] = s;
        }
    for (int i = 0; i < M; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = i == j ? Rd[i] : 0.0;
            for (int q = 0; q < 9; ++q) s += HP[(size_t)i * 9 + q] * H[(size_t)j * 9 + q];
            S[(size_t)i * M + j] = s;
        }
    // llt (lower), then y = L^-1 r, chi2 = y . y
    double chi2 = 0.0;
    for (int j = 0; j < M; ++j) {
        double* Lj = &S[(size_t)j * M];
        double d = Lj[j];
        for (int q = 0; q < j; ++q) d -= Lj[q] * Lj[q];
        const double c = std::sqrt(d);
        Lj[j] = c;
        for (int i = j + 1; i < M; ++i) {
            double* Li = &S[(size_t)i * M];
            double v = Li[j];
            for (int q = 0; q < j; ++q) v -= Li[q] * Lj[q];
            Li[j] = v / c;
        }
        double y = r[j];
        for (int q = 0; q < j; ++q) y -= Lj[q] * r[q];
        r[j] = y / c;
        chi2 += r[j] * r[j];
    }
    return chi2;
}

static int run_file(const char* path, int dense_reps) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    std::vector<double> v;
    double x;
    while (std::fscanf(f, "%lf", &x) == 1) v.push_back(x);
    std::fclose(f);
    size_t o = 0;
    ZuptCheckConsts k{};
    k.left = (int)v.at(o++);
    k.sigma_w2 = v.at(o++); k.sigma_a2 = v.at(o++); k.sigma_wb = v.at(o++); k.sigma_ab = v.at(o++);
    const double* R = &v.at(o); o += 9;
    const double* ba = &v.at(o); o += 3;
    const double* g = &v.at(o); o += 3;
    const int n = (int)v.at(o++);
    const double* P = &v.at(o); o += (size_t)n * n;
    const int S = (int)v.at(o++);
    if (v.size() != o + (size_t)S * 7 || S < 2 || S > ZCHK_MAX_SAMPLES) return 3;
    std::vector<double> rows((size_t)(S - 1) * ZCHK_ROW);
    if (zupt_check_pack(&v[o], S, rows.data()) != 0) return 4;
    if (dense_reps > 0) {
        std::vector<double> us;
        double chi2 = 0.0;
        for (int it = 0; it < dense_reps; ++it) {
            const auto t0 = std::chrono::steady_clock::now();
            chi2 = dense_chi2(P, n, rows.data(), S - 1, R, ba, g, k);
            us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(us.begin(), us.end());
        std::printf("%.17g %.3f\n", chi2, us[us.size() / 2]);
        return 0;
    }
    double out[3];
    const int st = zupt_check_host(P, n, rows.data(), S - 1, R, ba, g, k, out);
    std::printf("%d %.17g %.17g %.17g\n", st, out[0], out[1], out[2]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 3 && std::string(argv[2]) == "dense") return run_file(argv[1], std::atoi(argv[3]));
    if (argc > 1) return run_file(argv[1], 0);
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ba[3] = {0.01, -0.02, 0.005}, g[3] = {0, 0, -9.81};
    const int n = 22;
    std::vector<double> P((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) P[(size_t)i * n + i] = i < 3 ? 4e-4 : (i >= 9 && i < 15 ? 1e-3 : 0.1);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int left = 0; left < 2; ++left) {
        const ZuptCheckConsts k = consts(left);
        for (int S : {2, 3, 65, (int)ZCHK_MAX_SAMPLES}) {   // one row block .. the capacity: rows is exactly (S - 1) x 4, the sanitizer watches its end
            const std::vector<double> smp = make_samples(S, 200.0);
            std::vector<double> rows((size_t)(S - 1) * ZCHK_ROW);
            CHECK(zupt_check_pack(smp.data(), S, rows.data()) == 0);
            double out[3];
            CHECK(zupt_check_host(P.data(), n, rows.data(), S - 1, R, ba, g, k, out) == ZCHK_OK);
            CHECK(std::isfinite(out[0]) && out[0] > 0.0 && out[0] <= out[1]);
            CHECK(std::fabs(out[2] - (S - 1) / 200.0) < 1e-9);
        }
        // S = 0 and S = 1: nothing to pack, nothing written
        double none[1] = {-1.0};
        CHECK(zupt_check_pack(nullptr, 0, none) == 0 && zupt_check_pack(make_samples(1, 200.0).data(), 1, none) == 0 && none[0] == -1.0);
        // intervals the reference would divide by
        for (double bad : {0.0, -0.005, nan}) {
            std::vector<double> smp = make_samples(5, 200.0);
            smp[3 * 7] = std::isnan(bad) ? nan : smp[2 * 7] + bad;
            std::vector<double> rows(4 * ZCHK_ROW);
            CHECK(zupt_check_pack(smp.data(), 5, rows.data()) == 1 + 2);
        }
        const std::vector<double> smp = make_samples(5, 200.0);
        std::vector<double> rows(4 * ZCHK_ROW);
        CHECK(zupt_check_pack(smp.data(), 5, rows.data()) == 0);
        double out[3];
        {   // a NaN inside the marginal (either triangle) is refused; one elsewhere in P is not examined
            std::vector<double> Q = P;
            Q[(size_t)12 * n + 1] = nan;
            CHECK(zupt_check_host(Q.data(), n, rows.data(), 4, R, ba, g, k, out) == ZCHK_NOT_FINITE);
            Q = P; Q[(size_t)1 * n + 12] = nan;
            CHECK(zupt_check_host(Q.data(), n, rows.data(), 4, R, ba, g, k, out) == ZCHK_NOT_FINITE);
            Q = P; Q[(size_t)4 * n + 4] = nan; Q[(size_t)3 * n + 9] = nan; Q[(size_t)21 * n + 0] = nan;
            CHECK(zupt_check_host(Q.data(), n, rows.data(), 4, R, ba, g, k, out) == ZCHK_OK);
        }
        {   // a negative diagonal, an indefinite marginal
            std::vector<double> Q = P;
            Q[(size_t)2 * n + 2] = -4e-4;
            CHECK(zupt_check_host(Q.data(), n, rows.data(), 4, R, ba, g, k, out) == ZCHK_P_NOT_SPD);
            Q = P; Q[(size_t)0 * n + 1] = Q[(size_t)1 * n + 0] = 1.0;
            CHECK(zupt_check_host(Q.data(), n, rows.data(), 4, R, ba, g, k, out) == ZCHK_P_NOT_SPD);
        }
        {   // both triangles are read: an entry in one triangle only counts half
            std::vector<double> Q = P, Qs = P;
            Q[(size_t)0 * n + 12] = 2e-4;
            Qs[(size_t)0 * n + 12] = Qs[(size_t)12 * n + 0] = 1e-4;
            double a[3], b[3];
            CHECK(zupt_check_host(Q.data(), n, rows.data(), 4, R, ba, g, k, a) == ZCHK_OK && zupt_check_host(Qs.data(), n, rows.data(), 4, R, ba, g, k, b) == ZCHK_OK);
            CHECK(a[0] == b[0]);
        }
    }
    std::printf("zupt check model ok\n");
    return 0;
}
