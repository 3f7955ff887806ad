// Host half of orcvio_msckf_io_triangulate (orcvio_amd/csrc/triangulate_arm.hpp: config and mode validation, the layout of the pinned
// block, staging of the modes) on its own, built with -fsanitize=address,undefined by tests/test_triangulate_arm.py: the block and
// the mode arrays are heap blocks of exactly the size the layout asks for, so a write or read past them is reported.  No device.
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/triangulate_arm.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const orcvio_triangulation_config good{0.2, 0.01, 5e-7, 1e-3, 10, 10, 4.7673e-4, 5.0};
    CHECK(tri_config_ok(&good) && !tri_config_ok(nullptr));
    for (int field = 0; field < 6; ++field)
        for (double v : {nan, inf, -inf}) {
            orcvio_triangulation_config c = good;
            double* p[6] = {&c.translation_threshold, &c.huber_epsilon, &c.estimation_precision, &c.initial_damping, &c.cost_threshold, &c.init_final_dist_threshold};
            *p[field] = v;
            CHECK(!tri_config_ok(&c));
        }
    { orcvio_triangulation_config c = good; c.outer_loop_max_iteration = -1; CHECK(!tri_config_ok(&c)); c = good; c.inner_loop_max_iteration = -1; CHECK(!tri_config_ok(&c));
      c = good; c.outer_loop_max_iteration = 0; c.inner_loop_max_iteration = 0; CHECK(tri_config_ok(&c)); }
    for (int maxF : {1, 63, 64, 65, 2048}) {
        const TriBlock b = tri_block_layout(maxF);
        const size_t F = (size_t)maxF;
        // the parts follow one another without overlap, 256-byte aligned, each large enough
        CHECK(b.mode == 0 && b.valid >= b.mode + 4 * F && b.flags >= b.valid + 4 * F && b.cost >= b.flags + 4 * F && b.p_w >= b.cost + 8 * F &&
              b.inv_param >= b.p_w + 24 * F && b.bytes >= b.inv_param + 24 * F);
        for (size_t o : {b.mode, b.valid, b.flags, b.cost, b.p_w, b.inv_param, b.bytes}) CHECK(o % 256 == 0);
        std::unique_ptr<char[]> block(new char[b.bytes]);
        for (size_t i = 0; i < b.bytes; ++i) block[i] = (char)0x5a;
        const char* why = nullptr;
        for (int Fu : {0, 1, maxF / 2, maxF}) {
            std::unique_ptr<int32_t[]> mode(new int32_t[Fu > 0 ? Fu : 1]);
            for (int j = 0; j < Fu; ++j) mode[j] = j % 3;
            CHECK(tri_first_bad_mode(mode.get(), Fu) == -1 && tri_first_bad_mode(nullptr, Fu) == -1);
            const std::vector<char> pre(block.get(), block.get() + b.bytes);
            CHECK(tri_arm_stage(&good, mode.get(), Fu, maxF, block.get(), &why) == ORCVIO_OK && why && !why[0]);
            const int32_t* staged = reinterpret_cast<const int32_t*>(block.get() + b.mode);
            for (int j = 0; j < Fu; ++j) CHECK(staged[j] == j % 3);
            // nothing but the Fu modes is written: the rest of the mode part stays, the results are the device's to write
            CHECK(std::memcmp(pre.data() + 4 * (size_t)Fu, block.get() + 4 * (size_t)Fu, b.bytes - 4 * (size_t)Fu) == 0);
            for (size_t i = b.valid; i < b.bytes; ++i) CHECK(block[i] == (char)0x5a);
            // refusals: nothing written, a reason given
            std::vector<char> before(block.get(), block.get() + b.bytes);
            auto untouched = [&] { return std::memcmp(before.data(), block.get(), b.bytes) == 0 && why && why[0]; };
            if (Fu > 0) {
                for (int v : {3, -1, 1 << 30}) {
                    std::unique_ptr<int32_t[]> bad(new int32_t[Fu]);
                    for (int j = 0; j < Fu; ++j) bad[j] = (j + 1) % 3;
                    bad[Fu - 1] = v;
                    CHECK(tri_first_bad_mode(bad.get(), Fu) == Fu - 1);
                    CHECK(tri_arm_stage(&good, bad.get(), Fu, maxF, block.get(), &why) == ORCVIO_ERR_INVALID && untouched());
                }
            }
            orcvio_triangulation_config c = good;
            c.cost_threshold = nan;
            CHECK(tri_arm_stage(&c, mode.get(), Fu, maxF, block.get(), &why) == ORCVIO_ERR_INVALID && untouched());
            CHECK(tri_arm_stage(nullptr, mode.get(), Fu, maxF, block.get(), &why) == ORCVIO_ERR_INVALID && untouched());
            CHECK(tri_arm_stage(&good, nullptr, maxF + 1, maxF, block.get(), &why) == ORCVIO_ERR_INVALID && untouched());   // (refused before anything is read)
            CHECK(tri_arm_stage(&good, nullptr, -1, maxF, block.get(), &why) == ORCVIO_ERR_INVALID && untouched());
            CHECK(tri_arm_stage(&good, nullptr, Fu, maxF, block.get(), &why) == ORCVIO_OK && std::memcmp(before.data(), block.get(), b.bytes) == 0);   // (no modes: nothing to stage)
        }
    }
    std::printf("triangulate arm ok\n");
    return 0;
}
