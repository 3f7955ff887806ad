// Host half of orcvio_msckf_io_triangulate_prune (orcvio_amd/csrc/triangulate_arm.hpp: tri_prune_layout, tri_prune_arm_stage,
// tri_prune_covers) on its own, built with -fsanitize=address,undefined by tests/test_prune_tri_arm.py: the block and every input array
// are heap blocks of exactly the size the layout or the list asks for, so a write or read past them is reported.  No device.
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/triangulate_arm.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct List {   // exactly-sized heap copies of a CSR list
    std::unique_ptr<int32_t[]> ptr, clone;
    std::unique_ptr<double[]> z;
    orcvio_msckf_tracks tr{};
};
// F tracks of M observations each on the clones first, first + 1, ..
static List make_list(int F, int M, int first = 0) {
    List l;
    const int nobs = F * M;
    l.ptr.reset(new int32_t[F + 1]);
    l.clone.reset(new int32_t[nobs > 0 ? nobs : 1]);
    l.z.reset(new double[nobs > 0 ? 2 * nobs : 1]);
    for (int j = 0; j <= F; ++j) l.ptr[j] = j * M;
    for (int o = 0; o < nobs; ++o) { l.clone[o] = first + o % M; l.z[2 * o] = 0.25 * o; l.z[2 * o + 1] = -0.5 * o; }
    l.tr.n_features = F; l.tr.p_w = nullptr; l.tr.obs_ptr = l.ptr.get(); l.tr.obs_clone = nobs > 0 ? l.clone.get() : nullptr;
    l.tr.obs_z = nobs > 0 ? l.z.get() : nullptr; l.tr.obs_zvel = nullptr;
    return l;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const orcvio_triangulation_config good{0.2, 0.01, 5e-7, 1e-3, 10, 10, 4.7673e-4, 5.0};
    // mode 3 is a mode of the prune arming alone (4 of neither): the first update's arming refuses it as it did
    { const int32_t m[4] = {0, 1, 2, 3}; CHECK(tri_first_bad_mode(m, 4, ORCVIO_TRI_ALL_MOTION_BUT_LAST) == -1 && tri_first_bad_mode(m, 4) == 3);
      const int32_t b[2] = {3, 4}; CHECK(tri_first_bad_mode(b, 2, ORCVIO_TRI_ALL_MOTION_BUT_LAST) == 1); }
    const int N = 40;
    for (int maxF : {1, 7, 64, 300}) {
        const int maxObs = maxF * ORCVIO_MAX_TRACK;
        const TriPruneBlock b = tri_prune_layout(maxF, maxObs);
        const TriBlock r = tri_block_layout(maxF);
        // the second block: the first block's layout, the list behind it, room for the fullest list
        CHECK(b.res.bytes == r.bytes && b.res.mode == r.mode && b.res.inv_param == r.inv_param && b.list == r.bytes && b.list % 256 == 0);
        const TriList cap = tri_list_layout(maxF, maxObs);
        CHECK(b.bytes == b.list + cap.bytes && cap.obs_ptr == 0 && cap.obs_clone >= 4 * (size_t)(maxF + 1) && cap.obs_z >= cap.obs_clone + 4 * (size_t)maxObs &&
              cap.bytes >= cap.obs_z + 16 * (size_t)maxObs);
        for (size_t o : {cap.obs_clone, cap.obs_z, cap.bytes}) CHECK(o % 256 == 0);
        std::unique_ptr<char[]> block(new char[b.bytes]);
        for (size_t i = 0; i < b.bytes; ++i) block[i] = (char)0x5a;
        const char* why = nullptr;
        for (int F : {0, 1, maxF})
            for (int M : {2, 3, ORCVIO_MAX_TRACK}) {
                List l = make_list(F, M);
                const int nobs = F * M;
                const TriList ll = tri_list_layout(F, nobs);
                CHECK(ll.bytes <= cap.bytes && ll.bytes % 256 == 0);
                for (int with_mode = 0; with_mode < 2; ++with_mode) {
                    std::unique_ptr<int32_t[]> mode(new int32_t[F > 0 ? F : 1]);
                    for (int j = 0; j < F; ++j) mode[j] = j % 4;
                    for (size_t i = 0; i < b.bytes; ++i) block[i] = (char)0x5a;
                    CHECK(tri_prune_arm_stage(&good, &l.tr, with_mode ? mode.get() : nullptr, N, maxF, maxObs, block.get(), &why) == ORCVIO_OK && why && !why[0]);
                    const int32_t* md = reinterpret_cast<const int32_t*>(block.get() + b.res.mode);
                    for (int j = 0; j < F; ++j) CHECK(md[j] == (with_mode ? j % 4 : (int)ORCVIO_TRI_ALL_MOTION_BUT_LAST));
                    const char* lp = block.get() + b.list;
                    CHECK(std::memcmp(lp + ll.obs_ptr, l.ptr.get(), 4 * (size_t)(F + 1)) == 0);
                    if (nobs > 0) CHECK(std::memcmp(lp + ll.obs_clone, l.clone.get(), 4 * (size_t)nobs) == 0 && std::memcmp(lp + ll.obs_z, l.z.get(), 16 * (size_t)nobs) == 0);
                    // the results are the device's to write; nothing behind the list's own bytes is touched
                    for (size_t i = b.res.valid; i < b.list; ++i) CHECK(block[i] == (char)0x5a);
                    for (size_t i = b.list + ll.bytes; i < b.bytes; ++i) CHECK(block[i] == (char)0x5a);
                    // the frame call's check: every prune observation's clone occurs in its track's list
                    CHECK(tri_prune_covers(block.get(), maxF, maxObs, F, l.ptr.get(), l.clone.get()));
                    if (F > 0) {
                        List other = make_list(F, M, 1);   // (clones 1 .. M: the last one is not in the staged list)
                        CHECK(!tri_prune_covers(block.get(), maxF, maxObs, F, other.ptr.get(), other.clone.get()));
                        List fewer = make_list(F, 1);      // (a subset: the first clone of every track)
                        CHECK(tri_prune_covers(block.get(), maxF, maxObs, F, fewer.ptr.get(), fewer.clone.get()));
                    }
                }
                // ---- refusals: their code, a reason, nothing written
                const std::vector<char> before(block.get(), block.get() + b.bytes);
                auto refused = [&](int code, const orcvio_triangulation_config* c, const orcvio_msckf_tracks* t, const int32_t* m, int n_clones) {
                    why = nullptr;
                    return tri_prune_arm_stage(c, t, m, n_clones, maxF, maxObs, block.get(), &why) == code && why && why[0] &&
                           std::memcmp(before.data(), block.get(), b.bytes) == 0;
                };
                orcvio_triangulation_config c = good;
                c.huber_epsilon = nan;
                CHECK(refused(ORCVIO_ERR_INVALID, &c, &l.tr, nullptr, N) && refused(ORCVIO_ERR_INVALID, nullptr, &l.tr, nullptr, N));
                CHECK(refused(ORCVIO_ERR_INVALID, &good, nullptr, nullptr, N));
                { orcvio_msckf_tracks t = l.tr; t.obs_ptr = nullptr; CHECK(refused(ORCVIO_ERR_INVALID, &good, &t, nullptr, N)); }
                { orcvio_msckf_tracks t = l.tr; t.n_features = -1; CHECK(refused(ORCVIO_ERR_INVALID, &good, &t, nullptr, N)); }
                if (F > 0) {
                    for (int v : {4, -1, 1 << 30}) {
                        std::unique_ptr<int32_t[]> bad(new int32_t[F]);
                        for (int j = 0; j < F; ++j) bad[j] = 3;
                        bad[F - 1] = v;
                        CHECK(refused(ORCVIO_ERR_INVALID, &good, &l.tr, bad.get(), N));
                    }
                    CHECK(refused(ORCVIO_ERR_INVALID, &good, &l.tr, nullptr, M - 1));   // the last clone of every track is outside the window
                    { List d = make_list(F, M); d.clone[nobs - 1] = -1; CHECK(refused(ORCVIO_ERR_INVALID, &good, &d.tr, nullptr, N)); }
                    { List d = make_list(F, M); d.clone[1] = d.clone[0]; CHECK(refused(ORCVIO_ERR_INVALID, &good, &d.tr, nullptr, N)); }   // not ascending
                    { List d = make_list(F, M); std::swap(d.clone[nobs - 1], d.clone[nobs - 2]); CHECK(refused(ORCVIO_ERR_INVALID, &good, &d.tr, nullptr, N)); }
                    { List d = make_list(F, M); d.ptr[0] = 1; CHECK(refused(ORCVIO_ERR_INVALID, &good, &d.tr, nullptr, N)); }
                    { List d = make_list(F, M); d.tr.obs_z = nullptr; CHECK(refused(ORCVIO_ERR_INVALID, &good, &d.tr, nullptr, N)); }
                    if (F > 1 && M == 2) { List d = make_list(F, M); d.ptr[1] = d.ptr[2] + 1; CHECK(refused(ORCVIO_ERR_INVALID, &good, &d.tr, nullptr, N)); }   // not monotone
                }
            }
        // longer than ORCVIO_MAX_TRACK; more tracks, more observations than the handle holds
        { List d = make_list(1, ORCVIO_MAX_TRACK + 1); const std::vector<char> before(block.get(), block.get() + b.bytes);
          CHECK(tri_prune_arm_stage(&good, &d.tr, nullptr, N, maxF, maxObs, block.get(), &why) == ORCVIO_ERR_TRACK_TOO_LONG && why[0] && std::memcmp(before.data(), block.get(), b.bytes) == 0); }
        { List d = make_list(maxF + 1, 2); const std::vector<char> before(block.get(), block.get() + b.bytes);
          CHECK(tri_prune_arm_stage(&good, &d.tr, nullptr, N, maxF, maxObs, block.get(), &why) == ORCVIO_ERR_CAPACITY && why[0] && std::memcmp(before.data(), block.get(), b.bytes) == 0); }
        { List d = make_list(maxF, 3); const std::vector<char> before(block.get(), block.get() + b.bytes);
          CHECK(tri_prune_arm_stage(&good, &d.tr, nullptr, N, maxF, 3 * maxF - 1, block.get(), &why) == ORCVIO_ERR_CAPACITY && why[0] && std::memcmp(before.data(), block.get(), b.bytes) == 0); }
    }
    std::printf("prune tri arm ok\n");
    return 0;
}
