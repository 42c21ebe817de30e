// The PPO learner's host-only plan (csrc/ev2g_policy_host.h: plan_ppo, ppo_lds) and the index the device repack writes by, without HIP:
//   * packed_f32_index(n, k, K) is where pack_linear_f32 puts W[n][k], for matrices with padding rows and columns; writing exactly the
//     indices of the real elements into a zeroed image reproduces the host image, so the entries never written are exactly the padding zeros;
//   * unpack_linear_f32 inverts pack_linear_f32;
//   * plan_ppo accepts every network with d_in <= 192, d_out <= 64 and hidden widths <= 64, its LDS blocks do not overlap and fit 160 KiB, its
//     slab regions do not overlap, the flat offsets are the arrays' sizes in SB3's order, and a refusal names the width.
#include <cstdio>
#include <cstdlib>

#include "../../ev2gym_amd/csrc/ev2g_policy_host.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static void check_index(int n_out, int n_in, int kpad) {
    const int N = mlp_round_up(n_out, 32), K = mlp_round_up(n_in, kpad);
    std::vector<float> W((size_t)n_out * n_in);
    for (size_t i = 0; i < W.size(); i++) W[i] = 1.0f + (float)i;   // (no zero among the real elements)
    const std::vector<float> img = pack_linear_f32(W.data(), n_out, n_in, N, K);
    std::vector<float> mine(img.size(), 0.f), back(W.size(), -1.f);
    for (int n = 0; n < n_out; n++)
        for (int k = 0; k < n_in; k++) {
            const size_t at = packed_f32_index(n, k, K);
            CHECK(at < mine.size() && mine[at] == 0.f, "index (%d, %d) of %d x %d lands at %zu twice or outside", n, k, n_out, n_in, at);
            if (at < mine.size()) mine[at] = W[(size_t)n * n_in + k];
        }
    CHECK(mine == img, "%d x %d (K %d): the image written by index differs from pack_linear_f32's", n_out, n_in, K);
    unpack_linear_f32(img.data(), n_out, n_in, K, back.data());
    CHECK(back == W, "%d x %d: unpack_linear_f32 does not invert pack_linear_f32", n_out, n_in);
}

int main() {
    for (const auto &s : {std::array<int, 3>{64, 162, 8}, {33, 63, 8}, {17, 33, 32}, {50, 64, 32}, {1, 1, 8}, {64, 50, 32}, {40, 20, 32}, {96, 192, 8}})
        check_index(s[0], s[1], s[2]);
    int accepted = 0;
    for (int d_in : {1, 63, 162, 192})
        for (int d_out : {1, 20, 50, 64})
            for (int h1 : {1, 33, 64})
                for (int h2 : {17, 64})
                    for (int v1 : {1, 40, 64})
                        for (int v2 : {64, 7}) {
                            const PpoPlan p = plan_ppo(d_in, h1, h2, v1, v2, d_out);
                            CHECK(p.err == EV2G_OK, "%d %d %d %d %d %d refused: %s", d_in, h1, h2, v1, v2, d_out, p.refusal.c_str());
                            if (p.err) continue;
                            accepted++;
                            const PpoLds &l = p.lds;
                            CHECK(l.bytes <= EV2G_PPO_LDS_LIMIT, "LDS %zu", l.bytes);
                            const int R = EV2G_PPO_ROWS;
                            const int off[13] = {l.oIV, l.oX, l.oH1, l.oH2, l.oV1, l.oV2, l.oMU, l.oACT, l.oD1, l.oD2, l.oE1, l.oE2, l.oROW};
                            const int len[13] = {2 * p.ac.n3, R * l.sX, R * l.sH1, R * l.sH2, R * l.sV1, R * l.sV2, R * l.sMU, R * l.sMU, R * l.sH1, R * l.sH2, R * l.sV1,
                                                 R * l.sV2, 3 * R};
                            for (int i = 0; i < 13; i++) {
                                CHECK(off[i] % 4 == 0, "LDS block %d starts at float %d: not 16-byte aligned", i, off[i]);
                                CHECK(i == 12 ? (size_t)(off[i] + len[i]) * 4 == l.bytes : off[i] + len[i] == off[i + 1], "LDS block %d overlaps or leaves a gap", i);
                            }
                            CHECK(l.sX >= p.k1r + 4 && p.k1r % 32 == 0 && p.k1r >= p.ac.k1, "x stride %d for k1r %d", l.sX, p.k1r);
                            const int want[13] = {h1 * d_in, h1, h2 * h1, h2, v1 * d_in, v1, v2 * v1, v2, d_out * h2, d_out, v2, 1, d_out};
                            int o = 0;
                            for (int i = 0; i < 13; i++) {
                                CHECK(p.off[i] == o && p.rows[i] * p.cols[i] == want[i], "array %d: offset %d size %d", i, p.off[i], p.rows[i] * p.cols[i]);
                                o += want[i];
                                const int end = p.slab_off[i] + (p.rows[i] - 1) * p.slab_ld[i] + p.cols[i];
                                CHECK(end <= (i == 12 ? p.slab_floats : p.slab_off[i + 1]) && p.cols[i] <= std::max(p.slab_ld[i], 1), "array %d's slab region", i);
                            }
                            CHECK(p.n_params == o && p.grid_cap == EV2G_PPO_GRID_CAP, "n_params %d", p.n_params);
                            CHECK(p.workspace_bytes == (size_t)p.grid_cap * ((size_t)p.slab_floats * 4 + 64), "workspace bytes");
                        }
    CHECK(accepted == 4 * 4 * 3 * 2 * 3 * 2, "accepted %d", accepted);
    const struct { int s[6]; const char *word; } bad[] = {{{193, 64, 64, 64, 64, 50}, "d_in 193"}, {{0, 64, 64, 64, 64, 50}, "d_in 0"}, {{162, 64, 64, 64, 64, 65}, "d_out 65"},
                                                           {{162, 0, 64, 64, 64, 50}, "h1 0"}, {{162, 64, 64, 257, 64, 50}, "v1 257"},
                                                           {{192, 128, 128, 128, 128, 64}, "h1 128"}, {{192, 64, 64, 256, 256, 64}, "v1 256"}};
    for (const auto &b : bad) {
        const PpoPlan p = plan_ppo(b.s[0], b.s[1], b.s[2], b.s[3], b.s[4], b.s[5]);
        CHECK(p.err == EV2G_ERR_ARG && p.refusal.find(b.word) != std::string::npos, "refusal of %d.. says '%s', expected '%s'", b.s[0], p.refusal.c_str(), b.word);
    }
    if (fails) return 1;
    std::printf("ppo_plan_check: ok (%d plans)\n", accepted);
    return 0;
}
