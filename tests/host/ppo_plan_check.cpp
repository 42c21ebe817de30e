// The PPO learner's host-only plan (csrc/ev2g_policy_host.h: plan_ppo, ppo_lds) and the index the device repack writes by, without HIP:
//   * packed_f32_index(n, k, K) is where pack_linear_f32 puts W[n][k], for matrices with padding rows and columns; writing exactly the
//     indices of the real elements into a zeroed image reproduces the host image, so the entries never written are exactly the padding zeros;
//   * unpack_linear_f32 inverts pack_linear_f32;
//   * plan_ppo accepts every network with d_in <= 192, d_out <= 64 and hidden widths <= 64, its LDS blocks do not overlap and fit 160 KiB, its
//     slab regions do not overlap, the flat offsets are the arrays' sizes in SB3's order, and a refusal names the width;
//   * ppo_map(plan, images, transposed images) is the table the device places elements by: applied on the host exactly as ev2g_ppo_repack_kernel
//     applies it (ev2g_ppo_which, then packed_f32_index(r, c, img_k) or e) to random masters and zeroed images, it gives pack_ac's twelve images and
//     pack_linear_f32 of the three transposed matrices, byte for byte -- every element lands where the kernels read it and padding stays zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

// ev2g_ppo.h: ev2g_ppo_which and the body of ev2g_ppo_repack_kernel (transposed_only 0) over all elements, with every store bounds-checked
struct Image { std::vector<float> v; };
static void put(float *base, size_t at, float t, const Image *images, int n_images) {
    for (int k = 0; k < n_images; k++)
        if (base == images[k].v.data()) {
            CHECK(at < images[k].v.size(), "a store at %zu of an image of %zu floats", at, images[k].v.size());
            if (at < images[k].v.size()) base[at] = t;
            return;
        }
    CHECK(false, "a store through a pointer that is none of the fifteen images");
}
static void host_repack(const PpoMap &mp, const float *theta, const Image *images, int n_images) {
    for (int i = 0; i < mp.n_params; i++) {
        int a = 0;
        for (int k = 1; k < EV2G_PPO_ARRAYS; k++) a += i >= mp.off[k] ? 1 : 0;
        const int e = i - mp.off[a];
        if (!mp.img[a]) continue;
        const float t = theta[i];
        if (mp.img_k[a] == 0) { put(mp.img[a], (size_t)e, t, images, n_images); continue; }
        const int r = e / mp.cols[a], c = e - r * mp.cols[a];
        put(mp.img[a], packed_f32_index(r, c, mp.img_k[a]), t, images, n_images);
        if (mp.imgT[a]) put(mp.imgT[a], packed_f32_index(c, r, mp.imgT_k[a]), t, images, n_images);
    }
}
static bool same_bytes(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}
static std::vector<float> transposed(const float *W, int n_out, int n_in) {
    std::vector<float> t((size_t)n_out * n_in);
    for (int r = 0; r < n_out; r++)
        for (int c = 0; c < n_in; c++) t[(size_t)c * n_out + r] = W[(size_t)r * n_in + c];
    return t;
}

static void check_map(const PpoPlan &p, int d_in, int h1, int h2, int v1, int v2, int d_out) {
    const AcPlan &a = p.ac;
    std::vector<float> theta((size_t)p.n_params);
    uint32_t x = 0x9e3779b9u ^ (uint32_t)(d_in * 131 + h1 * 17 + v2);
    for (float &t : theta) { x = x * 1664525u + 1013904223u; t = (float)(int32_t)(x | 1u) * 4.656612873077393e-10f; }   // (-1, 1), never zero
    // the arrays in SB3's order, cut out of the flat masters by the sizes written out by hand
    const int size[12] = {h1 * d_in, h1, h2 * h1, h2, v1 * d_in, v1, v2 * v1, v2, d_out * h2, d_out, v2, 1};
    AcWeights w{};
    int o = 0;
    for (int i = 0; i < 12; i++) { w.a[i] = theta.data() + o; o += size[i]; }
    CHECK(o + d_out == p.n_params, "the masters' length");
    const auto want = pack_ac(a, w);
    // fifteen zeroed images: the twelve in AcDev's order, then w2t [n1 x n2], w3t [n2 x n3], u2t [m1 x m2]
    Image images[15];
    for (int i = 0; i < 12; i++) images[i].v.assign(want[(size_t)i].size(), 0.f);
    images[12].v.assign((size_t)a.n1 * a.n2, 0.f); images[13].v.assign((size_t)a.n2 * a.n3, 0.f); images[14].v.assign((size_t)a.m1 * a.m2, 0.f);
    float *img[12], *img_t[3];
    for (int i = 0; i < 12; i++) img[i] = images[i].v.data();
    for (int i = 0; i < 3; i++) img_t[i] = images[12 + i].v.data();
    const PpoMap mp = ppo_map(p, img, img_t);
    CHECK(mp.n_params == p.n_params && mp.slab_floats == p.slab_floats && mp.P == d_out && mp.off[13] == p.n_params, "the map's scalars");
    for (int i = 0; i < 13; i++)
        CHECK(mp.off[i] == p.off[i] && mp.cols[i] == p.cols[i] && mp.slab_off[i] == p.slab_off[i] && mp.slab_ld[i] == p.slab_ld[i], "the map's array %d", i);
    CHECK(mp.img[12] == nullptr && mp.imgT[12] == nullptr, "log_std has no image");
    host_repack(mp, theta.data(), images, 15);
    for (int i = 0; i < 12; i++) CHECK(same_bytes(images[i].v, want[(size_t)i]), "%d %d %d %d %d %d: image %d differs from pack_ac's", d_in, h1, h2, v1, v2, d_out, i);
    const std::vector<float> w2t = transposed(w.a[2], h2, h1), w3t = transposed(w.a[8], d_out, h2), u2t = transposed(w.a[6], v2, v1);
    CHECK(same_bytes(images[12].v, pack_linear_f32(w2t.data(), h1, h2, a.n1, a.n2)), "%d %d %d %d %d %d: the transposed image of pi_W2", d_in, h1, h2, v1, v2, d_out);
    CHECK(same_bytes(images[13].v, pack_linear_f32(w3t.data(), h2, d_out, a.n2, a.n3)), "%d %d %d %d %d %d: the transposed image of action_W", d_in, h1, h2, v1, v2, d_out);
    CHECK(same_bytes(images[14].v, pack_linear_f32(u2t.data(), v1, v2, a.m1, a.m2)), "%d %d %d %d %d %d: the transposed image of vf_W2", d_in, h1, h2, v1, v2, d_out);
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
                            check_map(p, d_in, h1, h2, v1, v2, d_out);
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
