// policy_plan_check.cpp -- enumerates a policy's plan (ev2gym_amd/csrc/ev2g_policy_host.h: plan_mlp) and checks it against predicates written
// here from the contract's wording (include/ev2g.h: ev2g_mlp_create_ex; the kernels' own descriptions in csrc/ev2g_mlp.h; the packing
// route_fused expects), then checks every element of the weight and bias images (pack_linear, pack_linear_s16, pack_linear_f32, pack_mlp,
// pack_ac and its inverse unpack_ac) against the index each layout documents, plan_ac's refusals, and host_bf16 against a round-to-nearest-even written on the two halves of the word.
// Exits non-zero at the first failure.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/policy_plan_check.cpp -o policy_plan_check && ./policy_plan_check
//
// (tests/test_policy_plan_cpu.py does exactly that; the same source builds with -fsanitize=address,undefined.)
//
// The plan's inputs: d_in 1..256 x d_out 1..160 x the three precisions, exhaustive; per point h1 in {1, 127, 128, 400, 401, 416, 417, 512,
// 513} and h2 in those and {304, 305, 320, 321}, plus three widths each drawn from a counter-based hash (two below 640, one below 4096: the
// LDS refusal).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ev2gym_amd/csrc/ev2g_policy_host.h"

static std::string g_case;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            std::fprintf(stderr, "FAIL [%s] line %d: %s\n", g_case.c_str(), __LINE__, #cond);                \
            std::exit(1);                                                                                    \
        }                                                                                                    \
    } while (0)

static bool same(const char *a, const char *b) { return a && b && std::strcmp(a, b) == 0; }
static uint64_t hash64(uint64_t x) {   // splitmix64's finaliser over a counter
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static int ceil_to(int x, int m) { return ((x + m - 1) / m) * m; }

// ---- a. the plan ----
static const char *const kBadArgs = "ev2g_mlp_create: bad arguments";
static const char *const kOutLo = "ev2g_mlp_create: out_lo must be -1 or 0";
static const char *const kPrecision = "ev2g_mlp_create_ex: precision must be EV2G_MLP_BF16, EV2G_MLP_F32 or EV2G_MLP_F32X3";
static const char *const kTooWide = "ev2g_mlp_create: layers too wide for the LDS-resident activations";
static const size_t kLdsLimit = 160 * 1024;

// the streaming kernel's LDS: NX copies (1 for bf16, 3 for the float32 modes) of the bf16 operand rows of the input (ks1 k-steps of 32) and the two
// hidden layers (400 -> 13 k-steps = 416 columns, 304 -> 10 = 320), each row 8 elements longer; then the biases of 25 + 19 + nt3 tiles of 16 floats
static size_t want_s16_lds(int ks1, int nt3, int nx, int rows) {
    return (size_t)rows * ((ks1 * 32 + 8) + (416 + 8) + (320 + 8)) * 2 * nx + (size_t)(25 + 19 + nt3) * 16 * 4;
}

static long long g_plans = 0, g_refused = 0, g_kind[4] = {0, 0, 0, 0};
static void check_plan(int d_in, int h1, int h2, int d_out, int precision) {
    const MlpPlan p = plan_mlp(d_in, h1, h2, d_out, -1.0f, precision);
    g_plans++;
    const bool bf16 = precision == EV2G_MLP_BF16;
    const int nw = bf16 ? 1 : precision == EV2G_MLP_F32 ? 2 : 3;
    // ev2g.h: networks that fit the shipped shapes (inputs <= 192, hidden layers <= 400 / 304 with at least one >= 128, outputs <= 64) run on the
    // streaming kernel; its second shape is 64 -> 400 -> 304 -> 32, and the smaller one wins
    const bool hidden_fit = h1 <= 400 && h2 <= 304 && (h1 >= 128 || h2 >= 128);
    const bool narrow = hidden_fit && d_in <= 64 && d_out <= 32, wide = hidden_fit && d_in <= 192 && d_out <= 64;
    const bool streaming = narrow || wide;
    const int k1 = ceil_to(d_in, 16), n1 = ceil_to(h1, 32), n2 = ceil_to(h2, 32), n3 = ceil_to(d_out, 32);
    // the 32-row kernels' LDS: two activation blocks of 32 rows (the wider of input / layer 2, and layer 1), rows 16 bytes longer than the data;
    // the bf16 kernels stage the padded biases behind them
    const size_t lds_bf16 = (size_t)32 * ((std::max(k1, n2) + 8) + (n1 + 8)) * 2 + (size_t)(n1 + n2 + n3) * 4;
    const size_t lds_f32 = (size_t)32 * ((std::max(k1, n2) + 4) + (n1 + 4)) * 4;
    const size_t lds = streaming ? want_s16_lds(narrow ? 2 : 6, narrow ? 2 : 4, bf16 ? 1 : 3, 16) : bf16 ? lds_bf16 : lds_f32;
    if (lds > kLdsLimit) {
        CHECK(p.err == EV2G_ERR_ARG && same(p.refusal, kTooWide));
        g_refused++;
        return;
    }
    CHECK(p.err == EV2G_OK && p.refusal == nullptr);
    CHECK(p.d_in == d_in && p.h1 == h1 && p.h2 == h2 && p.d_out == d_out && p.precision == precision);
    CHECK(p.k1 == k1 && p.n1 == n1 && p.n2 == n2 && p.n3 == n3);
    CHECK(p.lds == lds);
    CHECK(p.index >= 0 && p.index < MLP_TABLE_ENTRIES && mlp_table_key(p.index).kind == p.kind);
    CHECK(p.kind >= 0 && p.kind < 4);
    g_kind[p.kind]++;
    CHECK((p.kind == MLP_KIND_S16) == streaming);
    CHECK((p.big_index >= 0) == (streaming && bf16));
    if (streaming) {
        // the packing route_fused expects: (2, 25, 19, 2) for PublicPST's rows, (6, 25, 19, 4) for the head-table states, and the terms per weight
        CHECK(p.s16.ks1 == (narrow ? 2 : 6) && p.s16.nt1 == 25 && p.s16.nt2 == 19 && p.s16.nt3 == (narrow ? 2 : 4) && p.s16.nw == nw);
        CHECK(p.rows == 16 && p.threads == (bf16 ? 8 : 4) * 64);   // 8 wavefronts for bf16, 4 otherwise
        const MlpKey k = mlp_table_key(p.index);
        CHECK(p.index >= 4 && p.index < 10);
        CHECK(k.a == p.s16.ks1 && k.b == 25 && k.c == 19 && k.d == p.s16.nt3 && k.nw == nw && k.wv * 64 == p.threads && k.rb == 1);
        if (bf16) {
            const MlpKey b = mlp_table_key(p.big_index);
            CHECK(p.big_index >= 10 && p.big_index < MLP_TABLE_ENTRIES && b.kind == MLP_KIND_S16);
            CHECK(b.a == p.s16.ks1 && b.b == 25 && b.c == 19 && b.d == p.s16.nt3 && b.nw == 1 && b.wv == 4 && b.rb == 2);
            CHECK(p.big_rows == 32 && p.big_threads == 256 && p.big_lds == want_s16_lds(p.s16.ks1, p.s16.nt3, 1, 32) && p.big_lds <= kLdsLimit);
        }
    } else {
        CHECK(p.s16.ks1 == 0 && p.s16.nt1 == 0 && p.s16.nt2 == 0 && p.s16.nt3 == 0 && p.s16.nw == 0);
        CHECK(p.rows == 32 && p.threads == 256);
        // the fixed kernels: the padded (k1 / 16, n1 / 16, n2 / 16) of the shapes next to the shipped ones, at most 128 ports
        const bool f11 = k1 / 16 == 11 && n1 / 16 == 26 && n2 / 16 == 20, f4 = k1 / 16 == 4 && n1 / 16 == 26 && n2 / 16 == 20;
        const bool fixed = bf16 && (f11 || f4) && d_out <= 128;
        CHECK((p.kind == MLP_KIND_FIXED) == fixed);
        CHECK((p.kind == MLP_KIND_F32) == !bf16);
        CHECK((p.kind == MLP_KIND_ANY) == (bf16 && !fixed));
        if (fixed) {
            const MlpKey k = mlp_table_key(p.index);
            CHECK(k.a == (f11 ? 11 : 4) && k.b == 26 && k.c == 20);
        }
    }
    if (p.big_index < 0) CHECK(p.big_lds == 0 && p.big_rows == 0 && p.big_threads == 0);
}

static void check_plans() {
    g_case = "plan";
    const int e1[] = {1, 127, 128, 400, 401, 416, 417, 512, 513};
    const int e2[] = {1, 127, 128, 400, 401, 416, 417, 512, 513, 304, 305, 320, 321};
    uint64_t ctr = 0;
    for (int d_in = 1; d_in <= 256; d_in++)
        for (int d_out = 1; d_out <= 160; d_out++)
            for (int prec = 0; prec < 3; prec++) {
                int w1[12], w2[16], c1 = 0, c2 = 0;
                for (int v : e1) w1[c1++] = v;
                for (int v : e2) w2[c2++] = v;
                for (int s = 0; s < 3; s++) {
                    w1[c1++] = 1 + (int)(hash64(ctr++) % (s == 2 ? 4096 : 640));
                    w2[c2++] = 1 + (int)(hash64(ctr++) % (s == 2 ? 4096 : 640));
                }
                for (int i = 0; i < c1; i++)
                    for (int j = 0; j < c2; j++) check_plan(d_in, w1[i], w2[j], d_out, prec);
            }
    CHECK(g_refused > 0 && g_kind[0] > 0 && g_kind[1] > 0 && g_kind[2] > 0 && g_kind[3] > 0);
    // the shapes the GPU suite names
    CHECK(plan_mlp(162, 400, 300, 50, -1.f, EV2G_MLP_BF16).index == mlp_s16_index(0, 1, 1) && plan_mlp(63, 400, 300, 20, 0.f, EV2G_MLP_F32X3).index == mlp_s16_index(1, 3, 1));
    CHECK(mlp_kernel_name(plan_mlp(170, 410, 300, 50, -1.f, EV2G_MLP_BF16).index) == "ev2g_mlp3_fixed<11,26,20>");
    CHECK(mlp_kernel_name(plan_mlp(63, 410, 300, 20, -1.f, EV2G_MLP_BF16).index) == "ev2g_mlp3_fixed<4,26,20>");
    CHECK(plan_mlp(20, 520, 64, 5, -1.f, EV2G_MLP_BF16).kind == MLP_KIND_ANY && plan_mlp(17, 40, 70, 3, -1.f, EV2G_MLP_F32).kind == MLP_KIND_F32);
    CHECK(same(plan_mlp(20, 3000, 64, 5, -1.f, EV2G_MLP_BF16).refusal, kTooWide));
    // the refusals' order: sizes, out_lo, precision, LDS
    const int bad[4][4] = {{0, 8, 8, 8}, {8, -1, 8, 8}, {8, 8, 0, 8}, {8, 8, 8, 0}};
    for (const auto &b : bad) {
        const MlpPlan p = plan_mlp(b[0], b[1], b[2], b[3], 0.5f, 7);
        CHECK(p.err == EV2G_ERR_ARG && same(p.refusal, kBadArgs));
    }
    CHECK(same(plan_mlp(8, 8, 8, 8, 0.5f, 7).refusal, kOutLo) && same(plan_mlp(8, 3000, 8, 8, 1.0f, EV2G_MLP_BF16).refusal, kOutLo));
    CHECK(same(plan_mlp(8, 8, 8, 8, 0.0f, 7).refusal, kPrecision) && same(plan_mlp(8, 3000, 8, 8, -1.0f, -1).refusal, kPrecision));
    CHECK(plan_mlp(8, 8, 8, 8, 0.0f, EV2G_MLP_F32).err == EV2G_OK);
    // the table's index functions and the names, entry by entry
    g_case = "table";
    const char *names[MLP_TABLE_ENTRIES] = {"ev2g_mlp3_any", "ev2g_mlp3_fixed<11,26,20>", "ev2g_mlp3_fixed<4,26,20>", "ev2g_mlp3_f32",
                                            "ev2g_mlp3_s16<6,25,19,4,1,8>", "ev2g_mlp3_s16<6,25,19,4,2,4>", "ev2g_mlp3_s16<6,25,19,4,3,4>",
                                            "ev2g_mlp3_s16<2,25,19,2,1,8>", "ev2g_mlp3_s16<2,25,19,2,2,4>", "ev2g_mlp3_s16<2,25,19,2,3,4>",
                                            "ev2g_mlp3_s16<6,25,19,4,1,4,2>", "ev2g_mlp3_s16<2,25,19,2,1,4,2>"};
    for (int i = 0; i < MLP_TABLE_ENTRIES; i++) {
        const MlpKey k = mlp_table_key(i);
        CHECK(mlp_kernel_name(i) == names[i]);
        if (k.kind == MLP_KIND_FIXED) CHECK(mlp_fixed_index(k.a, k.b, k.c) == i);
        if (k.kind == MLP_KIND_S16) CHECK(mlp_s16_index(k.a == 6 ? 0 : 1, k.nw, k.rb) == i && (k.a == 6 || k.a == 2));
        if (k.kind == MLP_KIND_ANY) CHECK(i == 0);
        if (k.kind == MLP_KIND_F32) CHECK(i == 3);
    }
    CHECK(mlp_fixed_index(11, 26, 19) == -1 && mlp_fixed_index(5, 26, 20) == -1);
}

// ---- c. bf16 rounding ----
// round to nearest, ties to even, on the word's halves: the high half goes up by one when the low half is above the midpoint, or at it with an odd
// high half; a carry out of the high half is dropped (what the function under test does with the non-finite encodings 0x7fff.... / 0xffff....)
static uint16_t want_bf16_bits(uint32_t u) {
    const uint32_t hi = u >> 16, lo = u & 0xffffu;
    const bool up = lo > 0x8000u || (lo == 0x8000u && (hi & 1u));
    return (uint16_t)((hi + (up ? 1u : 0u)) & 0xffffu);
}
static uint16_t want_bf16(float f) { uint32_t u; std::memcpy(&u, &f, 4); return want_bf16_bits(u); }
static float bf16_value(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float f; std::memcpy(&f, &u, 4); return f; }

static void check_bf16() {
    g_case = "host_bf16";
    const uint32_t lows[] = {0x0000u, 0x0001u, 0x7fffu, 0x8000u, 0x8001u, 0xffffu};
    for (uint32_t hi = 0; hi < 0x10000u; hi++)
        for (uint32_t lo : lows) {
            const uint32_t u = (hi << 16) | lo;
            float f;
            std::memcpy(&f, &u, 4);
            CHECK(host_bf16(f) == want_bf16_bits(u));
        }
    CHECK(host_bf16(1.0f) == 0x3f80 && host_bf16(-2.0f) == 0xc000 && host_bf16(1.00390625f) == 0x3f80 && host_bf16(1.01171875f) == 0x3f82);
}

// ---- b. the three weight layouts ----
static std::vector<float> random_weights(size_t n, uint64_t seed) {   // uniform in (-0.25, 0.25), never tiny: normal float32 values
    std::vector<float> w(n);
    for (size_t i = 0; i < n; i++) {
        const double u = (double)(hash64(seed * 0x100000001b3ull + i) >> 11) / 9007199254740992.0;
        w[i] = (float)((u < 0.5 ? -1.0 : 1.0) * (0.001 + 0.249 * std::fabs(2.0 * u - 1.0)));
    }
    return w;
}

// pack_linear's comment: [n_tile][k_step][lane][8]; lane l of tile (nt, ks) holds W[j][k] for j = nt*32 + (l & 31), k = ks*16 + (l >> 5)*8 + 0..7
static std::vector<uint16_t> want_linear(const float *W, int n_out, int n_in, int N, int K) {
    std::vector<uint16_t> p((size_t)N * K, 0);
    for (int j = 0; j < n_out; j++)
        for (int k = 0; k < n_in; k++) {
            const size_t tile = (size_t)(j / 32) * (K / 16) + k / 16, lane = (size_t)(j % 32) + 32 * ((k % 16) / 8);
            p[(tile * 64 + lane) * 8 + k % 8] = want_bf16(W[(size_t)j * n_in + k]);
        }
    return p;
}
// pack_linear_s16's: [tile of 16 outputs][k-step of 32][term][lane][8]; lane l holds W[tile*16 + (l & 15)][ks*32 + 8*(l >> 4) + 0..7]; term t is the bf16
// rounding of what terms 0..t-1 left
static std::vector<uint16_t> want_linear_s16(const float *W, int n_out, int n_in, int NT, int KS, int NW) {
    std::vector<uint16_t> p((size_t)NT * KS * NW * 512, 0);
    for (int j = 0; j < n_out; j++)
        for (int k = 0; k < n_in; k++) {
            const size_t frag = (size_t)(j / 16) * KS + k / 32, lane = (size_t)(j % 16) + 16 * ((k % 32) / 8);
            const float w = W[(size_t)j * n_in + k];
            float left = w;
            double sum = 0.0;
            for (int t = 0; t < NW; t++) {
                const uint16_t term = want_bf16(left);
                p[((frag * NW + t) * 64 + lane) * 8 + k % 8] = term;
                left = left - bf16_value(term);
                sum += (double)bf16_value(term);
            }
            // two terms carry 16 significant bits of the weight, three all 24
            if (NW == 2) CHECK(std::fabs((double)w - sum) <= std::ldexp(std::fabs((double)w), -16));
            if (NW == 3) CHECK(std::fabs((double)w - sum) <= std::ldexp(std::fabs((double)w), -24));
        }
    return p;
}
// pack_linear_f32's: [n_tile][k_group of 8][lane][4], lane l <-> (n = tile*32 + (l & 31), k = 8 g + 4 (l >> 5) + 0..3)
static std::vector<float> want_linear_f32(const float *W, int n_out, int n_in, int N, int K) {
    std::vector<float> p((size_t)N * K, 0.f);
    for (int n = 0; n < n_out; n++)
        for (int k = 0; k < n_in; k++) {
            const size_t group = (size_t)(n / 32) * (K / 8) + k / 8, lane = (size_t)(n % 32) + 32 * ((k % 8) / 4);
            p[(group * 64 + lane) * 4 + k % 4] = W[(size_t)n * n_in + k];
        }
    return p;
}
template <typename T>
static bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static std::vector<float> want_padded(const float *b, int n, int N) {
    std::vector<float> v((size_t)N, 0.f);
    for (int i = 0; i < n; i++) v[(size_t)i] = b[i];
    return v;
}

static void check_layouts() {
    const int shapes[6][2] = {{1, 1}, {17, 33}, {20, 63}, {50, 162}, {300, 400}, {400, 162}};   // (outputs, inputs)
    for (const auto &s : shapes) {
        const int n_out = s[0], n_in = s[1];
        g_case = "layout " + std::to_string(n_out) + "x" + std::to_string(n_in);
        const std::vector<float> W = random_weights((size_t)n_out * n_in, (uint64_t)(n_out * 1000 + n_in));
        // the paddings a plan gives a layer: columns to 32; inputs to 16 (layer 1) or 32 (a hidden layer's padded width); the streaming kernel's tiles of
        // 16 and k-steps of 32, also inside a larger instantiation; the actor-critic's inputs to 8
        const int N = ceil_to(n_out, 32);
        for (int K : {ceil_to(n_in, 16), ceil_to(n_in, 32)}) {
            CHECK(same_bits(pack_linear(W.data(), n_out, n_in, N, K), want_linear(W.data(), n_out, n_in, N, K)));
            CHECK(same_bits(pack_linear_f32(W.data(), n_out, n_in, N, K), want_linear_f32(W.data(), n_out, n_in, N, K)));
        }
        CHECK(same_bits(pack_linear_f32(W.data(), n_out, n_in, N + 32, ceil_to(n_in, 8)), want_linear_f32(W.data(), n_out, n_in, N + 32, ceil_to(n_in, 8))));
        const int NT = ceil_to(n_out, 16) / 16, KS = ceil_to(n_in, 32) / 32;
        for (int NW = 1; NW <= 3; NW++) {
            CHECK(same_bits(pack_linear_s16(W.data(), n_out, n_in, NT, KS, NW), want_linear_s16(W.data(), n_out, n_in, NT, KS, NW)));
            CHECK(same_bits(pack_linear_s16(W.data(), n_out, n_in, NT + 3, KS + 2, NW), want_linear_s16(W.data(), n_out, n_in, NT + 3, KS + 2, NW)));
        }
    }
}

// ---- d. pack_mlp: every image of a network, the streaming kernel's single bias array among them ----
static void check_images() {
    const int nets[5][4] = {{162, 400, 300, 50}, {63, 400, 300, 20}, {17, 40, 70, 3}, {170, 410, 300, 50}, {1, 128, 1, 1}};
    for (const auto &n : nets)
        for (int prec = 0; prec < 3; prec++) {
            const int d_in = n[0], h1 = n[1], h2 = n[2], d_out = n[3];
            g_case = "images " + std::to_string(d_in) + "-" + std::to_string(h1) + "-" + std::to_string(h2) + "-" + std::to_string(d_out) + " precision " + std::to_string(prec);
            const std::vector<float> W1 = random_weights((size_t)h1 * d_in, 1), W2 = random_weights((size_t)h2 * h1, 2), W3 = random_weights((size_t)d_out * h2, 3);
            const std::vector<float> b1 = random_weights((size_t)h1, 4), b2 = random_weights((size_t)h2, 5), b3 = random_weights((size_t)d_out, 6);
            const MlpPlan p = plan_mlp(d_in, h1, h2, d_out, -1.0f, prec);
            CHECK(p.err == EV2G_OK);
            const MlpImages m = pack_mlp(p, W1.data(), b1.data(), W2.data(), b2.data(), W3.data(), b3.data());
            const float *W[3] = {W1.data(), W2.data(), W3.data()};
            const float *b[3] = {b1.data(), b2.data(), b3.data()};
            const int outs[3] = {h1, h2, d_out}, ins[3] = {d_in, h1, h2};
            if (p.kind == MLP_KIND_S16) {
                const bool narrow = d_in <= 64 && d_out <= 32;
                const int NT[3] = {25, 19, narrow ? 2 : 4}, KS[3] = {narrow ? 2 : 6, 13, 10};   // 400 = 25 tiles -> 13 k-steps, 304 = 19 -> 10
                for (int i = 0; i < 3; i++) {
                    CHECK(m.w32[i].empty() && same_bits(m.w16[i], want_linear_s16(W[i], outs[i], ins[i], NT[i], KS[i], prec + 1)));
                    CHECK(m.weight(i) == m.w16[i].data() && m.weight_bytes(i) == m.w16[i].size() * 2);
                }
                // b1 | b2 | b3, each padded with zeros to its tiles
                CHECK(m.bias_off[0] == 0 && m.bias_off[1] == 400 && m.bias_off[2] == 704 && m.bias[1].empty() && m.bias[2].empty());
                std::vector<float> all((size_t)(704 + NT[2] * 16), 0.f);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < outs[i]; j++) all[(size_t)(m.bias_off[i] + j)] = b[i][j];
                CHECK(same_bits(m.bias[0], all));
                continue;
            }
            const int Np[3] = {ceil_to(h1, 32), ceil_to(h2, 32), ceil_to(d_out, 32)}, Kp[3] = {ceil_to(d_in, 16), Np[0], Np[1]};
            for (int i = 0; i < 3; i++) {
                if (prec == EV2G_MLP_BF16) CHECK(m.w32[i].empty() && same_bits(m.w16[i], want_linear(W[i], outs[i], ins[i], Np[i], Kp[i])) && m.weight_bytes(i) == (size_t)Np[i] * Kp[i] * 2);
                else CHECK(m.w16[i].empty() && same_bits(m.w32[i], want_linear_f32(W[i], outs[i], ins[i], Np[i], Kp[i])) && m.weight(i) == m.w32[i].data() && m.weight_bytes(i) == (size_t)Np[i] * Kp[i] * 4);
                CHECK(m.bias_off[i] == 0 && same_bits(m.bias[i], want_padded(b[i], outs[i], Np[i])));
            }
        }
}

// ---- e. the actor-critic ----
static void check_ac() {
    const int nets[3][6] = {{192, 256, 256, 256, 256, 64}, {63, 64, 64, 64, 64, 20}, {17, 33, 5, 40, 7, 3}};   // d_in, h1, h2, v1, v2, d_out (the first: the limits)
    for (const auto &n : nets) {
        const int d_in = n[0], h1 = n[1], h2 = n[2], v1 = n[3], v2 = n[4], d_out = n[5];
        g_case = "actor-critic d_in " + std::to_string(d_in);
        const AcPlan p = plan_ac(d_in, h1, h2, v1, v2, d_out);
        CHECK(p.d_in == d_in && p.h1 == h1 && p.h2 == h2 && p.v1 == v1 && p.v2 == v2 && p.d_out == d_out);
        // inputs padded to 8, every layer's columns to 32
        CHECK(p.k1 == ceil_to(d_in, 8) && p.n1 == ceil_to(h1, 32) && p.n2 == ceil_to(h2, 32) && p.m1 == ceil_to(v1, 32) && p.m2 == ceil_to(v2, 32) && p.n3 == ceil_to(d_out, 32));
        const std::vector<float> pW1 = random_weights((size_t)h1 * d_in, 11), pb1 = random_weights((size_t)h1, 12), pW2 = random_weights((size_t)h2 * h1, 13),
                                 pb2 = random_weights((size_t)h2, 14), vW1 = random_weights((size_t)v1 * d_in, 15), vb1 = random_weights((size_t)v1, 16),
                                 vW2 = random_weights((size_t)v2 * v1, 17), vb2 = random_weights((size_t)v2, 18), aW = random_weights((size_t)d_out * h2, 19),
                                 ab = random_weights((size_t)d_out, 20), cW = random_weights((size_t)v2, 21), cb = random_weights(1, 22);
        const AcWeights w{pW1.data(), pb1.data(), pW2.data(), pb2.data(), vW1.data(), vb1.data(), vW2.data(), vb2.data(), aW.data(), ab.data(), cW.data(), cb.data()};
        const auto img = pack_ac(p, w);
        const auto sizes = ac_array_sizes(p);
        CHECK(AC_ARRAYS == 12 && img.size() == 12 && sizes.size() == 12);
        const std::vector<float> want[12] = {
            want_linear_f32(pW1.data(), h1, d_in, p.n1, p.k1), want_padded(pb1.data(), h1, p.n1), want_linear_f32(pW2.data(), h2, h1, p.n2, p.n1),
            want_padded(pb2.data(), h2, p.n2), want_linear_f32(aW.data(), d_out, h2, p.n3, p.n2), want_padded(ab.data(), d_out, p.n3),
            want_linear_f32(vW1.data(), v1, d_in, p.m1, p.k1), want_padded(vb1.data(), v1, p.m1), want_linear_f32(vW2.data(), v2, v1, p.m2, p.m1),
            want_padded(vb2.data(), v2, p.m2), want_padded(cW.data(), v2, p.m2), want_padded(cb.data(), 1, 1)};
        for (int i = 0; i < 12; i++) CHECK(sizes[(size_t)i] == want[i].size() && same_bits(img[(size_t)i], want[i]));
        // unpack_ac inverts pack_ac: the twelve arrays come back bit for bit, and nothing is written past an array's own size
        const std::vector<float> *src[12] = {&pW1, &pb1, &pW2, &pb2, &vW1, &vb1, &vW2, &vb2, &aW, &ab, &cW, &cb};
        std::vector<float> back[12];
        float *out[12];
        const float guard = 12345.f;
        for (int i = 0; i < 12; i++) { back[i].assign(src[i]->size() + 1, guard); out[i] = back[i].data(); }
        unpack_ac(p, img, out);
        for (int i = 0; i < 12; i++) {
            CHECK(back[i].back() == guard);
            back[i].pop_back();
            CHECK(same_bits(back[i], *src[i]));
        }
    }
    // plan_ac's refusals: each limit holds, one past it (and zero) names its width in ev2g_ac_create's words, the first bad width in argument order wins
    g_case = "actor-critic refusals";
    const int ok[6] = {192, 256, 256, 256, 256, 64};   // d_in, h1, h2, v1, v2, d_out at their limits
    const char *const word[6] = {"d_in must be 1 .. 192", "h1 must be 1 .. 256", "h2 must be 1 .. 256", "v1 must be 1 .. 256", "v2 must be 1 .. 256", "d_out must be 1 .. 64"};
    CHECK(plan_ac(ok[0], ok[1], ok[2], ok[3], ok[4], ok[5]).err == EV2G_OK && plan_ac(1, 1, 1, 1, 1, 1).err == EV2G_OK);
    CHECK(plan_ac(1, 1, 1, 1, 1, 1).refusal.empty());
    for (int i = 0; i < 6; i++)
        for (int bad : {ok[i] + 1, 0, -1}) {
            int n[6];
            for (int j = 0; j < 6; j++) n[j] = j == i ? bad : ok[j] - 1;
            const AcPlan p = plan_ac(n[0], n[1], n[2], n[3], n[4], n[5]);
            CHECK(p.err == EV2G_ERR_ARG && p.refusal == std::string("ev2g_ac_create: ") + word[i]);
            for (int j = i + 1; j < 6; j++) {   // a second bad width behind it does not change the message
                int m[6];
                for (int k = 0; k < 6; k++) m[k] = k == j ? ok[k] + 1 : n[k];
                CHECK(plan_ac(m[0], m[1], m[2], m[3], m[4], m[5]).refusal == p.refusal);
            }
            n[i] = bad > 0 ? ok[i] : 1;   // the limit itself, and the smallest width
            CHECK(plan_ac(n[0], n[1], n[2], n[3], n[4], n[5]).err == EV2G_OK);
        }
}

int main() {
    check_bf16();
    check_plans();
    check_layouts();
    check_images();
    check_ac();
    std::printf("plans %lld (refused %lld; any %lld fixed %lld f32 %lld streaming %lld)\n", g_plans, g_refused, g_kind[0], g_kind[1], g_kind[2], g_kind[3]);
    std::printf("policy_plan_check: ok\n");
    return 0;
}
