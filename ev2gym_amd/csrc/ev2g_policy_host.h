// ev2g_policy_host.h -- the host-only half of a policy object: which actor kernel a network gets, and the weight images that kernel reads.
//
// plan_mlp(sizes, out_lo, precision) is the whole decision of ev2g_mlp_create_ex: the refusals, the padded sizes, the kernel (a kind and an
// index into ev2g_host.hip's kMlpTable), the streaming kernel's fragment packing (the FusedPacking route_fused reads), LDS bytes, rows per
// workgroup and threads, and the 32-row variant bf16 streaming policies run on large batches.  pack_mlp(plan, weights) builds the host
// images of the three weight matrices in that kernel's MFMA fragment order and of the biases.  plan_ac is the same for the Gaussian
// actor-critic (ev2g_ac.h), which reads float32 operands in ev2g_mlp3_f32's layout, and ac_params(plan) is the one table of its thirteen
// parameter arrays: pack_ac / unpack_ac / ac_array_sizes, the offsets and slabs of plan_ppo (the plan of its PPO learner, ev2g_ppo.h: accepted
// widths, LDS layout, grid cap, workspace) and ppo_map (where the learner's kernels place every element) are loops over it.  ev2g_host.hip is
// the device stage: it uploads the images and launches the table's entry.  mlp_image_map(plan, images) is pack_mlp's inverse element by element: where
// element (n, k) of a layer sits in its image and which bf16 term it is (the TD3 learner's refresh writes by it, ev2g_td3.h).  Nothing here needs HIP, a handle or a kernel header, so a plain C++17 program can
// enumerate the plan and check every packed element (tests/host/policy_plan_check.cpp, ppo_plan_check.cpp).
//
// The LDS geometry of the actor kernels lives here too, as constexpr functions of ints: ev2g_mlp.h includes this header and lays its LDS
// out by them, so the plan's byte counts and the kernels' pointers come from one definition.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_route_host.h"

// ---- LDS geometry (shared with the kernels of ev2g_mlp.h) ----
#define EV2G_MLP_ROWS 32     // env rows per workgroup of ev2g_mlp3_any / _fixed / _f32
#define EV2G_MLP_BLOCK 256
#define EV2G_MLPS_ROWS 16    // env rows per block of rows of ev2g_mlp3_s16
#define EV2G_MLPS_RING 52

constexpr int ev2g_mlp_lds_stride(int k) { return k + 8; }   // bf16 elements per LDS row: +16 bytes against bank conflicts
constexpr size_t ev2g_mlp_lds_bytes(int k1, int n1, int n2, int n3) {
    return (size_t)EV2G_MLP_ROWS * (ev2g_mlp_lds_stride(k1 > n2 ? k1 : n2) + ev2g_mlp_lds_stride(n1)) * sizeof(uint16_t) +
           (size_t)(n1 + n2 + n3) * sizeof(float);   // + the staged biases
}
constexpr int ev2g_mlp32_lds_stride(int k) { return k + 4; }   // floats per LDS row (+16 bytes against bank conflicts)
constexpr size_t ev2g_mlp32_lds_bytes(int k1, int n1, int n2) {
    return (size_t)EV2G_MLP_ROWS * (ev2g_mlp32_lds_stride(k1 > n2 ? k1 : n2) + ev2g_mlp32_lds_stride(n1)) * sizeof(float);
}

// ev2g_mlp3_s16<KS1, NT1, NT2, NT3, NW, WV, RB>'s constants (ev2g_mlp.h: MlpS16 holds them as template statics).  WV: wavefronts per workgroup
// (4: one per SIMD; 8: two); RB: blocks of 16 env rows per workgroup; NW: bf16 terms per weight.
struct MlpS16Geom {
    int ROWS, NX, KS2, KS3, NTH, MT1, MT2, MT3, S1, S2, S3, STOT, SX, SH1, SH2, NB, RING;
    size_t lds_bytes;
};
constexpr MlpS16Geom mlp_s16_geom(int KS1, int NT1, int NT2, int NT3, int NW, int WV, int RB) {
    MlpS16Geom g{};
    g.ROWS = EV2G_MLPS_ROWS * RB;
    g.NX = NW == 1 ? 1 : 3;   // terms of an activation
    g.KS2 = (NT1 * 16 + 31) / 32; g.KS3 = (NT2 * 16 + 31) / 32;
    g.NTH = WV * 64;
    g.MT1 = (NT1 + WV - 1) / WV; g.MT2 = (NT2 + WV - 1) / WV; g.MT3 = (NT3 + WV - 1) / WV;   // tile slots per wavefront
    g.S1 = g.MT1 * KS1 * NW; g.S2 = g.MT2 * g.KS2 * NW; g.S3 = g.MT3 * g.KS3 * NW; g.STOT = g.S1 + g.S2 + g.S3;   // fragments of the sequence, per layer
    g.SX = KS1 * 32 + 8; g.SH1 = g.KS2 * 32 + 8; g.SH2 = g.KS3 * 32 + 8;   // LDS row strides (bf16 elements; +16 bytes against bank conflicts)
    g.NB = (NT1 + NT2 + NT3) * 16;                                        // staged biases (floats)
    g.RING = (NW == 1 ? EV2G_MLPS_RING : 36) * 4 / WV;                    // (three operand copies per k-step take the registers)
    g.lds_bytes = (size_t)g.ROWS * (g.SX + g.SH1 + g.SH2) * 2 * g.NX + (size_t)g.NB * 4;
    return g;
}

// ---- the actor kernels as a table index and back ----
enum MlpKind {
    MLP_KIND_ANY = 0,   // ev2g_mlp3_any: bf16, any layer widths
    MLP_KIND_FIXED,     // ev2g_mlp3_fixed<K1, K2, K3>: bf16, two shapes next to the shipped ones that the streaming kernel does not cover
    MLP_KIND_F32,       // ev2g_mlp3_f32: float32 operands, any layer widths
    MLP_KIND_S16        // ev2g_mlp3_s16: the streaming kernel, all three precisions
};
// [0] any, [1] fixed<11,26,20>, [2] fixed<4,26,20>, [3] f32, [4, 10) the streaming kernel's 16-row instantiations (4 + 3 * shape + nw - 1;
// shape 0: 192 -> 400 -> 304 -> 64, shape 1: 64 -> 400 -> 304 -> 32), [10, 12) its 32-row bf16 variants of the two shapes.
constexpr int MLP_TABLE_ENTRIES = 12;
struct MlpKey { int kind, a, b, c, d, nw, wv, rb; };   // FIXED: <a, b, c>; S16: <a, b, c, d, nw, wv, rb>
constexpr int mlp_fixed_index(int k1_16, int k2_16, int k3_16) {
    return (k1_16 == 11 && k2_16 == 26 && k3_16 == 20) ? 1 : (k1_16 == 4 && k2_16 == 26 && k3_16 == 20) ? 2 : -1;
}
constexpr int mlp_s16_index(int shape, int nw, int rb) { return rb == 2 ? 10 + shape : 4 + 3 * shape + nw - 1; }
constexpr MlpKey mlp_table_key(int i) {
    // the bf16 network runs eight wavefronts per workgroup (two per SIMD: one's epilogue and LDS waits under the other's MFMAs -- 7.48 -> 7.39 us at
    // 162 inputs, 6.35 -> 5.88 at 63); the float32 modes and the 32-row variant need the registers of four.
    return i == 0 ? MlpKey{MLP_KIND_ANY, 0, 0, 0, 0, 0, 0, 0}
         : i == 1 ? MlpKey{MLP_KIND_FIXED, 11, 26, 20, 0, 0, 0, 0}
         : i == 2 ? MlpKey{MLP_KIND_FIXED, 4, 26, 20, 0, 0, 0, 0}
         : i == 3 ? MlpKey{MLP_KIND_F32, 0, 0, 0, 0, 0, 0, 0}
         : i < 10 ? MlpKey{MLP_KIND_S16, (i - 4) / 3 ? 2 : 6, 25, 19, (i - 4) / 3 ? 2 : 4, (i - 4) % 3 + 1, (i - 4) % 3 == 0 ? 8 : 4, 1}
                  : MlpKey{MLP_KIND_S16, i - 10 ? 2 : 6, 25, 19, i - 10 ? 2 : 4, 1, 4, 2};
}
inline std::string mlp_kernel_name(int i) {
    const MlpKey k = mlp_table_key(i);
    auto n = [](int v) { return std::to_string(v); };
    if (k.kind == MLP_KIND_ANY) return "ev2g_mlp3_any";
    if (k.kind == MLP_KIND_F32) return "ev2g_mlp3_f32";
    if (k.kind == MLP_KIND_FIXED) return "ev2g_mlp3_fixed<" + n(k.a) + "," + n(k.b) + "," + n(k.c) + ">";
    return "ev2g_mlp3_s16<" + n(k.a) + "," + n(k.b) + "," + n(k.c) + "," + n(k.d) + "," + n(k.nw) + "," + n(k.wv) + (k.rb == 1 ? "" : "," + n(k.rb)) + ">";
}

// ---- the plan ----
struct MlpPlan {
    int err = EV2G_OK;              // a refusal: the code ...
    const char *refusal = nullptr;  // ... and the message; nothing below is decided then
    int d_in = 0, h1 = 0, h2 = 0, d_out = 0, precision = EV2G_MLP_BF16;
    int k1 = 0, n1 = 0, n2 = 0, n3 = 0;   // padded: k1 = ceil16(d_in), n1 = ceil32(h1), n2 = ceil32(h2), n3 = ceil32(d_out) (MlpDev's)
    int kind = MLP_KIND_ANY, index = 0;   // the kernel: kMlpTable[index]
    FusedPacking s16;                     // the streaming kernel's fragment packing (zeros: another kernel's)
    size_t lds = 0;
    int rows = EV2G_MLP_ROWS, threads = EV2G_MLP_BLOCK;   // env rows per workgroup of that kernel, its block
    // batches of more rows than 16 x CUs (the device stage knows the CU count): the same bf16 streaming kernel with 32 rows per workgroup -- a
    // weight fragment then feeds two MFMAs, and the weights are streamed once per CU instead of once per 16-row workgroup (two or more of which
    // would share a CU).  -1: the kernel has no such variant.
    int big_index = -1;
    size_t big_lds = 0;
    int big_rows = 0, big_threads = 0;
};

constexpr int mlp_round_up(int x, int m) { return (x + m - 1) / m * m; }

inline MlpPlan plan_mlp(int d_in, int h1, int h2, int d_out, float out_lo, int precision) {
    MlpPlan p;
    auto refuse = [&p](const char *why) { p.err = EV2G_ERR_ARG; p.refusal = why; return p; };
    if (d_in <= 0 || h1 <= 0 || h2 <= 0 || d_out <= 0) return refuse("ev2g_mlp_create: bad arguments");
    if (out_lo != -1.0f && out_lo != 0.0f) return refuse("ev2g_mlp_create: out_lo must be -1 or 0");
    if (precision != EV2G_MLP_BF16 && precision != EV2G_MLP_F32 && precision != EV2G_MLP_F32X3)
        return refuse("ev2g_mlp_create_ex: precision must be EV2G_MLP_BF16, EV2G_MLP_F32 or EV2G_MLP_F32X3");
    p.d_in = d_in; p.h1 = h1; p.h2 = h2; p.d_out = d_out; p.precision = precision;
    p.k1 = mlp_round_up(d_in, 16); p.n1 = mlp_round_up(h1, 32); p.n2 = mlp_round_up(h2, 32); p.n3 = mlp_round_up(d_out, 32);
    // nw: bf16 terms per weight -- 1: the bf16 network; 2 / 3: the float32 network as split bf16 operands (EV2G_MLP_F32 / EV2G_MLP_F32X3, ev2g_mlp.h)
    const int nw = precision == EV2G_MLP_BF16 ? 1 : (precision == EV2G_MLP_F32 ? 2 : 3);
    // The streaming kernel's instantiations are for the shipped shapes (162 / 63 observations -> 400 -> 300 -> 50 / 20 ports); a network that FITS
    // one of them runs on it zero-padded (weights and biases of the missing rows / columns are zeros, ReLU(0) = 0): any input up to 192 (64),
    // hidden layers up to 400 / 304, outputs up to 64 (32).  Small networks (both hidden layers under 128) keep the generic kernel: they would
    // pay the full-size stream.
    const int ks1 = (d_in + 31) / 32, nt1 = (h1 + 15) / 16, nt2 = (h2 + 15) / 16, nt3 = (d_out + 15) / 16;
    int shape = -1;
    if (nt1 <= 25 && nt2 <= 19 && (h1 >= 128 || h2 >= 128)) shape = (ks1 <= 2 && nt3 <= 2) ? 1 : (ks1 <= 6 && nt3 <= 4) ? 0 : -1;
    if (shape >= 0) {
        p.kind = MLP_KIND_S16;
        p.index = mlp_s16_index(shape, nw, 1);
        const MlpKey k = mlp_table_key(p.index);
        p.s16 = FusedPacking{k.a, k.b, k.c, k.d, k.nw};
        p.lds = mlp_s16_geom(k.a, k.b, k.c, k.d, k.nw, k.wv, k.rb).lds_bytes;
        p.rows = EV2G_MLPS_ROWS; p.threads = k.wv * 64;
        if (nw == 1) {
            p.big_index = mlp_s16_index(shape, 1, 2);
            const MlpKey b = mlp_table_key(p.big_index);
            p.big_lds = mlp_s16_geom(b.a, b.b, b.c, b.d, b.nw, b.wv, b.rb).lds_bytes;
            p.big_rows = EV2G_MLPS_ROWS * b.rb; p.big_threads = b.wv * 64;
        }
    } else if (precision != EV2G_MLP_BF16) {
        p.kind = MLP_KIND_F32; p.index = 3;
        p.lds = ev2g_mlp32_lds_bytes(p.k1, p.n1, p.n2);
    } else {
        // the fixed-shape kernels exist for the layer widths of the shipped configs (obs 162 / 63 -> 400 -> 300 -> ports); anything else runs
        // the generic one (the fixed kernels unroll over at most 4 / 3 / 1 column tiles per wavefront: 400 -> 13 tiles, 300 -> 10, ports <= 128)
        const bool narrow = p.n1 / 32 <= 16 && p.n2 / 32 <= 12 && p.n3 / 32 <= 4;
        const int fixed = narrow ? mlp_fixed_index(p.k1 / 16, p.n1 / 16, p.n2 / 16) : -1;
        p.kind = fixed >= 0 ? MLP_KIND_FIXED : MLP_KIND_ANY;
        p.index = fixed >= 0 ? fixed : 0;
        p.lds = ev2g_mlp_lds_bytes(p.k1, p.n1, p.n2, p.n3);
    }
    if (p.lds > 160 * 1024) return refuse("ev2g_mlp_create: layers too wide for the LDS-resident activations");
    return p;
}

// ---- the weight images ----
inline uint16_t host_bf16(float f) {   // round to nearest even (same as the kernel's)
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// torch.nn.Linear weight W[n_out, n_in] -> MFMA B-fragment order [n_tile][k_step][lane][8] (bf16, zero padded):
// lane l of tile (nt, ks) holds B[k][j] = W[j][k] for j = nt*32 + (l & 31), k = ks*16 + (l >> 5)*8 + 0..7
inline std::vector<uint16_t> pack_linear(const float *W, int n_out, int n_in, int N, int K) {
    const int NT = N / 32, KS = K / 16;
    std::vector<uint16_t> p((size_t)NT * KS * 64 * 8, 0);
    for (int nt = 0; nt < NT; nt++)
        for (int ks = 0; ks < KS; ks++)
            for (int l = 0; l < 64; l++) {
                const int j = nt * 32 + (l & 31);
                for (int i = 0; i < 8; i++) {
                    const int k = ks * 16 + (l >> 5) * 8 + i;
                    if (j < n_out && k < n_in) p[(((size_t)nt * KS + ks) * 64 + l) * 8 + i] = host_bf16(W[(size_t)j * n_in + k]);
                }
            }
    return p;
}

// ... and for ev2g_mlp3_s16 (weights are the MFMA's A operand there): [tile of 16 outputs][k-step of 32][term][lane][8],
// lane l holds W[tile*16 + (l & 15)][ks*32 + 8*(l >> 4) + 0..7]; term t of NW is the bf16 rounding of what terms 0..t-1 left of the float32 weight
inline std::vector<uint16_t> pack_linear_s16(const float *W, int n_out, int n_in, int NT, int KS, int NW) {
    std::vector<uint16_t> p((size_t)NT * KS * NW * 64 * 8, 0);
    for (int t = 0; t < NT; t++)
        for (int ks = 0; ks < KS; ks++)
            for (int l = 0; l < 64; l++) {
                const int j = t * 16 + (l & 15);
                for (int i = 0; i < 8; i++) {
                    const int k = ks * 32 + (l >> 4) * 8 + i;
                    if (j >= n_out || k >= n_in) continue;
                    float r = W[(size_t)j * n_in + k];
                    for (int q = 0; q < NW; q++) {
                        const uint16_t hb = host_bf16(r);
                        p[((((size_t)t * KS + ks) * NW + q) * 64 + l) * 8 + i] = hb;
                        uint32_t u = (uint32_t)hb << 16; float hf; std::memcpy(&hf, &u, 4);
                        r -= hf;   // (exact)
                    }
                }
            }
    return p;
}

// float32 weights in the operand order of ev2g_mlp32_layer: [n_tile][k_group of 8][lane][4], lane l <-> (n = tile*32 + (l & 31), k = 8 g + 4 (l >> 5) + 0..3)
inline std::vector<float> pack_linear_f32(const float *W, int n_out, int n_in, int N, int K) {
    std::vector<float> v((size_t)N * K, 0.f);
    const int KG = K / 8;
    for (int nt = 0; nt < N / 32; nt++)
        for (int g = 0; g < KG; g++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 4; j++) {
                    const int n = nt * 32 + (l & 31), k = g * 8 + 4 * (l >> 5) + j;
                    v[(((size_t)nt * KG + g) * 64 + l) * 4 + j] = (n < n_out && k < n_in) ? W[(size_t)n * n_in + k] : 0.f;
                }
    return v;
}

// inverse of pack_linear_f32 / pad_bias: the [n_out, n_in] matrix an image holds (ev2g_ac_get_weights on a policy without a learner)
inline void unpack_linear_f32(const float *img, int n_out, int n_in, int K, float *W) {
    const int KG = K / 8;
    for (int n = 0; n < n_out; n++)
        for (int k = 0; k < n_in; k++)
            W[(size_t)n * n_in + k] = img[(((size_t)(n >> 5) * KG + (k >> 3)) * 64 + (n & 31) + 32 * ((k & 7) >> 2)) * 4 + (k & 3)];
}
// where element (n, k) of a matrix sits in its pack_linear_f32 image of K padded inputs (the device repack of ev2g_ppo.h writes by it)
constexpr size_t packed_f32_index(int n, int k, int K) {
    return (((size_t)(n >> 5) * (size_t)(K / 8) + (size_t)(k >> 3)) * 64 + (size_t)((n & 31) + 32 * ((k & 7) >> 2))) * 4 + (size_t)(k & 3);
}
// ... and of element (p, k) of head `head` (0: mu, 1: log_std) in the SAC actor's stacked-head image: pack_linear_f32 of the [2 n3, n_in] matrix
// whose rows head * n3 + p are the head's, so that each head starts on a 32-column tile (ev2g_sac.h; n3: the ports padded to 32)
constexpr size_t sac_head_index(int head, int p, int k, int n3, int K) { return packed_f32_index(head * n3 + p, k, K); }

inline std::vector<float> pad_bias(const float *b, int n, int N) {
    std::vector<float> v((size_t)N, 0.f);
    std::copy(b, b + n, v.begin());
    return v;
}

// What the device stage uploads for a plan.  Weights: w16 (bf16 fragments) or, for MLP_KIND_F32, w32.  Biases: three arrays padded with zeros to
// n1 / n2 / n3 -- or, for the streaming kernel, ONE array in bias[0] (b1 | b2 | b3, each padded with zeros to its 16-column tiles: one coalesced
// load in the kernel) and bias_off[i], where layer i's starts in it.
struct MlpImages {
    std::vector<uint16_t> w16[3];
    std::vector<float> w32[3];
    std::vector<float> bias[3];
    int bias_off[3] = {0, 0, 0};
    const void *weight(int i) const { return w32[i].empty() ? (const void *)w16[i].data() : (const void *)w32[i].data(); }
    size_t weight_bytes(int i) const { return w32[i].empty() ? w16[i].size() * sizeof(uint16_t) : w32[i].size() * sizeof(float); }
};

inline MlpImages pack_mlp(const MlpPlan &p, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3, const float *b3) {
    MlpImages m;
    if (p.kind == MLP_KIND_S16) {
        const FusedPacking &s = p.s16;
        m.w16[0] = pack_linear_s16(W1, p.h1, p.d_in, s.nt1, s.ks1, s.nw);
        m.w16[1] = pack_linear_s16(W2, p.h2, p.h1, s.nt2, (s.nt1 * 16 + 31) / 32, s.nw);
        m.w16[2] = pack_linear_s16(W3, p.d_out, p.h2, s.nt3, (s.nt2 * 16 + 31) / 32, s.nw);
        m.bias_off[1] = s.nt1 * 16; m.bias_off[2] = (s.nt1 + s.nt2) * 16;
        m.bias[0].assign((size_t)(s.nt1 + s.nt2 + s.nt3) * 16, 0.f);
        std::copy(b1, b1 + p.h1, m.bias[0].begin());
        std::copy(b2, b2 + p.h2, m.bias[0].begin() + m.bias_off[1]);
        std::copy(b3, b3 + p.d_out, m.bias[0].begin() + m.bias_off[2]);
        return m;
    }
    if (p.kind == MLP_KIND_F32) {
        m.w32[0] = pack_linear_f32(W1, p.h1, p.d_in, p.n1, p.k1);
        m.w32[1] = pack_linear_f32(W2, p.h2, p.h1, p.n2, p.n1);
        m.w32[2] = pack_linear_f32(W3, p.d_out, p.h2, p.n3, p.n2);
    } else {
        m.w16[0] = pack_linear(W1, p.h1, p.d_in, p.n1, p.k1);
        m.w16[1] = pack_linear(W2, p.h2, p.h1, p.n2, p.n1);
        m.w16[2] = pack_linear(W3, p.d_out, p.h2, p.n3, p.n2);
    }
    m.bias[0] = pad_bias(b1, p.h1, p.n1); m.bias[1] = pad_bias(b2, p.h2, p.n2); m.bias[2] = pad_bias(b3, p.d_out, p.n3);
    return m;
}

// ---- the Gaussian actor-critic (ev2g_ac.h): float32 operands in ev2g_mlp32_layer's order, inputs padded to 8, every layer's columns to 32 ----
#define EV2G_AC_MAX_IN 192
#define EV2G_AC_MAX_HIDDEN 256
#define EV2G_AC_MAX_OUT 64
// ... and its PPO learner (ev2g_ppo.h)
#define EV2G_PPO_ROWS 32
#define EV2G_PPO_BLOCK 256
#define EV2G_PPO_GRID_CAP 256   // workgroups of the gradient kernel at most (one per CU of an MI355X); more chunks loop
#define EV2G_PPO_ARRAYS 13
#define EV2G_PPO_MAX_IN 192
#define EV2G_PPO_MAX_OUT 64
#define EV2G_PPO_LDS_LIMIT (160 * 1024)

struct AcPlan {
    int d_in, h1, h2, v1, v2, d_out;   // the network's own widths
    int k1, n1, n2, m1, m2, n3;        // padded (AcDev's)
    int err = EV2G_OK;                 // a refusal of ev2g_ac_create: the code ...
    std::string refusal;               // ... and the message; the padded widths are not decided then
};
inline AcPlan plan_ac(int d_in, int h1, int h2, int v1, int v2, int d_out) {
    AcPlan p{d_in, h1, h2, v1, v2, d_out, 0, 0, 0, 0, 0, 0};
    auto refuse = [&p](const char *what, int hi) {
        p.err = EV2G_ERR_ARG; p.refusal = std::string("ev2g_ac_create: ") + what + " must be 1 .. " + std::to_string(hi);
        return p;
    };
    if (d_in < 1 || d_in > EV2G_AC_MAX_IN) return refuse("d_in", EV2G_AC_MAX_IN);
    const int hid[4] = {h1, h2, v1, v2};
    const char *name[4] = {"h1", "h2", "v1", "v2"};
    for (int i = 0; i < 4; i++)
        if (hid[i] < 1 || hid[i] > EV2G_AC_MAX_HIDDEN) return refuse(name[i], EV2G_AC_MAX_HIDDEN);
    if (d_out < 1 || d_out > EV2G_AC_MAX_OUT) return refuse("d_out", EV2G_AC_MAX_OUT);
    p.k1 = mlp_round_up(d_in, 8); p.n1 = mlp_round_up(h1, 32); p.n2 = mlp_round_up(h2, 32);
    p.m1 = mlp_round_up(v1, 32); p.m2 = mlp_round_up(v2, 32); p.n3 = mlp_round_up(d_out, 32);
    return p;
}
constexpr int ppo_k1r(int d_in) { return mlp_round_up(d_in, 32); }   // the learner pads the first layers' inputs to 32 (PpoDev's k1r)

// The network's thirteen parameter arrays, in the one order the ABI, SB3's state dict and the learner's flat buffers share.  Everything that
// places an array -- the images' sizes and packing, the read-back, the learner's offsets, slabs and PpoMap -- is derived from this table.
constexpr int AC_ARRAYS = 12;   // the arrays with a device image: all but log_std
enum AcSlot { AC_NO_IMAGE = -1, AC_W1, AC_B1, AC_W2, AC_B2, AC_W3, AC_B3, AC_U1, AC_C1, AC_U2, AC_C2, AC_U3, AC_C3 };   // AcDev's pointer members, in its order
enum AcSlotT { AC_NO_IMAGE_T = -1, AC_W2T, AC_W3T, AC_U2T };   // PpoDev's transposed images, in its order
struct AcParam {
    const char *name;       // as in messages and in Python (_abi.AC_PARAMS)
    int rows, cols;         // the array's own shape: [out, in] as torch.nn.Linear keeps it; a vector: cols 1
    int slot;               // the AcDev member its image lives in (log_std: AC_NO_IMAGE)
    int img_k;              // the image's padded input width (pack_linear_f32's K); 0: a vector image, element e at e
    size_t img_floats;      // the image's allocated size
    int slot_t, img_t_k;    // the learner's transposed image (pack_linear_f32 of the transpose) and its padded width, or AC_NO_IMAGE_T, 0
    int slab_rows, slab_ld; // the region in a gradient workgroup's slab: rows and row stride (vectors: stride 1)
};
inline std::array<AcParam, EV2G_PPO_ARRAYS> ac_params(const AcPlan &p) {
    const int k1r = ppo_k1r(p.d_in);
    auto mat = [](const char *name, int rows, int cols, int slot, int N, int K, int slot_t, int slab_ld) {
        return AcParam{name, rows, cols, slot, K, (size_t)N * K, slot_t, slot_t == AC_NO_IMAGE_T ? 0 : N, N, slab_ld};
    };
    auto vec = [](const char *name, int n, int slot, int N) { return AcParam{name, n, 1, slot, 0, (size_t)N, AC_NO_IMAGE_T, 0, N, 1}; };
    return {mat("pi_W1", p.h1, p.d_in, AC_W1, p.n1, p.k1, AC_NO_IMAGE_T, k1r), vec("pi_b1", p.h1, AC_B1, p.n1),
            mat("pi_W2", p.h2, p.h1, AC_W2, p.n2, p.n1, AC_W2T, p.n1),         vec("pi_b2", p.h2, AC_B2, p.n2),
            mat("vf_W1", p.v1, p.d_in, AC_U1, p.m1, p.k1, AC_NO_IMAGE_T, k1r), vec("vf_b1", p.v1, AC_C1, p.m1),
            mat("vf_W2", p.v2, p.v1, AC_U2, p.m2, p.m1, AC_U2T, p.m1),         vec("vf_b2", p.v2, AC_C2, p.m2),
            mat("action_W", p.d_out, p.h2, AC_W3, p.n3, p.n2, AC_W3T, p.n2),   vec("action_b", p.d_out, AC_B3, p.n3),
            // the value head: [1, v2] in SB3's layout, but a vector image of m2 floats (the kernel's FMA chain reads it as a row); its bias is one
            // float with a slab region of four
            AcParam{"value_W", 1, p.v2, AC_U3, 0, (size_t)p.m2, AC_NO_IMAGE_T, 0, 1, p.m2},
            AcParam{"value_b", 1, 1, AC_C3, 0, (size_t)1, AC_NO_IMAGE_T, 0, 4, 1},
            AcParam{"log_std", p.d_out, 1, AC_NO_IMAGE, 0, (size_t)0, AC_NO_IMAGE_T, 0, p.n3, 1}};
}

// the twelve host arrays of a network, in the table's order
struct AcWeights { const float *a[AC_ARRAYS]; };
// the twelve device images, in AcDev's order: their sizes, their contents, and the arrays they hold (unpack_ac inverts pack_ac)
inline std::array<size_t, AC_ARRAYS> ac_array_sizes(const AcPlan &p) {
    std::array<size_t, AC_ARRAYS> s{};
    const auto tab = ac_params(p);
    for (int i = 0; i < AC_ARRAYS; i++) s[(size_t)tab[i].slot] = tab[i].img_floats;
    return s;
}
inline std::array<std::vector<float>, AC_ARRAYS> pack_ac(const AcPlan &p, const AcWeights &w) {
    std::array<std::vector<float>, AC_ARRAYS> img;
    const auto tab = ac_params(p);
    for (int i = 0; i < AC_ARRAYS; i++) {
        const AcParam &a = tab[i];
        img[(size_t)a.slot] = a.img_k ? pack_linear_f32(w.a[i], a.rows, a.cols, (int)(a.img_floats / (size_t)a.img_k), a.img_k)
                                      : pad_bias(w.a[i], a.rows * a.cols, (int)a.img_floats);
    }
    return img;
}
inline void unpack_ac(const AcPlan &p, const std::array<std::vector<float>, AC_ARRAYS> &img, float *const out[AC_ARRAYS]) {
    const auto tab = ac_params(p);
    for (int i = 0; i < AC_ARRAYS; i++) {
        const AcParam &a = tab[i];
        const float *src = img[(size_t)a.slot].data();
        if (a.img_k) unpack_linear_f32(src, a.rows, a.cols, a.img_k, out[i]);
        else std::copy(src, src + a.rows * a.cols, out[i]);
    }
}

// ---- the PPO learner of a Gaussian actor-critic (ev2g_ppo.h) ----
// Thirteen gradient arrays in SB3's parameter order: the twelve of AcWeights, then log_std.  The gradient kernel's workgroup keeps, per 32 gathered
// rows, every activation and every layer's delta in LDS (float32 rows of stride width + 4, as ev2g_ac_lds), and its partial sums in a slab of
// its own in the workspace: matrices [padded out][padded in] row-major with the inputs of the first layers padded to 32 (the weight-gradient
// tiles are 32 x 32), vectors padded likewise.
struct PpoLds {   // offsets in floats from the 16-byte aligned base; the first n3 doubles are exp(-2 log_std)
    int sX, sH1, sH2, sV1, sV2, sMU;   // row strides: x, the trunks' hidden layers, the mean (and the actions)
    int oIV, oX, oH1, oH2, oV1, oV2, oMU, oACT, oD1, oD2, oE1, oE2, oROW;   // D / E: the deltas of H / V; ROW: [3][32] per-row head values
    size_t bytes;
};
constexpr PpoLds ppo_lds(int k1r, int n1, int n2, int m1, int m2, int n3) {
    PpoLds l{};
    l.sX = k1r + 4; l.sH1 = n1 + 4; l.sH2 = n2 + 4; l.sV1 = m1 + 4; l.sV2 = m2 + 4; l.sMU = n3 + 4;
    int o = 2 * n3;
    const int R = EV2G_PPO_ROWS;
    l.oIV = 0;
    l.oX = o; o += R * l.sX;
    l.oH1 = o; o += R * l.sH1;
    l.oH2 = o; o += R * l.sH2;
    l.oV1 = o; o += R * l.sV1;
    l.oV2 = o; o += R * l.sV2;
    l.oMU = o; o += R * l.sMU;
    l.oACT = o; o += R * l.sMU;
    l.oD1 = o; o += R * l.sH1;
    l.oD2 = o; o += R * l.sH2;
    l.oE1 = o; o += R * l.sV1;
    l.oE2 = o; o += R * l.sV2;
    l.oROW = o; o += 3 * R;
    l.bytes = (size_t)o * sizeof(float);
    return l;
}

struct PpoPlan {
    int err = EV2G_OK;
    std::string refusal;
    AcPlan ac{};
    int k1r = 0;                            // the first layers' inputs padded to 32
    PpoLds lds{};
    int grid_cap = EV2G_PPO_GRID_CAP;
    int rows[EV2G_PPO_ARRAYS] = {}, cols[EV2G_PPO_ARRAYS] = {};   // the arrays' own shapes (vectors: cols 1)
    int off[EV2G_PPO_ARRAYS + 1] = {};      // where each starts in the flat [n_params] master / m / v / gradient buffers
    int slab_off[EV2G_PPO_ARRAYS] = {}, slab_ld[EV2G_PPO_ARRAYS] = {};   // ... and in a workgroup's slab (row stride; vectors: 1)
    int slab_floats = 0;
    int n_params = 0;
    size_t workspace_bytes = 0;             // grid_cap slabs + grid_cap x 8 doubles of statistics partials
};
inline PpoPlan plan_ppo(int d_in, int h1, int h2, int v1, int v2, int d_out) {
    PpoPlan p;
    auto refuse = [&p](const std::string &why) { p.err = EV2G_ERR_ARG; p.refusal = why; return p; };
    if (d_in < 1 || d_in > EV2G_PPO_MAX_IN) return refuse("ev2g_ppo: d_in " + std::to_string(d_in) + " is outside 1 .. " + std::to_string(EV2G_PPO_MAX_IN));
    if (d_out < 1 || d_out > EV2G_PPO_MAX_OUT) return refuse("ev2g_ppo: d_out " + std::to_string(d_out) + " is outside 1 .. " + std::to_string(EV2G_PPO_MAX_OUT));
    const int hid[4] = {h1, h2, v1, v2};
    const char *name[4] = {"h1", "h2", "v1", "v2"};
    for (int i = 0; i < 4; i++)
        if (hid[i] < 1 || hid[i] > 256) return refuse(std::string("ev2g_ppo: ") + name[i] + " " + std::to_string(hid[i]) + " is outside 1 .. 256");
    p.ac = plan_ac(d_in, h1, h2, v1, v2, d_out);
    const AcPlan &a = p.ac;
    p.k1r = ppo_k1r(d_in);
    p.lds = ppo_lds(p.k1r, a.n1, a.n2, a.m1, a.m2, a.n3);
    if (p.lds.bytes > EV2G_PPO_LDS_LIMIT) {
        int w = 0;   // the widest hidden layer is the one to name
        for (int i = 1; i < 4; i++) if (hid[i] > hid[w]) w = i;
        return refuse(std::string("ev2g_ppo: ") + name[w] + " " + std::to_string(hid[w]) + " is too wide: the gradient kernel's LDS plan takes " +
                      std::to_string(p.lds.bytes) + " bytes of the CU's " + std::to_string(EV2G_PPO_LDS_LIMIT));
    }
    const auto tab = ac_params(a);
    int o = 0, s = 0;
    for (int i = 0; i < EV2G_PPO_ARRAYS; i++) {
        p.rows[i] = tab[i].rows; p.cols[i] = tab[i].cols; p.off[i] = o; o += tab[i].rows * tab[i].cols;
        p.slab_off[i] = s; p.slab_ld[i] = tab[i].slab_ld; s += tab[i].slab_rows * tab[i].slab_ld;
    }
    p.off[EV2G_PPO_ARRAYS] = o; p.n_params = o; p.slab_floats = s;
    p.workspace_bytes = (size_t)p.grid_cap * ((size_t)s * sizeof(float) + 8 * sizeof(double));
    return p;
}

// where the thirteen arrays sit: the flat buffers, the slabs, the packed images.  Passed to the kernels of ev2g_ppo.h by value.
struct PpoMap {
    int off[EV2G_PPO_ARRAYS + 1], cols[EV2G_PPO_ARRAYS], slab_off[EV2G_PPO_ARRAYS], slab_ld[EV2G_PPO_ARRAYS];
    int slab_floats, n_params, P;
    float *img[EV2G_PPO_ARRAYS];    // the image AcDev points at (log_std: null)
    int img_k[EV2G_PPO_ARRAYS];     // a matrix: the padded inputs of its pack_linear_f32 image; a vector: 0 (element i at i)
    float *imgT[EV2G_PPO_ARRAYS];   // the transposed image, or null
    int imgT_k[EV2G_PPO_ARRAYS];
};
// img: the policy's twelve images in AcDev's order (AcSlot); img_t: the learner's three transposed images in PpoDev's (AcSlotT)
inline PpoMap ppo_map(const PpoPlan &pl, float *const img[AC_ARRAYS], float *const img_t[3]) {
    PpoMap mp{};
    const auto tab = ac_params(pl.ac);
    for (int i = 0; i < EV2G_PPO_ARRAYS; i++) {
        const AcParam &a = tab[i];
        mp.off[i] = pl.off[i]; mp.cols[i] = pl.cols[i]; mp.slab_off[i] = pl.slab_off[i]; mp.slab_ld[i] = pl.slab_ld[i];
        mp.img[i] = a.slot == AC_NO_IMAGE ? nullptr : img[a.slot]; mp.img_k[i] = a.img_k;
        mp.imgT[i] = a.slot_t == AC_NO_IMAGE_T ? nullptr : img_t[a.slot_t]; mp.imgT_k[i] = a.img_t_k;
    }
    mp.off[EV2G_PPO_ARRAYS] = pl.off[EV2G_PPO_ARRAYS];
    mp.slab_floats = pl.slab_floats; mp.n_params = pl.n_params; mp.P = pl.ac.d_out;
    return mp;
}

// ---- the element map of a policy's images: the inverse of pack_mlp, element by element (the TD3 learner's refresh, ev2g_td3.h) ----
// Where element (n, k) of a layer's [n_out, n_in] matrix sits in the image pack_mlp built for the plan, for each of its rounding terms: the bf16
// fragment packing (pack_linear: one term), the streaming kernel's 16-column packing (pack_linear_s16: nw terms, term q the bf16 rounding of
// what terms 0 .. q - 1 left), the generic float32 packing (pack_linear_f32: the float itself).  The 32-row variant of a bf16 streaming policy
// reads the same images.  Bias element n of layer i sits at bias[i][n] (the streaming kernel's single array: bias[i] points into it).  Only
// positions (n < n_out, k < n_in) exist in the map: padding is never addressed.
enum MlpImageKind { MLP_IMG_BF16 = 0, MLP_IMG_S16, MLP_IMG_F32 };
struct MlpLayerMap {
    int kind, n_out, n_in;
    int K;            // BF16 / F32: the image's padded input width; S16: its k-steps of 32
    int nw;           // terms per weight (F32: 1, the float itself)
    void *w;          // the image (uint16_t, F32: float)
    float *bias;
    int w_off, b_off; // where the layer's matrix and bias start in a flat buffer W1 | b1 | W2 | b2 | W3 | b3
};
struct MlpImageMap { MlpLayerMap layer[3]; };
constexpr size_t mlp_image_index(const MlpLayerMap &L, int n, int k, int q) {
    return L.kind == MLP_IMG_F32 ? packed_f32_index(n, k, L.K)
         : L.kind == MLP_IMG_BF16 ? (((size_t)(n >> 5) * (size_t)(L.K / 16) + (size_t)(k >> 4)) * 64 + (size_t)((n & 31) + 32 * ((k & 15) >> 3))) * 8 + (size_t)(k & 7)
                                  : ((((size_t)(n >> 4) * (size_t)L.K + (size_t)(k >> 5)) * (size_t)L.nw + (size_t)q) * 64 + (size_t)((n & 15) + 16 * ((k & 31) >> 3))) * 8 + (size_t)(k & 7);
}
inline MlpImageMap mlp_image_map(const MlpPlan &p, void *const w[3], float *const bias[3]) {
    MlpImageMap mp{};
    const int n_out[3] = {p.h1, p.h2, p.d_out}, n_in[3] = {p.d_in, p.h1, p.h2};
    const int pad_in[3] = {p.k1, p.n1, p.n2};
    const FusedPacking &s = p.s16;
    const int ks[3] = {s.ks1, (s.nt1 * 16 + 31) / 32, (s.nt2 * 16 + 31) / 32};
    int off = 0;
    for (int i = 0; i < 3; i++) {
        MlpLayerMap &L = mp.layer[i];
        L.kind = p.kind == MLP_KIND_S16 ? MLP_IMG_S16 : p.kind == MLP_KIND_F32 ? MLP_IMG_F32 : MLP_IMG_BF16;
        L.n_out = n_out[i]; L.n_in = n_in[i];
        L.K = L.kind == MLP_IMG_S16 ? ks[i] : pad_in[i];
        L.nw = L.kind == MLP_IMG_S16 ? s.nw : 1;
        L.w = w[i]; L.bias = bias[i];
        L.w_off = off; off += n_out[i] * n_in[i];
        L.b_off = off; off += n_out[i];
    }
    return mp;
}
