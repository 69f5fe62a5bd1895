// What the units of the CondUNetTiny evaluator and sampler share (unet_cond.hip, unet_first.hip, unet_head.hip,
// unet_step.hip, unet.hip, sampler.hip): the structs that cross between them and the functions they call in
// each other.  Internal: no other file includes it.
#pragma once
#include "common.hpp"

namespace tcx {

constexpr float kTwoPi = 6.283185307179586f;

// Two structs are kernel parameters AND cross between units.  The kernels keep taking CondTab / StepArgs of
// the unnamed namespace, so their mangled names (which the profile tools match) stay what they were; a
// function defined in another unit cannot have an unnamed-namespace type in its signature, so the fields
// live in a named base and the host code passes that.
struct CondRows {
    const float* bias_img;   // [B][C0] of this evaluation's images (null: per-evaluation k_cond)
    const float* bias_null;  // [C0] the null-token row (CFG's unconditional half)
};

struct StepFields {
    const float* r;       // [Bt][9][HW]
    float out_b;
    int B, H, W, cfg;
    float guidance;
    int mode;
    const float* scal;    // current row of the step table
    const float* x;       // U-Net input image [B][HW] (x_t, or x_e in Heun stage 2)
    float* x_inout;       // sampler state
    float* x2;            // Heun x_e
    float* eps_out;
    const float* z;
    uint64_t seed, step;
    size_t e0;  // element offset of this batch chunk (Philox counter = e0 + i: chunking-invariant noise)
    const float* coef;    // DPM-Solver++ (modes 6 / 7): current row of the coefficient table [TCX_DPM_COEF]
    float* hist;          // DPM-Solver++: the previous step's data prediction x0 [B][HW]
};

namespace {

// One evaluation's view of the sampler's bias table: its images' rows and the null-token row.
struct CondTab : CondRows {};

__device__ __forceinline__ const float* cond_bias_row(const CondTab& ct, int row, int B, int cfg, int C0) {
    return (cfg && row < B) ? ct.bias_null : ct.bias_img + (size_t)(row % B) * C0;
}

struct StepArgs : StepFields {};

}  // namespace

// ---------------------------------------------------------------- workspace plan of one pass
struct Plan {
    int Bt, H, W, C, C2, P0, P1, P2;
    float *bias0, *a64, *b64, *h1, *a32, *b32, *h2, *a16, *b16, *qkv, *r;
    double* gn;
    float* tab;  // GroupNorm scale/shift tables: [11 norms][2][Bt][C2]
    size_t bytes;
    float* sc(int i) const { return tab + (size_t)(2 * i) * Bt * C2; }
    float* sh(int i) const { return tab + (size_t)(2 * i + 1) * Bt * C2; }
};

inline int groups_of(int ch) {
    for (int g : {8, 4, 2})
        if (ch % g == 0) return g;
    return 1;
}

// the scale / shift tables of norm idx from its partials (ns splits in gn)
inline int gn_tab(const tcx_unet* net, const Plan& P, int idx, int HW, int C, const double* gn, int ns, hipStream_t st) {
    return tcx_gn_finalize(gn, P.Bt, HW, C, groups_of(C), ns, net->gn_w[idx], net->gn_b[idx], 1e-5f, P.sc(idx),
                           P.sh(idx), st);
}

// split-path context of one evaluation (on: sources are h2 and the f16x3 conv runs)
struct H2Ctx {
    bool on;
    unsigned* ovf;
    bool bf;  // precision 2: bf16 records, one bf16 MFMA per product (no range limit, no flag)
    int fmt;  // conv / writer format flag: 0 h2, 1 bf16 records, 2 two-byte bf16 ("b2", h2.hpp: config 5)
};

// One (possibly chunked) U-Net evaluation + sampler step: tcx_unet_eval's arguments, then e_base, the
// element offset of x[0] within the whole sampling batch (the Philox noise counter of element i is
// e_base + i, so a batch evaluated in pieces — chunks or concurrent lanes — draws the same noise as in
// one piece), and the evaluation's rows of the sampler's conditioning table (none: k_cond runs).
struct EvalArgs {
    const tcx_unet* net;
    const float *x, *t, *y_cont, *scal, *z, *coef;
    float *x2, *x_inout, *eps_out, *hist;
    const int64_t* y_cat;
    int t_per_sample, B, H, W, mode;
    float guidance;
    uint64_t seed, step;
    void* ws;
    size_t ws_bytes, e_base;
    hipStream_t stream;
    CondRows ct;
};

// The sampler's conditioning tables in the caller's workspace (make_cond_maps): tmaps [n_t][time_ch],
// cmaps [B + 1][cond_ch] (row B: null token), then the first-conv bias rows [n_t][B + 1][base_ch].
struct CondMaps {
    float* buf = nullptr;
    int time_ch = 0, cond_ch = 0, C0 = 0, B = 0, n_t = 0;
    float* tmaps() const { return buf; }
    float* cmaps() const { return buf + (size_t)n_t * time_ch; }
    float* bias() const { return cmaps() + (size_t)(B + 1) * cond_ch; }
    CondRows at(int step, int b0) const {
        if (!buf) return CondRows{};
        const float* row0 = bias() + (size_t)step * (B + 1) * C0;
        return CondRows{row0 + (size_t)b0 * C0, row0 + (size_t)B * C0};
    }
};

// unet_cond.hip
int launch_cond(const tcx_unet* net, const float* t, int t_per_sample, const int64_t* y_cat, const float* y_cont,
                int B, int cfg, int Bt, float* bias_b, hipStream_t st);
int launch_fold_bias(const CondRows& ct, int C0, int B, int cfg, int Bt, float* bias_b, hipStream_t st);
size_t cond_tab_bytes(const tcx_unet* net, int B, int n_t);
int make_cond_maps(const tcx_unet* net, const float* scal_table, int n_t, const int64_t* y_cat, const float* y_cont,
                   int B, hipStream_t st, void* tab, CondMaps& cm);

// unet_first.hip: down1's first conv into P.a64 with the GroupNorm partials of norm 0 (*ns splits in P.gn), or,
// *first_fused, with silu(GroupNorm_0(.)) already applied and written as down1.net.3's records
int first_conv(const tcx_unet* net, const Plan& P, const float* x, int B, int cfg, const CondRows& ct, const H2Ctx& h2,
               hipStream_t st, int* ns, bool* first_fused);

// unet_head.hip: r = head partials of P.a64 under the tables of norm 10
int launch_head(const tcx_unet* net, const Plan& P, int fmt, hipStream_t st);

// unet_step.hip
int launch_step(const StepFields& a, hipStream_t st);

// unet.hip
int validate(const tcx_unet* net, int B, int H, int W);
size_t lane_ws_bytes(const tcx_unet* net, int Bt, int H, int W, int L);
int unet_eval_impl(const EvalArgs& a);

// sampler.hip
int lanes_setting();
int injected_failure();

}  // namespace tcx
