// CondUNetTiny's conditioning (the reference's models/sde_score_model.py:17-82 timestep_embedding and
// ConditionEmbedding, :195-202 time_mlp / to_*_map) folded into the first conv's bias:
//   k_cond       — per evaluation: the conditioning MLPs and the fold of the 16 spatially-constant map channels of
//                  the first conv into a per-(batch, channel) bias (circular padding keeps a constant map
//                  constant, so its 3x3 contribution is sum_taps(w) * value).
//   k_cond_maps, k_bias_table — the sampler's form: every step's and image's bias row once per call.
//   k_fold_bias  — gathers an evaluation's rows of that table for the generic first-conv path.
#include "unet.hpp"

namespace tcx {
namespace {

constexpr float kLn1e4 = 9.210340371976184f;  // math.log(10000.0)

struct CondArgs {
    const float *time_w1t, *time_b1, *time_w2t, *time_b2, *ttm_wt, *ttm_b, *tcm_wt, *tcm_b, *cat_emb, *cmlp_w1t,
        *cmlp_b1, *cmlp_w2t, *cmlp_b2, *cout_wt, *cout_b, *map_wsum, *conv_b;
    int E, n_types, ycd, time_ch, cond_ch, C0;
};

// One block of CT threads per (CFG-doubled) batch row.  Every linear layer is a split-K matvec
// (kgroups of threads each reduce K/kgroups products, then one fixed-order fold over the groups):
// the serial dependency per layer is ~K/8 loads instead of K (one thread per output), which made
// this latency-bound kernel ~58 us per evaluation.
constexpr int CT = 1024;

// out[n] = act(bias[n] + sum_k wt[k*N + n] * in[k]) for n < N (wt: [K][N]); all CT threads call it.
__device__ void cond_mv(const float* __restrict__ wt, const float* __restrict__ bias, const float* in, int K, int N,
                        float* out, float* red, bool silu) {
    const int j = threadIdx.x;
    const int G = max(1, min(CT / N, 16));
    const int n = j % N, g = j / N;
    if (g < G) {
        float s = 0.f;
        for (int k = g; k < K; k += G) s = fmaf(wt[k * N + n], in[k], s);
        red[g * N + n] = s;
    }
    __syncthreads();
    if (j < N) {
        float s = bias[n];
        for (int gg = 0; gg < G; ++gg) s += red[gg * N + n];
        out[n] = silu ? silu_f(s) : s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(CT) void k_cond(CondArgs a, const float* __restrict__ t, int t_per_sample,
                                             const int64_t* __restrict__ y_cat, const float* __restrict__ y_cont,
                                             int B, int cfg, float* __restrict__ bias_b) {
    __shared__ float te[256], h1[256], te2[256], yv[16], g1[256], c2[256], u[512], ce[256], maps[64];
    __shared__ float red[16 * 256];
    const int bb = blockIdx.x;
    const int bs = bb % B;
    const bool null_c = cfg && bb < B;  // first half of a CFG batch = unconditional
    const int E = a.E, half = E / 2;
    const int j = threadIdx.x;
    const float tv = t_per_sample ? t[bs] : t[0];
    if (j < E) {
        // timestep_embedding: freqs = exp(-ln(1e4) * k / max(half-1,1)); args = (2*pi*t) * freqs
        const int k = j < half ? j : j - half;
        const float fr = expf((-kLn1e4 * (float)k) / (float)(half > 1 ? half - 1 : 1));
        const float arg = (kTwoPi * tv) * fr;
        te[j] = j < half ? cosf(arg) : sinf(arg);
    }
    if (j < a.ycd) {
        // y = y_cont; y[1] = sin(theta); y[2] = cos(y[1]).  NB: the reference takes
        // theta = y[:, 1] as a VIEW, so its cos reads the already-replaced sin(theta)
        // (sde_score_model.py:75-78): y[2] = cos(sin(theta)).
        float v = null_c ? 0.f : y_cont[(size_t)bs * a.ycd + j];
        const float th = null_c ? 0.f : y_cont[(size_t)bs * a.ycd + 1];
        if (j == 1) v = sinf(th);
        if (j == 2) v = cosf(sinf(th));
        yv[j] = v;
    }
    __syncthreads();
    cond_mv(a.time_w1t, a.time_b1, te, E, E, h1, red, true);
    cond_mv(a.cmlp_w1t, a.cmlp_b1, yv, a.ycd, E, g1, red, true);
    cond_mv(a.time_w2t, a.time_b2, h1, E, E, te2, red, false);
    cond_mv(a.cmlp_w2t, a.cmlp_b2, g1, E, E, c2, red, false);
    if (j < E) {
        long long yc = null_c ? a.n_types : y_cat[bs];
        yc = yc < 0 ? 0 : (yc > a.n_types ? a.n_types : yc);
        u[j] = silu_f(a.cat_emb[(size_t)yc * E + j]);
        u[E + j] = silu_f(c2[j]);
    }
    __syncthreads();
    cond_mv(a.cout_wt, a.cout_b, u, 2 * E, E, ce, red, false);
    const int nm = a.time_ch + a.cond_ch;
    cond_mv(a.ttm_wt, a.ttm_b, te2, E, a.time_ch, maps, red, false);
    cond_mv(a.tcm_wt, a.tcm_b, ce, E, a.cond_ch, maps + a.time_ch, red, false);
    for (int co = j; co < a.C0; co += CT) {
        float s = a.conv_b[co];
        for (int c = 0; c < nm; ++c) s = fmaf(maps[c], a.map_wsum[co * nm + c], s);
        bias_b[(size_t)bb * a.C0 + co] = s;
    }
}

// Sampler form of the conditioning (round 3): the reference recomputes timestep_embedding + time_mlp
// and ConditionEmbedding for every U-Net call (sde_score_model.py:243-252), but over one sampling
// call t takes only the n_t values of the step table and the condition rows never change.  One
// launch per call computes them all: block i < n_t the time map of t = tvals[i * tstride] (time_ch
// values), block n_t + r the condition map of image r (r == B: the null token with y_cont = 0, the
// unconditional half of every CFG batch).  Same per-value arithmetic as k_cond (cond_mv), so the
// first conv's folded bias (k_conv_first FOLD form) is bit-identical to the per-evaluation path.
__global__ __launch_bounds__(CT) void k_cond_maps(CondArgs a, const float* __restrict__ tvals, int tstride, int n_t,
                                                  const int64_t* __restrict__ y_cat, const float* __restrict__ y_cont,
                                                  int B, float* __restrict__ tmaps, float* __restrict__ cmaps) {
    __shared__ float te[256], h1[256], te2[256], yv[16], g1[256], c2[256], u[512], ce[256];
    __shared__ float red[16 * 256];
    const int E = a.E, half = E / 2;
    const int j = threadIdx.x;
    if ((int)blockIdx.x < n_t) {  // uniform per block
        const float tv = tvals[(size_t)blockIdx.x * tstride];
        if (j < E) {
            const int k = j < half ? j : j - half;
            const float fr = expf((-kLn1e4 * (float)k) / (float)(half > 1 ? half - 1 : 1));
            const float arg = (kTwoPi * tv) * fr;
            te[j] = j < half ? cosf(arg) : sinf(arg);
        }
        __syncthreads();
        cond_mv(a.time_w1t, a.time_b1, te, E, E, h1, red, true);
        cond_mv(a.time_w2t, a.time_b2, h1, E, E, te2, red, false);
        cond_mv(a.ttm_wt, a.ttm_b, te2, E, a.time_ch, tmaps + (size_t)blockIdx.x * a.time_ch, red, false);
        return;
    }
    const int r = blockIdx.x - n_t;
    const bool null_c = r >= B;
    if (j < a.ycd) {  // as k_cond: y[1] = sin(theta), y[2] = cos(sin(theta)) (the reference's view quirk)
        float v = null_c ? 0.f : y_cont[(size_t)r * a.ycd + j];
        const float th = null_c ? 0.f : y_cont[(size_t)r * a.ycd + 1];
        if (j == 1) v = sinf(th);
        if (j == 2) v = cosf(sinf(th));
        yv[j] = v;
    }
    __syncthreads();
    cond_mv(a.cmlp_w1t, a.cmlp_b1, yv, a.ycd, E, g1, red, true);
    cond_mv(a.cmlp_w2t, a.cmlp_b2, g1, E, E, c2, red, false);
    if (j < E) {
        long long yc = null_c ? a.n_types : y_cat[r];
        yc = yc < 0 ? 0 : (yc > a.n_types ? a.n_types : yc);
        u[j] = silu_f(a.cat_emb[(size_t)yc * E + j]);
        u[E + j] = silu_f(c2[j]);
    }
    __syncthreads();
    cond_mv(a.cout_wt, a.cout_b, u, 2 * E, E, ce, red, false);
    cond_mv(a.tcm_wt, a.tcm_b, ce, E, a.cond_ch, cmaps + (size_t)r * a.cond_ch, red, false);
}

// The first-conv bias of every (step, image) of a sampling call: the fold of k_cond (conv_b +
// sum_c maps[c] * map_wsum[co][c], time channels first, the same fmaf order), written once per call
// as bias_tab[n_t][B + 1][C0] (row B: the null token) so an evaluation only reads its rows.
__global__ __launch_bounds__(256) void k_bias_table(const float* __restrict__ tmaps, const float* __restrict__ cmaps,
                                                    const float* __restrict__ map_wsum, const float* __restrict__ conv_b,
                                                    int time_ch, int cond_ch, int C0, int B, int n_t,
                                                    float* __restrict__ bias_tab) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_t * (B + 1) * C0) return;
    const int co = (int)(i % C0);
    const int r = (int)((i / C0) % (B + 1));
    const int step = (int)(i / ((size_t)C0 * (B + 1)));
    const int nm = time_ch + cond_ch;
    const float* tm = tmaps + (size_t)step * time_ch;
    const float* cm = cmaps + (size_t)r * cond_ch;
    float s = conv_b[co];
    for (int c = 0; c < time_ch; ++c) s = fmaf(tm[c], map_wsum[co * nm + c], s);
    for (int c = 0; c < cond_ch; ++c) s = fmaf(cm[c], map_wsum[co * nm + time_ch + c], s);
    bias_tab[i] = s;
}

// generic first-conv path: gather the rows into the per-evaluation bias buffer
__global__ __launch_bounds__(256) void k_fold_bias(CondTab ct, int C0, int B, int cfg, int Bt, float* __restrict__ bias_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Bt * C0) return;
    const int row = i / C0, co = i - row * C0;
    bias_b[i] = cond_bias_row(ct, row, B, cfg, C0)[co];
}

CondArgs cond_args(const tcx_unet* net) {
    CondArgs a{};
    a.time_w1t = net->time_w1t; a.time_b1 = net->time_b1; a.time_w2t = net->time_w2t; a.time_b2 = net->time_b2;
    a.ttm_wt = net->ttm_wt; a.ttm_b = net->ttm_b; a.tcm_wt = net->tcm_wt; a.tcm_b = net->tcm_b;
    a.cat_emb = net->cat_emb; a.cmlp_w1t = net->cmlp_w1t; a.cmlp_b1 = net->cmlp_b1;
    a.cmlp_w2t = net->cmlp_w2t; a.cmlp_b2 = net->cmlp_b2; a.cout_wt = net->cout_wt; a.cout_b = net->cout_b;
    a.map_wsum = net->map_wsum; a.conv_b = net->down1_0.b;
    a.E = net->emb_dim; a.n_types = net->n_types; a.ycd = net->y_cont_dim;
    a.time_ch = net->time_ch; a.cond_ch = net->cond_ch; a.C0 = net->base_ch;
    return a;
}

}  // namespace

// the per-evaluation conditioning: bias_b [Bt][base_ch]
int launch_cond(const tcx_unet* net, const float* t, int t_per_sample, const int64_t* y_cat, const float* y_cont,
                int B, int cfg, int Bt, float* bias_b, hipStream_t st) {
    hipLaunchKernelGGL(k_cond, dim3(Bt), dim3(CT), 0, st, cond_args(net), t, t_per_sample, y_cat, y_cont, B, cfg,
                       bias_b);
    return check_launch("k_cond");
}

int launch_fold_bias(const CondRows& ct, int C0, int B, int cfg, int Bt, float* bias_b, hipStream_t st) {
    hipLaunchKernelGGL(k_fold_bias, dim3(cdiv(Bt * C0, 256)), dim3(256), 0, st, CondTab{ct}, C0, B, cfg, Bt, bias_b);
    return check_launch("k_fold_bias");
}

// The sampler's conditioning tables (k_cond_maps + k_bias_table), carved from the CALLER's workspace
// (tcx_sde_workspace_size / tcx_ode_workspace_size size them; the library never allocates): CondMaps'
// three arrays.  They replace the reference's per-call _make_maps (sde_score_model.py:227-241).
// TCX_COND_HOIST=0 keeps the per-evaluation k_cond (A/B; the tables are then left unused).
size_t cond_tab_bytes(const tcx_unet* net, int B, int n_t) {
    const size_t n = (size_t)n_t * net->time_ch + (size_t)(B + 1) * net->cond_ch + (size_t)n_t * (B + 1) * net->base_ch;
    return align_up(n * 4, 256);
}

// tab: cond_tab_bytes(net, B, n_t) bytes of the caller's workspace, 256-B aligned
int make_cond_maps(const tcx_unet* net, const float* scal_table, int n_t, const int64_t* y_cat, const float* y_cont,
                   int B, hipStream_t st, void* tab, CondMaps& cm) {
    static const bool on = env_on("TCX_COND_HOIST");
    if (!on) return TCX_OK;
    cm.time_ch = net->time_ch; cm.cond_ch = net->cond_ch; cm.C0 = net->base_ch; cm.B = B; cm.n_t = n_t;
    const size_t nbias = (size_t)n_t * (B + 1) * net->base_ch;
    cm.buf = reinterpret_cast<float*>(tab);
    hipLaunchKernelGGL(k_cond_maps, dim3(n_t + B + 1), dim3(CT), 0, st, cond_args(net), scal_table, TCX_SCAL, n_t,
                       y_cat, y_cont, B, cm.tmaps(), cm.cmaps());
    TCX_TRY(check_launch("k_cond_maps"));
    hipLaunchKernelGGL(k_bias_table, dim3((unsigned)((nbias + 255) / 256)), dim3(256), 0, st, cm.tmaps(), cm.cmaps(),
                       net->map_wsum, net->down1_0.b, net->time_ch, net->cond_ch, net->base_ch, B, n_t, cm.bias());
    return check_launch("k_bias_table");
}

}  // namespace tcx
