// Backward of the training attention (AttentionFn, toycrystals_amd/functional.py) without any N x N
// tensor: from qkv, out, dout and the forward's row log-sum-exp (tcx_attention_fwd_lse) two kernels
// recompute P = exp(scale s - lse) tile by tile and write dqkv [Bt,N,3C].  fp32 throughout on
// v_mfma_f32_32x32x2_f32, no atomics: every sum has a fixed order, two runs are bit-equal.
//
//   dP = dO V^T,  dS = P o (dP - delta),  delta[i] = sum_d dO[i][d] O[i][d]
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO
//
// Both kernels mirror the forward's register scheme (attention.hip): the row a lane owns (a query in
// k_attn_bwd_dq, a key in k_attn_bwd_dkv) has its d-vectors in registers as the B operands of the score
// products, the other side of the head streams through LDS, and the 32 x 32 accumulator tile of dS / P
// (row (r&3) + 8(r>>2) + 4 lh of the tile in register r, the lane's own row as the column) is at once
// the B operand of the gradient products, whose A operand is read from LDS in that same row order.
// LDS rows keep the forward's D + 4 stride: the b128 row reads of the score products and the
// lane-per-column reads of the gradient products are both conflict-free at it.
#include "common.hpp"

namespace tcx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int QB = 256;  // rows per workgroup (8 waves x 32 lanes-with-a-row)
constexpr int TL = 128;  // rows of the streamed side per staged tile when N > 256 (N <= 256: all N at once)

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// `rows` rows of two [.][D] head slices (row strides xs / ys floats) into LDS at stride D + 4
template <int D>
__device__ __forceinline__ void stage_pair(float* Xs, float* Ys, const float* __restrict__ x, size_t xs,
                                           const float* __restrict__ y, size_t ys, int rows) {
    constexpr int D4 = D / 4, KS = D + 4;
    for (int i = threadIdx.x; i < rows * D4; i += blockDim.x) {
        const int j = i / D4, d4 = i - (i / D4) * D4;
        *reinterpret_cast<float4*>(Xs + j * KS + d4 * 4) = *reinterpret_cast<const float4*>(x + j * xs + d4 * 4);
        *reinterpret_cast<float4*>(Ys + j * KS + d4 * 4) = *reinterpret_cast<const float4*>(y + j * ys + d4 * 4);
    }
}

// g^T accumulators (d = t*32 + 8i + 4lh + 0..3 in registers 4i..4i+3, the lane's row as the column) * alpha
// -> D floats at dst
template <int D>
__device__ __forceinline__ void store_rows(float* dst, const f32x16* acc, float alpha, int lh) {
#pragma unroll
    for (int t = 0; t < (D + 31) / 32; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t * 32 + 8 * i < D)  // D % 8 == 0: both lane halves' quads are inside
                *reinterpret_cast<float4*>(dst + t * 32 + 8 * i + 4 * lh) =
                    make_float4(acc[t][4 * i] * alpha, acc[t][4 * i + 1] * alpha, acc[t][4 * i + 2] * alpha,
                                acc[t][4 * i + 3] * alpha);
}

// ---------------------------------------------------------------------------------------------
// dQ: the query on the lane.  grid (N / 256 query blocks, heads, Bt), one wave per 32 queries.
// K and V of the head in LDS, kt keys at a time.  Per 32-key tile
//   S^T  = K Q^T   (A = K rows, B = Q^T in registers, d split by lane half as in the forward)
//   dP^T = V dO^T  (A = V rows, B = dO^T in registers)
//   dS^T = exp(scale S^T - lse[q]) (dP^T - delta[q])   in the accumulators
//   dQ^T += K^T dS^T  (A = K read down its columns in the accumulators' key order, B = dS^T)
// The prologue computes delta[q] from dO and O (half of d per lane half + one xor-32 shuffle) and
// stores it for k_attn_bwd_dkv.
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void k_attn_bwd_dq(const float* __restrict__ qkv, const float* __restrict__ out,
                                                     const float* __restrict__ dout, const float* __restrict__ lse,
                                                     float* __restrict__ dqkv, float* __restrict__ delta, int N, int C,
                                                     int kt, float scale) {
    constexpr int HD = D / 2, KS = D + 4, DT = (D + 31) / 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ks = sm;
    float* Vs = sm + kt * KS;
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int q = blockIdx.x * QB + w * 32 + li;
    const size_t rs = 3 * (size_t)C;
    const float* base = qkv + (size_t)b * N * rs + h * D;
    const size_t row = ((size_t)b * gridDim.y + h) * N + q;
    float qf[HD], dof[HD];
    float dl = 0.f;
    {
        const float* qs = base + q * rs + HD * lh;
        const size_t o = ((size_t)b * N + q) * C + h * D + HD * lh;
#pragma unroll
        for (int s4 = 0; s4 < HD / 4; ++s4) {
            const float4 v = *reinterpret_cast<const float4*>(qs + 4 * s4);
            const float4 g = *reinterpret_cast<const float4*>(dout + o + 4 * s4);
            const float4 y = *reinterpret_cast<const float4*>(out + o + 4 * s4);
            qf[4 * s4 + 0] = v.x; qf[4 * s4 + 1] = v.y; qf[4 * s4 + 2] = v.z; qf[4 * s4 + 3] = v.w;
            dof[4 * s4 + 0] = g.x; dof[4 * s4 + 1] = g.y; dof[4 * s4 + 2] = g.z; dof[4 * s4 + 3] = g.w;
            dl = fmaf(g.x, y.x, dl);
            dl = fmaf(g.y, y.y, dl);
            dl = fmaf(g.z, y.z, dl);
            dl = fmaf(g.w, y.w, dl);
        }
    }
    dl += __shfl_xor(dl, 32);
    if (lh == 0) delta[row] = dl;
    const float ls = lse[row];
    f32x16 dq[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) dq[t] = (f32x16){};
    for (int k0 = 0; k0 < N; k0 += kt) {
        __syncthreads();  // previous tile fully consumed
        stage_pair<D>(Ks, Vs, base + k0 * rs + C, rs, base + k0 * rs + 2 * C, rs, kt);
        __syncthreads();
        for (int n = 0; n < kt / 32; ++n) {
            f32x16 s = (f32x16){}, dp = (f32x16){};
            const float* kr = Ks + (n * 32 + li) * KS + HD * lh;
            const float* vr = Vs + (n * 32 + li) * KS + HD * lh;
#pragma unroll
            for (int s4 = 0; s4 < HD / 4; ++s4) {
                const float4 kv = *reinterpret_cast<const float4*>(kr + 4 * s4);
                const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * s4);
                s = mfma(kv.x, qf[4 * s4 + 0], s);
                dp = mfma(vv.x, dof[4 * s4 + 0], dp);
                s = mfma(kv.y, qf[4 * s4 + 1], s);
                dp = mfma(vv.y, dof[4 * s4 + 1], dp);
                s = mfma(kv.z, qf[4 * s4 + 2], s);
                dp = mfma(vv.z, dof[4 * s4 + 2], dp);
                s = mfma(kv.w, qf[4 * s4 + 3], s);
                dp = mfma(vv.w, dof[4 * s4 + 3], dp);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = expf(fmaf(s[r], scale, -ls)) * (dp[r] - dl);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* kc = Ks + (n * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * KS + li;
#pragma unroll
                for (int t = 0; t < DT; ++t) dq[t] = mfma(kc[t * 32], s[r], dq[t]);  // rows d >= D: never stored
            }
        }
    }
    store_rows<D>(dqkv + ((size_t)b * N + q) * rs + h * D, dq, scale, lh);
}

// ---------------------------------------------------------------------------------------------
// dK, dV: the key on the lane.  grid (N / 256 key blocks, heads, Bt), one wave per 32 keys; K^T and V^T
// of the lane's key in registers.  Q and dO of the head in LDS, qt queries at a time, lse and delta of
// those queries beside them.  Per 32-query tile
//   S  = Q K^T,  dP = dO V^T   (A = Q / dO rows, B = K^T / V^T in registers); accumulator rows are
//   queries, so lse / delta come per register quad from LDS (one broadcast b128 each)
//   P = exp(scale S - lse),  dS = P (dP - delta)   in the accumulators
//   dV^T += dO^T P,  dK^T += Q^T dS   (A = dO / Q read down their columns in the accumulators' query order)
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void k_attn_bwd_dkv(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      float* __restrict__ dqkv, int N, int C, int qt, float scale) {
    constexpr int HD = D / 2, KS = D + 4, DT = (D + 31) / 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qs = sm;
    float* Gs = sm + qt * KS;  // dO
    float* Ls = sm + 2 * qt * KS;
    float* Ds = Ls + qt;
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int key = blockIdx.x * QB + w * 32 + li;
    const size_t rs = 3 * (size_t)C;
    const float* base = qkv + (size_t)b * N * rs + h * D;
    const float* gbase = dout + (size_t)b * N * C + h * D;
    const size_t hrow = ((size_t)b * gridDim.y + h) * N;
    float kf[HD], vf[HD];
    {
        const float* ks = base + key * rs + C + HD * lh;
#pragma unroll
        for (int s4 = 0; s4 < HD / 4; ++s4) {
            const float4 k4 = *reinterpret_cast<const float4*>(ks + 4 * s4);
            const float4 v4 = *reinterpret_cast<const float4*>(ks + C + 4 * s4);
            kf[4 * s4 + 0] = k4.x; kf[4 * s4 + 1] = k4.y; kf[4 * s4 + 2] = k4.z; kf[4 * s4 + 3] = k4.w;
            vf[4 * s4 + 0] = v4.x; vf[4 * s4 + 1] = v4.y; vf[4 * s4 + 2] = v4.z; vf[4 * s4 + 3] = v4.w;
        }
    }
    f32x16 dv[DT], dk[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) dv[t] = dk[t] = (f32x16){};
    for (int q0 = 0; q0 < N; q0 += qt) {
        __syncthreads();  // previous tile fully consumed
        stage_pair<D>(Qs, Gs, base + q0 * rs, rs, gbase + (size_t)q0 * C, (size_t)C, qt);
        for (int i = threadIdx.x; i < qt; i += blockDim.x) {
            Ls[i] = lse[hrow + q0 + i];
            Ds[i] = delta[hrow + q0 + i];
        }
        __syncthreads();
        for (int n = 0; n < qt / 32; ++n) {
            f32x16 s = (f32x16){}, dp = (f32x16){};
            const float* qr = Qs + (n * 32 + li) * KS + HD * lh;
            const float* gr = Gs + (n * 32 + li) * KS + HD * lh;
#pragma unroll
            for (int s4 = 0; s4 < HD / 4; ++s4) {
                const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * s4);
                const float4 gv = *reinterpret_cast<const float4*>(gr + 4 * s4);
                s = mfma(qv.x, kf[4 * s4 + 0], s);
                dp = mfma(gv.x, vf[4 * s4 + 0], dp);
                s = mfma(qv.y, kf[4 * s4 + 1], s);
                dp = mfma(gv.y, vf[4 * s4 + 1], dp);
                s = mfma(qv.z, kf[4 * s4 + 2], s);
                dp = mfma(gv.z, vf[4 * s4 + 2], dp);
                s = mfma(qv.w, kf[4 * s4 + 3], s);
                dp = mfma(gv.w, vf[4 * s4 + 3], dp);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // registers 4i .. 4i+3: queries n*32 + 8i + 4lh + 0..3
                const float4 l4 = *reinterpret_cast<const float4*>(Ls + n * 32 + 8 * i + 4 * lh);
                const float4 d4 = *reinterpret_cast<const float4*>(Ds + n * 32 + 8 * i + 4 * lh);
                const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = expf(fmaf(s[4 * i + j], scale, -lq[j]));
                    s[4 * i + j] = p;
                    dp[4 * i + j] = p * (dp[4 * i + j] - dq[j]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = (n * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * KS + li;
#pragma unroll
                for (int t = 0; t < DT; ++t) {  // rows d >= D: never stored
                    dv[t] = mfma(Gs[qrow + t * 32], s[r], dv[t]);
                    dk[t] = mfma(Qs[qrow + t * 32], dp[r], dk[t]);
                }
            }
        }
    }
    float* dst = dqkv + ((size_t)b * N + key) * rs + h * D;
    store_rows<D>(dst + C, dk, scale, lh);
    store_rows<D>(dst + 2 * C, dv, 1.f, lh);
}

// LDS: two [t][D + 4] slices, and for dkv lse and delta of the tile behind them.  The column reads of the
// d >= D lanes (fewer than 32 floats past a slice's last row) land in what follows the slice: V behind K in
// dq, dO behind Q and lse / delta behind dO in dkv.  Their products fill accumulator rows that are never stored.
template <int D>
size_t bwd_lds_bytes(int t, bool dkv) {
    return ((size_t)2 * t * (D + 4) + (dkv ? 2 * t : 0)) * sizeof(float);
}

template <int D>
int launch_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta,
                    int Bt, int N, int C, int heads, hipStream_t st) {
    const float scale = (float)(1.0 / std::sqrt((double)D));
    const int t = N <= QB ? N : TL;
    static bool attr_set = false;  // > 64 KB of dynamic LDS needs the explicit opt-in
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_bwd_dq<D>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_bwd_dkv<D>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
            set_error("tcx_attention_bwd: cannot enable 160 KB dynamic LDS");
            return TCX_EHIP;
        }
        attr_set = true;
    }
    const dim3 grid(cdiv(N, QB), heads, Bt), block(2 * (N < QB ? N : QB));
    hipLaunchKernelGGL((k_attn_bwd_dq<D>), grid, block, bwd_lds_bytes<D>(t, false), st, qkv, out, dout, lse, dqkv,
                       delta, N, C, t, scale);
    TCX_TRY(check_launch("tcx_attention_bwd(dq)"));
    // same stream: reads the delta the first kernel wrote
    hipLaunchKernelGGL((k_attn_bwd_dkv<D>), grid, block, bwd_lds_bytes<D>(t, true), st, qkv, dout, lse, delta, dqkv, N,
                       C, t, scale);
    return check_launch("tcx_attention_bwd(dkv)");
}

}  // namespace
}  // namespace tcx

using namespace tcx;

extern "C" size_t tcx_attention_bwd_workspace(int Bt, int N, int C, int heads) {
    if (Bt <= 0 || C <= 0 || heads <= 0 || C % heads || !attn_train_shape_ok(N, C / heads)) return 0;
    return (size_t)Bt * heads * N * sizeof(float);
}

extern "C" int tcx_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                 int Bt, int N, int C, int heads, void* ws, size_t ws_bytes, void* stream) {
    TCX_REQUIRE(qkv && out && dout && lse && dqkv && heads > 0 && C > 0 && C % heads == 0, "tcx_attention_bwd: bad args");
    TCX_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && aligned16(ws),
                "tcx_attention_bwd: pointers must be 16-B aligned");
    TCX_REQUIRE(Bt >= 0 && Bt <= 65535, "tcx_attention_bwd: Bt must be in [0, 65535] (one grid row per image)");
    TCX_REQUIRE(heads <= 65535, "tcx_attention_bwd: heads must be in [1, 65535] (one grid row per head)");
    const int D = C / heads;
    if (!attn_train_shape_ok(N, D)) {
        set_error("tcx_attention_bwd: N = %d, head dim %d unsupported (N %% 32 == 0 and N <= 256, or N %% 256 == 0; "
                  "head dim 8, 16, 24, 32, 48 or 64, above N = 256: 16, 32, 48, 64)", N, D);
        return TCX_EUNSUP;
    }
    if (Bt == 0) return TCX_OK;
    const size_t need = tcx_attention_bwd_workspace(Bt, N, C, heads);
    if (!ws || ws_bytes < need) {
        set_error("tcx_attention_bwd: workspace too small (%zu < %zu, tcx_attention_bwd_workspace)", ws ? ws_bytes : 0,
                  need);
        return TCX_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    float* delta = (float*)ws;
    switch (D) {
        case 8: return launch_attn_bwd<8>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        case 16: return launch_attn_bwd<16>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        case 24: return launch_attn_bwd<24>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        case 32: return launch_attn_bwd<32>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        case 48: return launch_attn_bwd<48>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        default: return launch_attn_bwd<64>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
    }
}
