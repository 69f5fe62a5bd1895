// Backward of the training attention at the WIDE head dims 80, 96 and 128, any token count N >= 1.  From qkv,
// out, dout and the row log-sum-exp of tcx_attention_wide_fwd_lse two kernels recompute
// P = exp(scale s - lse) per 32 x 32 tile and write dqkv [Bt,N,3C]; no N x N tensor exists.  fp32 on
// v_mfma_f32_32x32x2_f32, fixed-order sums, no atomics: two runs are bit-equal.
//
//   dP = dO V^T,  dS = P o (dP - delta),  delta[i] = sum_d dO[i][d] O[i][d]
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO
//
// Operand scheme of attention_ragged_bwd.hip: the row a lane owns (a query in k_attn_wbwd_dq, a key in
// k_attn_wbwd_dkv) has its d-vectors in registers as the B operands of the score products, and the 32 x 32
// accumulator tile of dS / P (row (r&3) + 8(r>>2) + 4 lh in register r, the lane's row as the column) is at
// once the B operand of the gradient products, whose A operand is read down LDS columns in that order.
// What the width changes:
//   registers  per lane the owned row's two half d-vectors (2 x 40 / 48 / 64 floats) and the gradient^T
//              accumulators (dq: DT = 3 / 3 / 4 tiles of 16; dkv: twice that) stay resident: 192 (dq) and 256
//              (dkv) floats at d = 128 before the two live 16-register score tiles and the staging registers.
//              The instantiations past 256 registers run ONE wave per SIMD with the unified 512-register file
//              (accumulators in AGPRs) instead of spilling: OCC_DQ / OCC_DKV below, set from the compiler's
//              resource report (zero scratch everywhere).
//   streamed tile  32 rows, one MFMA sub-tile (the narrow siblings stream 64): a stage X[32][D+4] | Y[32][D+4]
//              is 33.8 KB at d = 128, two stages 67.6 KB.  A tile is D score MFMAs and 16 DT (dq) or 32 DT (dkv)
//              gradient MFMAs, 192 / 256 at d = 128, which hide the next tile's global loads (issued to
//              registers before them, stored to the other stage after them; one barrier per tile).
//   split      grid (ceil(N/128), heads, Bt), 4 waves x 32 owned rows.
//   streamed tail  only the last tile can be ragged; it is peeled.  Its source rows (lse and delta too) are
//              clamped to N-1: nothing is read past a tensor and every staged value is finite.  A streamed
//              key >= N gets dS = 0 in dq, a streamed query >= N gets P = 0 and dS = 0 in dkv: selects to an
//              exact 0.
//   owned tail  lanes whose own row is >= N compute on the clamped row N-1 with its lse; only their stores
//              (dq rows, delta, dk and dv rows) are guarded.  No wave leaves before the last barrier.
//   columns  at d = 80 the gradient products read A down columns li + 64 up to 95, fewer than 12 floats past a
//              slice's last row.  dq reads only X (= K) by column, and Y follows it; dkv reads X and Y, and the
//              64 floats of lse / delta follow Y in BOTH stages, so every such read is inside the allocation
//              and of staged (finite) data.  The accumulator rows they feed are never stored.
#include "common.hpp"

namespace tcx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WO = 128;  // owned rows per workgroup (4 waves x 32)
constexpr int WT = 32;   // streamed rows per staged tile (one 32-row MFMA tile)

template <int D>
struct WBwd {
    static constexpr int HD = D / 2;          // d per lane half
    static constexpr int KS = D + 4;          // LDS row stride ((D+4)/4 odd: conflict-free b128 row reads)
    static constexpr int DT = (D + 31) / 32;  // 32-row tiles of a gradient^T
    static constexpr int D4 = D / 4;
    static constexpr int ITEMS = WT * D4;            // float4 granules of X (and of Y) per tile
    static constexpr int NU = (ITEMS + 255) / 256;   // per thread
    static constexpr int SLICE = WT * KS;
    static constexpr int STAGE_DQ = 2 * SLICE;            // K | V
    static constexpr int STAGE_DKV = 2 * SLICE + 2 * WT;  // Q | dO | lse | delta
    static constexpr size_t LDS_DQ = 2 * (size_t)STAGE_DQ * sizeof(float);
    static constexpr size_t LDS_DKV = 2 * (size_t)STAGE_DKV * sizeof(float);
    // workgroups per CU = waves per SIMD: 2 leaves 256 registers per lane, 1 leaves 512 (VGPR + AGPR).
    // dq fits 256 up to d = 96 (236 / 250); dkv does not even at d = 80 (248 B of scratch at 2)
    static constexpr int OCC_DQ = D > 96 ? 1 : 2;
    static constexpr int OCC_DKV = 1;
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Thread `tid` owns granules tid, tid + 256, ... of the tile's X and of its Y.  Rows r0 .. r0 + 31 of x / y (row
// strides xs / ys floats), each clamped to `lim`, into native vector registers.
template <int D>
__device__ __forceinline__ void fetch_pair(f32x4 (&xr)[WBwd<D>::NU], f32x4 (&yr)[WBwd<D>::NU],
                                           const float* __restrict__ x, size_t xs, const float* __restrict__ y,
                                           size_t ys, unsigned r0, unsigned lim, int tid) {
    using G = WBwd<D>;
#pragma unroll
    for (int u = 0; u < G::NU; ++u) {
        const int i = tid + 256 * u;
        if (G::ITEMS % 256 == 0 || i < G::ITEMS) {
            const int j = i / G::D4, d4 = i - j * G::D4;
            const size_t row = min(r0 + j, lim);
            xr[u] = *reinterpret_cast<const f32x4*>(x + row * xs + d4 * 4);
            yr[u] = *reinterpret_cast<const f32x4*>(y + row * ys + d4 * 4);
        }
    }
}

template <int D>
__device__ __forceinline__ void stash_pair(float* __restrict__ stage, const f32x4 (&xr)[WBwd<D>::NU],
                                           const f32x4 (&yr)[WBwd<D>::NU], int tid) {
    using G = WBwd<D>;
#pragma unroll
    for (int u = 0; u < G::NU; ++u) {
        const int i = tid + 256 * u;
        if (G::ITEMS % 256 == 0 || i < G::ITEMS) {
            const int j = i / G::D4, d4 = i - j * G::D4;
            *reinterpret_cast<f32x4*>(stage + j * G::KS + d4 * 4) = xr[u];
            *reinterpret_cast<f32x4*>(stage + G::SLICE + j * G::KS + d4 * 4) = yr[u];
        }
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
            if (t * 32 + 8 * i < D) {  // D % 8 == 0: both lane halves' quads are inside
                f32x4 v = {acc[t][4 * i] * alpha, acc[t][4 * i + 1] * alpha, acc[t][4 * i + 2] * alpha,
                           acc[t][4 * i + 3] * alpha};
                *reinterpret_cast<f32x4*>(dst + t * 32 + 8 * i + 4 * lh) = v;
            }
}

// S^T and dP^T of the 32-row tile: A = the rows of X / Y at `xr` / `yr` (this lane's row, its half of d),
// B = the owned row's two d-vectors
template <int D>
__device__ __forceinline__ void score_pair(const float* __restrict__ xr, const float* __restrict__ yr,
                                           const float (&xf)[D / 2], const float (&yf)[D / 2], f32x16& s, f32x16& dp) {
#pragma unroll
    for (int s4 = 0; s4 < D / 8; ++s4) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + 4 * s4);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(yr + 4 * s4);
        s = mfma(xv[0], xf[4 * s4 + 0], s);
        dp = mfma(yv[0], yf[4 * s4 + 0], dp);
        s = mfma(xv[1], xf[4 * s4 + 1], s);
        dp = mfma(yv[1], yf[4 * s4 + 1], dp);
        s = mfma(xv[2], xf[4 * s4 + 2], s);
        dp = mfma(yv[2], yf[4 * s4 + 2], dp);
        s = mfma(xv[3], xf[4 * s4 + 3], s);
        dp = mfma(yv[3], yf[4 * s4 + 3], dp);
    }
}

// ---------------------------------------------------------------------------------------------
// dQ: the query on the lane.  One 32-key tile (K rows at Ks, V rows at Vs) against the wave's 32 queries:
//   S^T = K Q^T,  dP^T = V dO^T,  dS^T = exp(scale S^T - lse[q]) (dP^T - delta[q]),  dQ^T += K^T dS^T
// TAIL: the peeled last tile with `rem` (1..32) live keys.
// ---------------------------------------------------------------------------------------------
template <int D, bool TAIL>
__device__ __forceinline__ void dq_tile(const float* __restrict__ Ks, const float* __restrict__ Vs,
                                        const float (&qf)[D / 2], const float (&dof)[D / 2], int li, int lh, int rem,
                                        float scale, float ls, float dl, f32x16 (&dq)[(D + 31) / 32]) {
    using G = WBwd<D>;
    f32x16 s = (f32x16){}, dp = (f32x16){};
    score_pair<D>(Ks + li * G::KS + G::HD * lh, Vs + li * G::KS + G::HD * lh, qf, dof, s, dp);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float ds = expf(fmaf(s[r], scale, -ls)) * (dp[r] - dl);
        s[r] = TAIL && (r & 3) + 8 * (r >> 2) + 4 * lh >= rem ? 0.f : ds;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* kc = Ks + ((r & 3) + 8 * (r >> 2) + 4 * lh) * G::KS + li;
#pragma unroll
        for (int t = 0; t < G::DT; ++t) dq[t] = mfma(kc[t * 32], s[r], dq[t]);  // rows d >= D: never stored
    }
}

template <int D>
__global__ __launch_bounds__(256, WBwd<D>::OCC_DQ) void k_attn_wbwd_dq(
    const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ dout,
    const float* __restrict__ lse, float* __restrict__ dqkv, float* __restrict__ delta, int N, int C, float scale) {
    using G = WBwd<D>;
    extern __shared__ __attribute__((aligned(16))) float sm[];  // stage 0 | stage 1, each K[32][KS] V[32][KS]
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const unsigned last = (unsigned)N - 1u;
    const unsigned q = blockIdx.x * (unsigned)WO + w * 32 + li;  // unsigned: below N + 127 < 2^32
    const size_t qc = min(q, last);
    const size_t rs = 3 * (size_t)C;
    const float* base = qkv + (size_t)b * N * rs + h * D;
    const size_t hrow = ((size_t)b * gridDim.y + h) * N;
    float qf[G::HD], dof[G::HD];
    float dl = 0.f;
    {   // prologue: the owned query's q and dO halves, and delta = sum_d dO O for both kernels
        const float* qs = base + qc * rs + G::HD * lh;
        const size_t o = ((size_t)b * N + qc) * C + h * D + G::HD * lh;
#pragma unroll
        for (int s4 = 0; s4 < G::HD / 4; ++s4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(qs + 4 * s4);
            const f32x4 g = *reinterpret_cast<const f32x4*>(dout + o + 4 * s4);
            const f32x4 y = *reinterpret_cast<const f32x4*>(out + o + 4 * s4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                qf[4 * s4 + e] = v[e];
                dof[4 * s4 + e] = g[e];
                dl = fmaf(g[e], y[e], dl);
            }
        }
    }
    dl += __shfl_xor(dl, 32);
    if (lh == 0 && q < (unsigned)N) delta[hrow + q] = dl;
    const float ls = lse[hrow + qc];
    f32x4 kreg[G::NU], vreg[G::NU];
    const unsigned nt = last / WT + 1;  // key tiles; the last has rem = N - (nt-1)*32 in 1..32 live keys
    fetch_pair<D>(kreg, vreg, base + C, rs, base + 2 * C, rs, 0, last, tid);
    stash_pair<D>(sm, kreg, vreg, tid);
    __syncthreads();
    f32x16 dq[G::DT];
#pragma unroll
    for (int t = 0; t < G::DT; ++t) dq[t] = (f32x16){};
    for (unsigned t = 0; t + 1 < nt; ++t) {
        float* cur = sm + (t & 1) * G::STAGE_DQ;
        float* nxt = sm + ((t & 1) ^ 1) * G::STAGE_DQ;
        fetch_pair<D>(kreg, vreg, base + C, rs, base + 2 * C, rs, (t + 1) * WT, last, tid);  // clamps in the last tile only
        __builtin_amdgcn_sched_barrier(0);  // keep every load ahead of the tile's MFMAs
        dq_tile<D, false>(cur, cur + G::SLICE, qf, dof, li, lh, WT, scale, ls, dl, dq);
        stash_pair<D>(nxt, kreg, vreg, tid);
        __syncthreads();  // nxt complete for the next iteration; cur free to be rewritten in it
    }
    {
        const float* cur = sm + ((nt - 1) & 1) * G::STAGE_DQ;
        dq_tile<D, true>(cur, cur + G::SLICE, qf, dof, li, lh, (int)(N - (nt - 1) * WT), scale, ls, dl, dq);
    }
    if (q < (unsigned)N) store_rows<D>(dqkv + ((size_t)b * N + q) * rs + h * D, dq, scale, lh);
}

// ---------------------------------------------------------------------------------------------
// dK, dV: the key on the lane.  One 32-query tile (Q rows at Qs, dO rows at Gs, lse and delta of those
// queries at Ls / Ds) against the wave's 32 keys:
//   S = Q K^T,  dP = dO V^T;  accumulator rows are queries, so lse / delta come per register quad from LDS
//   P = exp(scale S - lse),  dS = P (dP - delta),  dV^T += dO^T P,  dK^T += Q^T dS
// TAIL: the peeled last tile with `rem` (1..32) live queries.
// ---------------------------------------------------------------------------------------------
template <int D, bool TAIL>
__device__ __forceinline__ void dkv_tile(const float* __restrict__ Qs, const float* __restrict__ Gs,
                                         const float* __restrict__ Ls, const float* __restrict__ Ds,
                                         const float (&kf)[D / 2], const float (&vf)[D / 2], int li, int lh, int rem,
                                         float scale, f32x16 (&dk)[(D + 31) / 32], f32x16 (&dv)[(D + 31) / 32]) {
    using G = WBwd<D>;
    f32x16 s = (f32x16){}, dp = (f32x16){};
    score_pair<D>(Qs + li * G::KS + G::HD * lh, Gs + li * G::KS + G::HD * lh, kf, vf, s, dp);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // registers 4i .. 4i+3: queries 8i + 4lh + 0..3
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + 8 * i + 4 * lh);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(Ds + 8 * i + 4 * lh);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float p = expf(fmaf(s[4 * i + j], scale, -l4[j]));
            const float ds = p * (dp[4 * i + j] - d4[j]);
            const bool dead = TAIL && 8 * i + 4 * lh + j >= rem;
            s[4 * i + j] = dead ? 0.f : p;
            dp[4 * i + j] = dead ? 0.f : ds;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qrow = ((r & 3) + 8 * (r >> 2) + 4 * lh) * G::KS + li;
#pragma unroll
        for (int t = 0; t < G::DT; ++t) {  // rows d >= D: never stored
            dv[t] = mfma(Gs[qrow + t * 32], s[r], dv[t]);
            dk[t] = mfma(Qs[qrow + t * 32], dp[r], dk[t]);
        }
    }
}

template <int D>
__global__ __launch_bounds__(256, WBwd<D>::OCC_DKV) void k_attn_wbwd_dkv(
    const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dqkv, int N, int C, float scale) {
    using G = WBwd<D>;
    // stage 0 | stage 1, each Q[32][KS] dO[32][KS] lse[32] delta[32]
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const unsigned last = (unsigned)N - 1u;
    const unsigned key = blockIdx.x * (unsigned)WO + w * 32 + li;
    const size_t rs = 3 * (size_t)C;
    const float* base = qkv + (size_t)b * N * rs + h * D;
    const float* gbase = dout + (size_t)b * N * C + h * D;
    const size_t hrow = ((size_t)b * gridDim.y + h) * N;
    float kf[G::HD], vf[G::HD];
    {
        const float* ks = base + (size_t)min(key, last) * rs + C + G::HD * lh;
#pragma unroll
        for (int s4 = 0; s4 < G::HD / 4; ++s4) {
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(ks + 4 * s4);
            const f32x4 v4 = *reinterpret_cast<const f32x4*>(ks + C + 4 * s4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kf[4 * s4 + e] = k4[e];
                vf[4 * s4 + e] = v4[e];
            }
        }
    }
    // threads 0..31 carry lse, 32..63 delta of the tile's queries
    const float* lsrc = (tid < WT ? lse : delta) + hrow;
    const int lslot = 2 * G::SLICE + tid;  // Ls[tid] or Ds[tid - 32]: contiguous
    f32x4 qreg[G::NU], greg[G::NU];
    float lreg = 0.f;
    const unsigned nt = last / WT + 1;  // query tiles; the last has rem = N - (nt-1)*32 in 1..32 live queries
    fetch_pair<D>(qreg, greg, base, rs, gbase, (size_t)C, 0, last, tid);
    if (tid < 2 * WT) lreg = lsrc[min((unsigned)(tid & (WT - 1)), last)];
    stash_pair<D>(sm, qreg, greg, tid);
    if (tid < 2 * WT) sm[lslot] = lreg;
    __syncthreads();
    f32x16 dv[G::DT], dk[G::DT];
#pragma unroll
    for (int t = 0; t < G::DT; ++t) dv[t] = dk[t] = (f32x16){};
    for (unsigned t = 0; t + 1 < nt; ++t) {
        float* cur = sm + (t & 1) * G::STAGE_DKV;
        float* nxt = sm + ((t & 1) ^ 1) * G::STAGE_DKV;
        fetch_pair<D>(qreg, greg, base, rs, gbase, (size_t)C, (t + 1) * WT, last, tid);  // clamps in the last tile only
        if (tid < 2 * WT) lreg = lsrc[min((t + 1) * WT + (tid & (WT - 1)), last)];
        __builtin_amdgcn_sched_barrier(0);  // keep every load ahead of the tile's MFMAs
        dkv_tile<D, false>(cur, cur + G::SLICE, cur + 2 * G::SLICE, cur + 2 * G::SLICE + WT, kf, vf, li, lh, WT, scale, dk,
                           dv);
        stash_pair<D>(nxt, qreg, greg, tid);
        if (tid < 2 * WT) nxt[lslot] = lreg;
        __syncthreads();  // nxt complete for the next iteration; cur free to be rewritten in it
    }
    {
        const float* cur = sm + ((nt - 1) & 1) * G::STAGE_DKV;
        dkv_tile<D, true>(cur, cur + G::SLICE, cur + 2 * G::SLICE, cur + 2 * G::SLICE + WT, kf, vf, li, lh,
                          (int)(N - (nt - 1) * WT), scale, dk, dv);
    }
    if (key >= (unsigned)N) return;  // after the last barrier
    float* dst = dqkv + ((size_t)b * N + key) * rs + h * D;
    store_rows<D>(dst + C, dk, scale, lh);
    store_rows<D>(dst + 2 * C, dv, 1.f, lh);
}

template <int D>
int launch_attn_wbwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta,
                     int Bt, int N, int C, int heads, hipStream_t st) {
    using G = WBwd<D>;
    const float scale = (float)(1.0 / std::sqrt((double)D));
    static bool attr_set = false;  // 67.6 KB at D = 128: above 64 KB dynamic LDS needs the explicit opt-in
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_wbwd_dq<D>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_DQ) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_wbwd_dkv<D>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_DKV) != hipSuccess) {
            set_error("tcx_attention_wide_bwd: cannot enable %zu B of dynamic LDS", G::LDS_DKV);
            return TCX_EHIP;
        }
        attr_set = true;
    }
    const dim3 grid((N - 1) / WO + 1, heads, Bt), block(256);
    hipLaunchKernelGGL((k_attn_wbwd_dq<D>), grid, block, G::LDS_DQ, st, qkv, out, dout, lse, dqkv, delta, N, C, scale);
    TCX_TRY(check_launch("tcx_attention_wide_bwd(dq)"));
    // same stream: reads the delta the first kernel wrote
    hipLaunchKernelGGL((k_attn_wbwd_dkv<D>), grid, block, G::LDS_DKV, st, qkv, dout, lse, delta, dqkv, N, C, scale);
    return check_launch("tcx_attention_wide_bwd(dkv)");
}

inline bool wbwd_dim_ok(int D) { return D == 80 || D == 96 || D == 128; }

}  // namespace
}  // namespace tcx

using namespace tcx;

extern "C" size_t tcx_attention_wide_bwd_workspace(int Bt, int N, int C, int heads) {
    if (Bt <= 0 || Bt > 65535 || N <= 0 || C <= 0 || heads <= 0 || heads > 65535 || C % heads || !wbwd_dim_ok(C / heads))
        return 0;
    return (size_t)Bt * heads * N * sizeof(float);
}

extern "C" int tcx_attention_wide_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                                      float* dqkv, int Bt, int N, int C, int heads, void* ws, size_t ws_bytes,
                                      void* stream) {
    TCX_REQUIRE(qkv && out && dout && lse && dqkv && heads > 0 && C > 0 && C % heads == 0,
                "tcx_attention_wide_bwd: bad args");
    TCX_REQUIRE(N > 0, "tcx_attention_wide_bwd: N must be >= 1");
    TCX_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(lse) && aligned16(dqkv) && aligned16(ws),
                "tcx_attention_wide_bwd: pointers must be 16-B aligned");
    TCX_REQUIRE(Bt >= 0 && Bt <= 65535, "tcx_attention_wide_bwd: Bt must be in [0, 65535] (one grid row per image)");
    TCX_REQUIRE(heads <= 65535, "tcx_attention_wide_bwd: heads must be in [1, 65535] (one grid row per head)");
    const int D = C / heads;
    if (!wbwd_dim_ok(D)) {
        set_error("tcx_attention_wide_bwd: head dim %d unsupported (80, 96 or 128)", D);
        return TCX_EUNSUP;
    }
    if (Bt == 0) return TCX_OK;
    const size_t need = tcx_attention_wide_bwd_workspace(Bt, N, C, heads);
    if (!ws || ws_bytes < need) {
        set_error("tcx_attention_wide_bwd: workspace too small (%zu < %zu, tcx_attention_wide_bwd_workspace)",
                  ws ? ws_bytes : 0, need);
        return TCX_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    float* delta = (float*)ws;
    switch (D) {
        case 80: return launch_attn_wbwd<80>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        case 96: return launch_attn_wbwd<96>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
        default: return launch_attn_wbwd<128>(qkv, out, dout, lse, dqkv, delta, Bt, N, C, heads, st);
    }
}
