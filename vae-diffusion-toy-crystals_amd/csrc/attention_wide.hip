// Self-attention of SelfAttention2d at the WIDE head dims 80, 96 and 128 (base_ch 160 / 192 / 256 with four
// heads), for any token count N >= 1: the head dims past the 64 every other attention kernel stops at.
// fp32 products on v_mfma_f32_32x32x2_f32 in the operand scheme of attention_ragged.hip:
//   S^T = K Q^T : A = K rows (keys) from LDS, B = Q^T in registers (query on the lane, d split by lane half);
//   O^T = V^T P^T: the probability accumulators ARE the B operands, key (r&3) + 8(r>>2) + 4 lh of the 32-key
//                 tile; A = V^T read from LDS in that key order.
// What the width changes:
//   registers  a query's half of d (40 / 48 / 64 floats) and DT = 3 / 3 / 4 accumulator tiles of O^T
//              (48 / 48 / 64 floats) stay in registers for the whole kernel: 128 of the 256 a lane has at two
//              waves per SIMD at d = 128.  So ONE 16-register score tile is live at a time, not two.
//   key tile   32 keys (one MFMA sub-tile), not 64: a stage is K[32][D+4] | V[32][32 DT], 33 KB at d = 128,
//              and two stages (66.5 KB) still fit twice per CU, which a 64-key tile (133 KB) would not once.
//              A tile is D/2 score MFMAs and 16 DT PV MFMAs (128 at d = 128), as many as a 64-key tile at d = 64,
//              so the global loads of tile t+1, issued to registers before them, hide as well.
//   split      grid (ceil(N/128), heads, Bt), 4 waves x 32 queries; every wave reads the same staged tile.
//   key tail   only the last tile can be ragged; it is peeled, so the main loop has no masking VALU.  Its
//              source rows are clamped to N-1 (nothing is read past the tensor) and the scores of keys >= N are
//              -inf before the row maximum: their p is exactly 0.  Key 0 of every tile is live and sits in
//              lane half 0, so after the xor-32 exchange the tile maximum is finite.
//   query tail lanes with q >= N compute on the clamped row N-1; only their stores are guarded.  No wave
//              leaves before the last barrier.
//   d = 80     the third tile of O^T is half used: V rows are zero padded to 96 columns once, never staged over.
// Online softmax: running maximum m, sum l and O^T rescaled by the same factor when a tile raises m;
// p = exp2((s - m) * scale * log2(e)) on v_exp_f32.  Fixed-order sums, no atomics but the range flag: two runs
// are bit-equal.
#include "common.hpp"
#include "h2.hpp"

namespace tcx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WQ = 128;  // queries per workgroup (4 waves x 32)
constexpr int WK = 32;   // keys per staged tile (one 32-key MFMA tile)

template <int D>
struct Wide {
    static constexpr int HD = D / 2;            // d per lane half
    static constexpr int KS = D + 4;            // K row stride ((D+4)/4 = 21 / 25 / 33, odd: conflict-free b128 row reads)
    static constexpr int DT = (D + 31) / 32;    // 32-row tiles of O^T
    static constexpr int VS = DT * 32;          // V row stride, zero padded to the tile (lane-per-column reads)
    static constexpr int D4 = D / 4;
    static constexpr int ITEMS = WK * D4;       // float4 granules of K (and of V) per tile
    static constexpr int NU = (ITEMS + 255) / 256;   // per thread
    static constexpr int STAGE = WK * (KS + VS);     // floats per LDS stage: K rows, then V rows
    static constexpr size_t LDS = 2 * (size_t)STAGE * sizeof(float);
};

// One 32-key tile against the wave's 32 queries.  TAIL: the peeled last tile with `rem` (1..32) live keys.
template <int D, bool TAIL>
__device__ __forceinline__ void wide_tile(const float* __restrict__ Ks, const float* __restrict__ Vs,
                                          const float (&qf)[D / 2], int li, int lh, int rem, float scale2, float& m,
                                          float& l, f32x16 (&oacc)[(D + 31) / 32]) {
    using G = Wide<D>;
    f32x16 sacc = (f32x16){};
    const float* kr = Ks + li * G::KS + G::HD * lh;
#pragma unroll
    for (int s4 = 0; s4 < G::HD / 4; ++s4) {
        const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + 4 * s4);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[0], qf[4 * s4 + 0], sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[1], qf[4 * s4 + 1], sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[2], qf[4 * s4 + 2], sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[3], qf[4 * s4 + 3], sacc, 0, 0, 0);
    }
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (TAIL && (r & 3) + 8 * (r >> 2) + 4 * lh >= rem) sacc[r] = -INFINITY;
        mt = fmaxf(mt, sacc[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));   // finite: key 0 of the tile is live
    const float mn = fmaxf(m, mt);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale2);   // 0 on the first tile (m = -inf)
    m = mn;
#pragma unroll
    for (int t = 0; t < G::DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
    float lt = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f((sacc[r] - mn) * scale2);   // masked key: exp2(-inf) = 0
        sacc[r] = pv;
        lt += pv;
    }
    lt += __shfl_xor(lt, 32);
    l = l * alpha + lt;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* vr = Vs + ((r & 3) + 8 * (r >> 2) + 4 * lh) * G::VS + li;
#pragma unroll
        for (int t = 0; t < G::DT; ++t)
            oacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[t * 32], sacc[r], oacc[t], 0, 0, 0);
    }
}

// 2 waves per SIMD (two workgroups per CU): 256 registers per lane
// LSE: the training forward (tcx_attention_wide_fwd_lse), which also stores the row log-sum-exp
template <int D, bool LSE = false>
__global__ __launch_bounds__(256, 2) void k_attention_wide(const float* __restrict__ qkv, void* __restrict__ out, int N,
                                                           int C, float scale2, int out_h2, unsigned* ovf,
                                                           float* __restrict__ lse, float scale) {
    using G = Wide<D>;
    extern __shared__ __attribute__((aligned(16))) float sm[];   // stage 0 | stage 1, each K[32][KS] V[32][VS]
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x;
    const size_t rs = 3 * (size_t)C;
    const float* base = qkv + (size_t)b * N * rs + h * D;
    const int lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const unsigned last = (unsigned)N - 1u;
    const unsigned q = blockIdx.x * (unsigned)WQ + w * 32 + li;   // unsigned: below N + 127 < 2^32
    float qf[G::HD];
    {
        const float* qs = base + (size_t)min(q, last) * rs + G::HD * lh;
#pragma unroll
        for (int s4 = 0; s4 < G::HD / 4; ++s4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(qs + 4 * s4);
            qf[4 * s4 + 0] = v[0]; qf[4 * s4 + 1] = v[1]; qf[4 * s4 + 2] = v[2]; qf[4 * s4 + 3] = v[3];
        }
    }
    if (G::VS > D) {   // d = 80: the V columns 80..95 of both stages: zero, never staged over
        constexpr int PADW = G::VS > D ? G::VS - D : 1;
        for (int i = tid; i < 2 * WK * PADW; i += 256) {
            const int s = i / (WK * PADW), k = i - s * (WK * PADW);
            const int j = k / PADW, e = k - j * PADW;
            sm[s * G::STAGE + WK * G::KS + j * G::VS + D + e] = 0.f;
        }
    }
    // staging: thread `tid` owns granules tid, tid + 256, ... of the tile's K and of its V, in native vectors
    f32x4 kreg[G::NU], vreg[G::NU];
    auto fetch = [&](unsigned k0) __attribute__((always_inline)) {   // rows clamped to the tensor's last
#pragma unroll
        for (int u = 0; u < G::NU; ++u) {
            const int i = tid + 256 * u;
            if (G::ITEMS % 256 == 0 || i < G::ITEMS) {
                const int j = i / G::D4, d4 = i - j * G::D4;
                const unsigned row = min(k0 + j, last);
                const float* src = base + (size_t)row * rs + d4 * 4;
                kreg[u] = *reinterpret_cast<const f32x4*>(src + C);
                vreg[u] = *reinterpret_cast<const f32x4*>(src + 2 * C);
            }
        }
    };
    auto stash = [&](float* stage) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < G::NU; ++u) {
            const int i = tid + 256 * u;
            if (G::ITEMS % 256 == 0 || i < G::ITEMS) {
                const int j = i / G::D4, d4 = i - j * G::D4;
                *reinterpret_cast<f32x4*>(stage + j * G::KS + d4 * 4) = kreg[u];
                *reinterpret_cast<f32x4*>(stage + WK * G::KS + j * G::VS + d4 * 4) = vreg[u];
            }
        }
    };
    const unsigned nt = last / WK + 1;   // key tiles; the last has rem = N - (nt-1)*32 in 1..32 live keys
    fetch(0);
    stash(sm);
    __syncthreads();
    f32x16 oacc[G::DT];
#pragma unroll
    for (int t = 0; t < G::DT; ++t) oacc[t] = (f32x16){};
    float m = -INFINITY, l = 0.f;
    for (unsigned t = 0; t + 1 < nt; ++t) {
        float* cur = sm + (t & 1) * G::STAGE;
        float* nxt = sm + ((t & 1) ^ 1) * G::STAGE;
        fetch((t + 1) * WK);   // clamps in the last tile only
        __builtin_amdgcn_sched_barrier(0);   // keep every load ahead of the tile's MFMAs
        wide_tile<D, false>(cur, cur + WK * G::KS, qf, li, lh, WK, scale2, m, l, oacc);
        stash(nxt);
        __syncthreads();   // nxt complete for the next iteration; cur free to be rewritten in it
    }
    {
        const float* cur = sm + ((nt - 1) & 1) * G::STAGE;
        wide_tile<D, true>(cur, cur + WK * G::KS, qf, li, lh, (int)(N - (nt - 1) * WK), scale2, m, l, oacc);
    }
    if (q >= (unsigned)N) return;   // after the last barrier
    const float inv = 1.f / l;
    if (LSE && lh == 0) lse[((size_t)b * gridDim.y + h) * N + q] = m * scale + logf(l);
    if (out_h2) {   // h2 record of the query's pixel (h2.hpp): 4 consecutive d per register quad
        bool bad = false;
#pragma unroll
        for (int t = 0; t < G::DT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = t * 32 + 8 * i + 4 * lh;
                if (t * 32 + 8 * i < D) {   // D % 8 == 0: both lane halves' quads are inside
                    const float4 v = make_float4(oacc[t][4 * i] * inv, oacc[t][4 * i + 1] * inv, oacc[t][4 * i + 2] * inv,
                                                 oacc[t][4 * i + 3] * inv);
                    store4_h2(reinterpret_cast<char*>(out), ((size_t)b * N + q) * C * 4, (h * D + d) >> 2, v);
                    bad = bad || h2_bad(v.x) || h2_bad(v.y) || h2_bad(v.z) || h2_bad(v.w);
                }
            }
        h2_flag(ovf, bad);
        return;
    }
    float* dst = reinterpret_cast<float*>(out) + ((size_t)b * N + q) * C + h * D;
#pragma unroll
    for (int t = 0; t < G::DT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t * 32 + 8 * i < D)
                *reinterpret_cast<float4*>(dst + t * 32 + 8 * i + 4 * lh) =
                    make_float4(oacc[t][4 * i] * inv, oacc[t][4 * i + 1] * inv, oacc[t][4 * i + 2] * inv,
                                oacc[t][4 * i + 3] * inv);
}

template <int D, bool LSE = false>
int launch_attn_wide(const float* qkv, void* out, int out_h2, int Bt, int N, int C, int heads, unsigned* ovf,
                     hipStream_t st, float* lse = nullptr) {
    const char* name = LSE ? "tcx_attention_wide_fwd_lse" : "tcx_attention_wide";
    // log2(e) / sqrt(D): the logits in exp2 units
    const float scale2 = (float)(1.4426950408889634 / std::sqrt((double)D));
    const float scale = (float)(1.0 / std::sqrt((double)D));
    static bool attr_set = false;   // 66.5 KB at D = 128: above 64 KB dynamic LDS needs the explicit opt-in
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_wide<D, LSE>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)Wide<D>::LDS) != hipSuccess) {
            set_error("%s: cannot enable %zu B of dynamic LDS", name, Wide<D>::LDS);
            return TCX_EHIP;
        }
        attr_set = true;
    }
    hipLaunchKernelGGL((k_attention_wide<D, LSE>), dim3((N - 1) / WQ + 1, heads, Bt), dim3(256), Wide<D>::LDS, st, qkv,
                       out, N, C, scale2, out_h2, ovf, lse, scale);
    return check_launch(name);
}

}  // namespace
}  // namespace tcx

using namespace tcx;

extern "C" int tcx_attention_wide(const float* qkv, void* out, int out_h2, int Bt, int N, int C, int heads,
                                  unsigned* ovf, void* stream) {
    TCX_REQUIRE(qkv && out, "tcx_attention_wide: null pointer");
    TCX_REQUIRE(heads > 0 && C > 0 && C % heads == 0, "tcx_attention_wide: bad args (need heads > 0, C %% heads == 0)");
    TCX_REQUIRE(N > 0, "tcx_attention_wide: N must be >= 1");
    TCX_REQUIRE(out_h2 == 0 || out_h2 == 1, "tcx_attention_wide: out_h2 must be 0 (fp32) or 1 (h2 records)");
    TCX_REQUIRE(aligned16(qkv) && aligned16(out), "tcx_attention_wide: pointers must be 16-B aligned");
    TCX_REQUIRE(Bt >= 0 && Bt <= 65535, "tcx_attention_wide: Bt must be in [0, 65535] (one grid row per image)");
    TCX_REQUIRE(heads <= 65535, "tcx_attention_wide: heads must be in [1, 65535] (one grid row per head)");
    const int D = C / heads;
    if (!(D == 80 || D == 96 || D == 128)) {
        set_error("tcx_attention_wide: head dim %d unsupported (80, 96 or 128)", D);
        return TCX_EUNSUP;
    }
    if (Bt == 0) return TCX_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 80: return launch_attn_wide<80>(qkv, out, out_h2, Bt, N, C, heads, ovf, st);
        case 96: return launch_attn_wide<96>(qkv, out, out_h2, Bt, N, C, heads, ovf, st);
        default: return launch_attn_wide<128>(qkv, out, out_h2, Bt, N, C, heads, ovf, st);
    }
}

// The training forward: k_attention_wide<D, true>, fp32 out bit-equal to tcx_attention_wide(out_h2 = 0) plus
// lse[b][h][q] = m * scale + ln l for tcx_attention_wide_bwd.
extern "C" int tcx_attention_wide_fwd_lse(const float* qkv, float* out, float* lse, int Bt, int N, int C, int heads,
                                          void* stream) {
    TCX_REQUIRE(qkv && out && lse, "tcx_attention_wide_fwd_lse: null pointer");
    TCX_REQUIRE(heads > 0 && C > 0 && C % heads == 0,
                "tcx_attention_wide_fwd_lse: bad args (need heads > 0, C %% heads == 0)");
    TCX_REQUIRE(N > 0, "tcx_attention_wide_fwd_lse: N must be >= 1");
    TCX_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(lse),
                "tcx_attention_wide_fwd_lse: pointers must be 16-B aligned");
    TCX_REQUIRE(Bt >= 0 && Bt <= 65535, "tcx_attention_wide_fwd_lse: Bt must be in [0, 65535] (one grid row per image)");
    TCX_REQUIRE(heads <= 65535, "tcx_attention_wide_fwd_lse: heads must be in [1, 65535] (one grid row per head)");
    const int D = C / heads;
    if (!(D == 80 || D == 96 || D == 128)) {
        set_error("tcx_attention_wide_fwd_lse: head dim %d unsupported (80, 96 or 128)", D);
        return TCX_EUNSUP;
    }
    if (Bt == 0) return TCX_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 80: return launch_attn_wide<80, true>(qkv, out, 0, Bt, N, C, heads, nullptr, st, lse);
        case 96: return launch_attn_wide<96, true>(qkv, out, 0, Bt, N, C, heads, nullptr, st, lse);
        default: return launch_attn_wide<128, true>(qkv, out, 0, Bt, N, C, heads, nullptr, st, lse);
    }
}
