// k_attn_block: the qkv 1x1 conv of SelfAttention2d computed inside the attention workgroup
// (reference src/toycrystals/models/sde_score_model.py:136-167: qkv = Conv2d(C, 3C, 1), softmax(q k^T /
// sqrt(d)) v per (batch, head)) for the split-precision evaluator's bottleneck: N = 256 tokens, C = 192,
// 4 heads of d = 48, f16x3 (h2.hpp).  It replaces the k_lin1x1 qkv launch and k_attention_split<48, 0>:
// the qkv tensor (N x 3C h2, 151 MB per evaluation at Bt = 256) is never written to or read from memory.
//
// One 512-thread workgroup per (image, head), as k_attention_split.  Phase 1 is k_lin1x1's GEMM
// restricted to the head's 144 weight rows (q, k, v: 48 each): K = 192 streamed in six 32-channel chunks
// by LDS-DMA, double-buffered, both tiles row-major with 128-B rows and the same XOR swizzle; wave w
// owns tokens 32 w .. 32 w + 31.  The products and their order per output element are k_lin1x1's
// (x_hi w_lo + x_lo w_hi + x_hi w_hi per 16-deep step, chunks in order), so q, k, v are bit-identical
// to the three-launch path.  The operand roles are chosen so that the accumulators already have the
// layouts the attention loop wants:
//   q, k : A = weight rows, B = the wave's token rows -> the token sits on the lane, 16 head dims in the
//          registers.  The weight row of MFMA row m is sigma(m) (m with bits 2 and 3 swapped), so that
//          registers 8 s + e of lane half h are dims 16 s + 8 h + e: for q that IS the B fragment of
//          S^T = K Q^T (no bounce through LDS), for k one 16-B hi and one 16-B lo piece of the token's
//          staged K row.  Tiles: q dims 0..31 | k dims 0..31 | q dims 32..47 with k dims 32..47.
//   v    : A = the wave's token rows, B = weight rows -> the head dim sits on the lane and registers
//          8 s + e of half h are keys 16 s + 8 (e >> 2) + 4 h + (e & 3), which is k_attention_split's slot
//          order 16 s + 8 h + e of V^T: one 16-B hi and one 16-B lo write per step.  Two tiles (dims 0..31,
//          32..47; lanes 16..31 of the second repeat dims 32..47 into the padding rows 48..63 of V^T,
//          whose O^T rows are never stored).
// After scale + bias the values are split with split1's arithmetic and range-tested (h2_flag on ovf for
// |v| >= kH2Max, as the qkv conv's epilogue did).  Phase 2 is k_attention_split<48, 0>'s loop body on the
// two 128-key tiles, which are both resident (N = 256): no loads, one barrier.
#include "conv_common.hpp"
#include "passes.hpp"

namespace tcx {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int B_N = 256;                    // tokens per image
constexpr int B_C = 192;                    // channels
constexpr int B_D = 48;                     // head dim
constexpr int B_ROWB = B_C * 4;             // bytes per h2 token / weight row
constexpr int B_NCH = B_C / 32;             // 32-channel chunks of K
constexpr int B_ABYTES = B_N * 128;         // activation chunk: 256 tokens x 32 channels h2
constexpr int B_WROWS = 3 * B_D;            // the head's q, k, v weight rows
constexpr int B_WBYTES = B_WROWS * 128;     // weight chunk
constexpr int B_GSTAGE = B_ABYTES + B_WBYTES;
// k_attention_split<48, 0>'s stage: 128 K rows, V^T hi, V^T lo
constexpr int B_KT = 128;
constexpr int B_KSB = B_D * 4 + 16;
constexpr int B_VSW = B_KT / 2 + 4;
constexpr int B_DP = 64;
constexpr int B_ASTAGE = B_KT * B_KSB + 2 * B_DP * B_VSW * 4;
constexpr int B_LDS = 2 * (B_ASTAGE > B_GSTAGE ? B_ASTAGE : B_GSTAGE);
constexpr int B_WAIT_VM7 = 0x0F77;  // s_waitcnt vmcnt(7): one stage (4 + 3 DMA per wave) in flight
constexpr int B_WAIT_VM0 = 0x0F70;

__device__ __forceinline__ void b_dma16(__amdgpu_buffer_rsrc_t r, char* lds, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}

__device__ __forceinline__ int sigma23(int m) { return (m & ~12) | ((m & 4) << 1) | ((m & 8) >> 1); }

// scale + bias, range test, split (split1's arithmetic) of 8 accumulators -> hi / lo fragments
__device__ __forceinline__ void b_split8(const f32x16& acc, int r0, float wsc, const f4 b0, const f4 b1, h8& hi, h8& lo,
                                         bool& bad) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = fmaf(acc[r0 + e], wsc, e < 4 ? b0[e & 3] : b1[e & 3]);
        // the fp32 value, as the conv epilogue has it before split1: without this the compiler folds the fma
        // into the f16 convert (v_fma_mix: one rounding instead of two), which differs on f16 ties
        asm volatile("" : "+v"(v));
        bad = bad || h2_bad(v);
        const _Float16 hh = (_Float16)v;
        hi[e] = hh;
        lo[e] = (_Float16)(v - (float)hh);
    }
}

__global__ __launch_bounds__(512) void k_attn_block(const char* __restrict__ x, const float* __restrict__ wq,
                                                    unsigned bytesw, const float* __restrict__ wscale,
                                                    const float* __restrict__ bias, char* __restrict__ out,
                                                    unsigned* __restrict__ ovf, float scale, int xcd) {
    constexpr int D = B_D, C = B_C, N = B_N, KSB = B_KSB, VSW = B_VSW, DP = B_DP, KT = B_KT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int lz;  // LDS-DMA destinations from a base the optimiser cannot fold to a constant (conv3l.hip)
    asm volatile("s_mov_b32 %0, 0" : "=s"(lz));
    char* const smd = smem + lz;

    int b = blockIdx.z, h = blockIdx.y;
    if (xcd) {  // the heads of an image on one XCD: they stream the same token rows (attention_split.hip)
        const int nh = gridDim.y;
        const int t = xcd_remap(blockIdx.y + nh * blockIdx.z, nh * gridDim.z);
        h = t % nh;
        b = t / nh;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const __amdgpu_buffer_rsrc_t ra =
        mk_rsrc(reinterpret_cast<const float*>(x + (size_t)b * N * B_ROWB), (unsigned)(N * B_ROWB));
    const __amdgpu_buffer_rsrc_t rw = mk_rsrc(wq, bytesw);

    // ---- phase 1: q, k, v of this head
    // DMA plan per chunk: activation instructions 4 w .. 4 w + 3 (8 token rows each), weight instructions
    // w, w + 8 and 16 + (w & 1) of 18 (the third is issued by four waves each with the same bytes, so
    // every wave has 7 loads per stage and one vmcnt serves all)
    const int lr = lane >> 3, lp = lane & 7;
    int aoff[4], boff[3], bdst[3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 8 * (4 * w + q) + lr;
        aoff[q] = r * B_ROWB + 16 * (lp ^ ((r >> 1) & 7));
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int ins = q == 0 ? w : q == 1 ? w + 8 : 16 + (w & 1);
        const int r = 8 * ins + lr;                       // row of the head's 144
        const int g = (r / D) * C + h * D + (r % D);      // row of the packed qkv weight
        boff[q] = g * B_ROWB + 16 * (lp ^ ((r >> 1) & 7));
        bdst[q] = B_ABYTES + ins * 1024;
    }
    auto issue = [&](int c, int buf) {
        char* const d = smd + buf * B_GSTAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q) b_dma16(ra, d + (4 * w + q) * 1024, aoff[q], c * 128);
#pragma unroll
        for (int q = 0; q < 3; ++q) b_dma16(rw, d + bdst[q], boff[q], c * 128);
    };
    auto rd = [&](int buf, int base, int r, int piece) {
        return __builtin_bit_cast(h8, *reinterpret_cast<const float4*>(smem + buf * B_GSTAGE + base + r * 128 +
                                                                         16 * (piece ^ ((r >> 1) & 7))));
    };
    // weight row (of the 144) this lane reads for tile t
    const int sg = sigma23(li);
    int wrow[5];
    wrow[0] = sg;                             // q dims 0..31
    wrow[1] = D + sg;                         // k dims 0..31
    wrow[2] = sg < 16 ? 32 + sg : D + 16 + sg;  // q dims 32..47 | k dims 32..47
    wrow[3] = 2 * D + li;                     // v dims 0..31
    wrow[4] = 2 * D + 32 + (li & 15);         // v dims 32..47 (twice)
    const int xrow = 32 * w + li;

    f32x16 acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) acc[t] = (f32x16){};

    issue(0, 0);
    issue(1, 1);
    for (int c = 0; c < B_NCH; ++c) {
        const int buf = c & 1;
        if (c + 1 < B_NCH) __builtin_amdgcn_s_waitcnt(B_WAIT_VM7);
        else __builtin_amdgcn_s_waitcnt(B_WAIT_VM0);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int s = 0; s < 2; ++s) {  // 16-deep k-step s: h2 group 2 s + lh of the chunk
            const int ph = 4 * s + 2 * lh;
            const h8 xh = rd(buf, 0, xrow, ph), xl = rd(buf, 0, xrow, ph + 1);
            h8 wh[5], wl[5];
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                wh[t] = rd(buf, B_ABYTES, wrow[t], ph);
                wl[t] = rd(buf, B_ABYTES, wrow[t], ph + 1);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t], xh, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 3; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl[t], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t], xl, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 3; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh[t], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t], xh, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 3; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh[t], acc[t], 0, 0, 0);
        }
        if (c + 2 < B_NCH) {
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's reads of `buf` are done
            __builtin_amdgcn_s_barrier();        // ... and every other wave's
            issue(c + 2, buf);
        }
    }
    __syncthreads();  // the GEMM staging becomes the K / V^T stages

    // ---- epilogue of phase 1: q into B fragments, k rows and V^T into the attention stages
    auto Kb = [&](int st) { return smem + st * B_ASTAGE; };
    auto Vhb = [&](int st) { return reinterpret_cast<unsigned*>(smem + st * B_ASTAGE + KT * KSB); };
    auto Vlb = [&](int st) { return reinterpret_cast<unsigned*>(smem + st * B_ASTAGE + KT * KSB + DP * VSW * 4); };
    h8 qh[3], ql[3];
    {
        const float wsc = *wscale;
        auto b8 = [&](int ch, f4& b0, f4& b1) {  // bias of 8 consecutive output channels from ch
            b0 = bias ? *reinterpret_cast<const f4*>(bias + ch) : (f4){};
            b1 = bias ? *reinterpret_cast<const f4*>(bias + ch + 4) : (f4){};
        };
        f4 bq[3][2], bk[3][2];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            b8(h * D + 16 * s + 8 * lh, bq[s][0], bq[s][1]);
            b8(C + h * D + 16 * s + 8 * lh, bk[s][0], bk[s][1]);
        }
        const float bv0 = bias ? bias[2 * C + h * D + li] : 0.f;
        const float bv1 = bias ? bias[2 * C + h * D + 32 + (li & 15)] : 0.f;
        bool bad = false;
        b_split8(acc[0], 0, wsc, bq[0][0], bq[0][1], qh[0], ql[0], bad);
        b_split8(acc[0], 8, wsc, bq[1][0], bq[1][1], qh[1], ql[1], bad);
        b_split8(acc[2], 0, wsc, bq[2][0], bq[2][1], qh[2], ql[2], bad);
        const int st = w >> 2, j = (w & 3) * 32 + li;  // this lane's key: stage and row
        char* const kr = Kb(st) + j * KSB;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            h8 kh, kl;
            b_split8(s < 2 ? acc[1] : acc[2], s < 2 ? 8 * s : 8, wsc, bk[s][0], bk[s][1], kh, kl, bad);
            *reinterpret_cast<h8*>(kr + (2 * s + lh) * 32) = kh;
            *reinterpret_cast<h8*>(kr + (2 * s + lh) * 32 + 16) = kl;
        }
        unsigned* const Vh = Vhb(st);
        unsigned* const Vl = Vlb(st);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float bv = t ? bv1 : bv0;
            const f4 bb = {bv, bv, bv, bv};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                h8 vh, vl;
                b_split8(acc[3 + t], 8 * s, wsc, bb, bb, vh, vl, bad);
                const int col = ((w & 3) * 32 + 16 * s + 8 * lh) >> 1;
                *reinterpret_cast<h8*>(&Vh[(32 * t + li) * VSW + col]) = vh;
                *reinterpret_cast<h8*>(&Vl[(32 * t + li) * VSW + col]) = vl;
            }
        }
        h2_flag(ovf, bad);
    }
    __syncthreads();

    // ---- phase 2: k_attention_split<48, 0>'s key-tile step on the two resident tiles
    constexpr int NST = KT / 32, DS = D / 16, DT = DP / 32;
    const float scale2 = scale * 1.4426950408889634f;  // log2(e) / sqrt(D)
    f32x16 oacc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) oacc[t] = (f32x16){};
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int cur = 0; cur < N / KT; ++cur) {
        const char* Ks = Kb(cur);
        const unsigned* Vh = Vhb(cur);
        const unsigned* Vl = Vlb(cur);
        f32x16 sacc[NST];
#pragma unroll
        for (int n = 0; n < NST; ++n) {
            sacc[n] = (f32x16){};
            const char* kr = Ks + (n * 32 + li) * KSB;
#pragma unroll
            for (int s = 0; s < DS; ++s) {
                const h8 kh = *reinterpret_cast<const h8*>(kr + (2 * s + lh) * 32);
                const h8 kl = *reinterpret_cast<const h8*>(kr + (2 * s + lh) * 32 + 16);
                sacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[s], sacc[n], 0, 0, 0);
                sacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[s], sacc[n], 0, 0, 0);
                sacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[s], sacc[n], 0, 0, 0);
            }
        }
        float mtn[NST];
#pragma unroll
        for (int n = 0; n < NST; ++n) {
            mtn[n] = sacc[n][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mtn[n] = fmaxf(mtn[n], sacc[n][r]);
        }
        float mt = mtn[0];
#pragma unroll
        for (int n = 1; n < NST; ++n) mt = fmaxf(mt, mtn[n]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale2);  // 0 on the first tile (m = -inf)
        const float mb = fmaf(-mn, scale2, 10.f);  // + 10: p is produced pre-scaled by 2^10
        m = mn;
        l *= alpha;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
        float ltn[NST];
#pragma unroll
        for (int n = 0; n < NST; ++n) {
            float& lt = ltn[n];
            lt = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int c0 = (n * 32 + 16 * s + 8 * lh) >> 1;
                h8 ph, pl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = __builtin_amdgcn_exp2f(fmaf(sacc[n][8 * s + e], scale2, mb));
                    lt += v;  // l, like the P operand, carries the 2^10 scale
                    const _Float16 hh = (_Float16)v;
                    ph[e] = hh;
                    pl[e] = (_Float16)(v - (float)hh);
                }
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const h8 vh = *reinterpret_cast<const h8*>(&Vh[(t * 32 + li) * VSW + c0]);
                    const h8 vl = *reinterpret_cast<const h8*>(&Vl[(t * 32 + li) * VSW + c0]);
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, oacc[t], 0, 0, 0);
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, oacc[t], 0, 0, 0);
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, oacc[t], 0, 0, 0);
                }
            }
        }
        float lt = ltn[0];
#pragma unroll
        for (int n = 1; n < NST; ++n) lt += ltn[n];
        lt += __shfl_xor(lt, 32);
        l += lt;
    }
    const float inv = 1.f / l;
    const int q = w * 32 + li;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = t * 32 + 8 * i + 4 * lh;
            if (d < D) {
                const float4 v = make_float4(oacc[t][4 * i] * inv, oacc[t][4 * i + 1] * inv, oacc[t][4 * i + 2] * inv,
                                             oacc[t][4 * i + 3] * inv);
                store4_h2x(out, ((size_t)b * N + q) * C * 4, (h * D + d) >> 2, v, false);
            }
        }
}

}  // namespace

// Shapes the fused kernel takes (unet.hip's unet_body falls back to the three launches otherwise): f16x3 records,
// N = 256 tokens, C = 192 in 4 heads, the qkv weight packed [3C][C] with no K padding, 16-B aligned pointers.
bool attn_block_ok(int fmt, int Bt, int N, int C, int heads, const tcx_conv& qkv, const tcx_conv& proj, const void* x,
                   const void* a, const void* o) {
    return fmt == 0 && Bt <= 65535 && N == B_N && C == B_C && heads * B_D == C && qkv.wh && qkv.wscale && proj.wh && proj.wscale &&
           qkv.ks == 1 && proj.ks == 1 && qkv.cin == C && qkv.cout == 3 * C && qkv.kpad == C &&
           qkv.cout_pad >= 3 * C && proj.cin == C && proj.cout == C && aligned16(x) && aligned16(a) && aligned16(o) &&
           aligned16(qkv.wh) && aligned16(proj.wh) && (!qkv.b || aligned16(qkv.b)) && x != o;
}

}  // namespace tcx

using namespace tcx;

extern "C" int tcx_attn_block_h2(const void* xh, float* a, void* oh, const void* qkv_wh, const float* qkv_wscale,
                                 const float* qkv_b, int qkv_cout_pad, const void* proj_wh, const float* proj_wscale,
                                 const float* proj_b, int proj_cout_pad, int Bt, int N, int C, int heads,
                                 unsigned* ovf, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    TCX_REQUIRE(xh && a && oh && qkv_wh && qkv_wscale && proj_wh && proj_wscale, "tcx_attn_block_h2: null pointer");
    TCX_REQUIRE(N == B_N && C == B_C && heads * B_D == C && qkv_cout_pad >= 3 * C && proj_cout_pad >= C,
                "tcx_attn_block_h2: needs N = 256, C = 192, 4 heads");
    TCX_REQUIRE(xh != oh && (const void*)a != oh, "tcx_attn_block_h2: the attention output must not alias an input");
    TCX_REQUIRE(aligned16(xh) && aligned16(a) && aligned16(oh) && aligned16(qkv_wh) && aligned16(proj_wh) &&
                    (!qkv_b || aligned16(qkv_b)),
                "tcx_attn_block_h2: pointers must be 16-B aligned");
    TCX_REQUIRE(Bt >= 0 && Bt <= 65535, "tcx_attn_block_h2: Bt must be in [0, 65535] (one grid row per image)");
    if (Bt == 0) return TCX_OK;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_block), hipFuncAttributeMaxDynamicSharedMemorySize,
                                B_LDS) != hipSuccess) {
            set_error("tcx_attn_block_h2: cannot enable %d B of dynamic LDS", B_LDS);
            return TCX_EHIP;
        }
        attr_set = true;
    }
    static const int xcd = [] {
        const char* e = getenv("TCX_ATTN_XCD");
        return (e && e[0] == '0') ? 0 : 1;
    }();
    const float scale = (float)(1.0 / std::sqrt((double)B_D));
    prof_begin(st);
    hipLaunchKernelGGL(k_attn_block, dim3(1, heads, Bt), dim3(512), B_LDS, st, (const char*)xh, (const float*)qkv_wh,
                       (unsigned)((size_t)qkv_cout_pad * C * 4), qkv_wscale, qkv_b, (char*)oh, ovf, scale, xcd);
    TCX_TRY(check_launch("tcx_attn_block_h2"));
    prof_end(st, 2.0 * Bt * N * 3.0 * C * C + 4.0 * Bt * (double)N * N * C);  // qkv GEMM + Q K^T + P V
    // proj + bias + residual, in place on a: the k_lin1x1 launch of the three-launch path, unchanged
    return tcx_conv2d_h2_pro(oh, nullptr, Bt, 0, N / 16, 16, C, 0, proj_wh, nullptr, proj_wscale, proj_b, nullptr, a, a, 0, C,
                             proj_cout_pad, C, 1, 1, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, ovf, st);
}
