// The head of CondUNetTiny: GroupNorm+SiLU of up1's last conv fused with the out conv's channel reduction,
//   r[b][tap][p] = sum_ci silu(gn(h))[b,p,ci] * w_out[ci][tap]   (a 9-wide GEMV per pixel);
// the out conv's 9-tap circular gather of r is k_step's (unet_step.hip).  Kernels: k_head (any C, LDS tile),
// k_head8 (C = 32 Q, 8 lanes per pixel) and k_head8r (its register-weight form); launch_head() picks.
#include "h2.hpp"
#include "passes.hpp"
#include "unet.hpp"

namespace tcx {
namespace {

// Head: out conv (C -> 1, 3x3 circular) split into a per-pixel channel reduction here and a
// 9-tap circular gather in k_step.  grid (HW/128, Bt); block 256.  The 128-pixel x C tile is read
// coalesced (contiguous 128*C floats), GroupNorm+SiLU applied from the per-image table, staged in
// LDS; then thread (pixel, tap set) computes r[b][tap][p] = sum_c h[p][c] * w_out[c][tap].
constexpr int HEAD_PX = 64;
__global__ __launch_bounds__(256) void k_head(const float* __restrict__ h, int HW, int C, const float* __restrict__ tsc,
                                              const float* __restrict__ tsh, const float* __restrict__ w_out,
                                              float* __restrict__ r) {
    extern __shared__ __attribute__((aligned(16))) float hs[];  // tile[128][C+4] | w[9][C] | sc[C] sh[C]
    const int LD = C + 4;
    float* tile = hs;
    float* w = hs + HEAD_PX * LD;
    float* sc = w + 9 * C;
    float* sh = sc + C;
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * HEAD_PX;
    const int tid = threadIdx.x;
    const int C4 = C / 4;
    const int npx = min(HEAD_PX, HW - p0);
    const float* src = h + ((size_t)b * HW + p0) * C;
    // the tile's loads are all issued before anything waits on them (HK float4 per thread in
    // flight: the block's whole 64 x C tile for C <= 128); a load-transform-store loop keeps one
    // load per thread in flight and ran at 2.8 TB/s
    constexpr int HK = 8;
    const int nq = npx * C4;
    const bool hoist = nq <= HK * 256;
    float4 v[HK];
    if (hoist) {
#pragma unroll
        for (int k = 0; k < HK; ++k) {
            const int i = tid + 256 * k;
            if (i < nq) v[k] = *reinterpret_cast<const float4*>(src + (size_t)i * 4);
        }
    }
    for (int i = tid; i < 9 * C; i += 256) {
        const int c = i / 9, k = i - (i / 9) * 9;  // w_out is [C][9]; stored tap-major
        w[k * C + c] = w_out[i];
    }
    for (int c = tid; c < C; c += 256) {
        sc[c] = tsc[(size_t)b * C + c];
        sh[c] = tsh[(size_t)b * C + c];
    }
    __syncthreads();
    auto put = [&](int i, float4 u) {
        const int px = i / C4, c = (i - (i / C4) * C4) * 4;
        u.x = silu_f(fmaf(u.x, sc[c], sh[c]));
        u.y = silu_f(fmaf(u.y, sc[c + 1], sh[c + 1]));
        u.z = silu_f(fmaf(u.z, sc[c + 2], sh[c + 2]));
        u.w = silu_f(fmaf(u.w, sc[c + 3], sh[c + 3]));
        *reinterpret_cast<float4*>(&tile[px * LD + c]) = u;
    };
    if (hoist) {
#pragma unroll
        for (int k = 0; k < HK; ++k) {
            const int i = tid + 256 * k;
            if (i < nq) put(i, v[k]);
        }
    } else {
        for (int i = tid; i < nq; i += 256) put(i, *reinterpret_cast<const float4*>(src + (size_t)i * 4));
    }
    __syncthreads();
    const int px = tid & (HEAD_PX - 1);
    const int tg = tid >> 6;  // tap group: taps tg, tg + 4, (tg + 8 for group 0)
    if (px >= npx) return;
    const int nk = tg == 0 ? 3 : 2;
    float acc[3] = {0.f, 0.f, 0.f};
    const float* row = &tile[px * LD];
    for (int c = 0; c < C; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < nk) {
                const float4 ww = *reinterpret_cast<const float4*>(&w[(tg + 4 * j) * C + c]);  // broadcast
                float a = acc[j];
                a = fmaf(v.x, ww.x, a);
                a = fmaf(v.y, ww.y, a);
                a = fmaf(v.z, ww.z, a);
                a = fmaf(v.w, ww.w, a);
                acc[j] = a;
            }
        }
    }
    float* dst = r + (size_t)b * 9 * HW + p0 + px;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < nk) dst[(size_t)(tg + 4 * j) * HW] = acc[j];
}

// Head, register form (round 3): as k_head8, but each lane's CL channels of w_out (9 taps) and of the
// image's scale / shift live in VGPRs for the whole block instead of being re-read from LDS for every
// element (5 LDS reads per element, ~22 LDS clocks per wave-element: the LDS, not HBM, bounded
// k_head8).  A block takes HR_PASS passes of 32 pixels of one image; the loads of the next two passes
// are in flight during the current pass's math (~185 VGPRs: 2 waves per SIMD).  Same arithmetic in the
// same order as k_head8 (bit-identical).
constexpr int HR_PASS = 8;
constexpr int HPR = 32 * HR_PASS;
// B2: the source is 2-byte bf16 (config 5: up1_1's pre-norm output, h2.hpp "b2"): 8 B per 4 channels
template <bool B2>
__device__ __forceinline__ float4 head_ld4(const float* h, size_t e) {
    if constexpr (B2) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(h) + e * 2);
        return make_float4(bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y));
    } else {
        return *reinterpret_cast<const float4*>(h + e);
    }
}
// LA: passes whose loads are in flight ahead of the one being computed (round 5: 2 -> 4, the whole pass
// loop unrolled so the ring is static; 2 passes ahead left the 403 MB read at 3.8 TB/s)
constexpr int HR_LA = 4;
// a + (a of the lane that DPP control CTRL names): an 8-lane group's xor-shuffle sum without the LDS
// crossbar (ds_bpermute: an address, an LDS round trip and a wait per stage)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float a) {
    // (every lane reads a lane of its own row: bound_ctrl only lets the move fold into the add's DPP operand)
    return a + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), CTRL, 0xf, 0xf, true));
}
// SHFL: the three reduction stages as __shfl_xor (the form before the DPP adds; tcx_debug_pass_forms bit 2)
template <int Q, bool B2 = false, bool SHFL = false>
__global__ __launch_bounds__(256) void k_head8r(const float* __restrict__ h, int HW, const float* __restrict__ tsc,
                                                const float* __restrict__ tsh, const float* __restrict__ w_out,
                                                float* __restrict__ r) {
    constexpr int C = 32 * Q;
    constexpr int CL = 4 * Q;
    const int p0 = blockIdx.x * HPR;
    const int b = p0 / HW;
    const int tid = threadIdx.x;
    const int sub = tid & 7, pl = tid >> 3;
    const int c0 = sub * CL;
    float4 v[HR_PASS][Q];  // pass k's channels; only HR_LA + 1 passes are live at a time
    const size_t src0 = (size_t)(p0 + pl) * C + c0;
    // config 5's b2 head (B2, C = 96, round 6): lane sub takes channels [8 sub, 8 sub + 8) — one 16-B load, the 8
    // lanes of a pixel its first 128 contiguous bytes — and [64 + 4 sub, 64 + 4 sub + 4) — one 8-B load, the
    // last 64 B — instead of 12 contiguous channels as three 8-B loads at a 24-B lane stride (the 1.06 GB read
    // ran at 2.3 TB/s, r06_b layers).  The lane's channel j is 8 sub + j (j < 8) or 64 + 4 sub + j - 8.
    constexpr bool CM = B2 && Q == 3;
    auto ld_pass = [&](int k) __attribute__((always_inline)) {
        if constexpr (CM) {
            const char* hp = reinterpret_cast<const char*>(h) + ((size_t)(p0 + pl + k * 32) * C) * 2;
            const uint4 a = *reinterpret_cast<const uint4*>(hp + 16 * sub);
            const uint2 c = *reinterpret_cast<const uint2*>(hp + 128 + 8 * sub);
            v[k][0] = make_float4(bf_lo(a.x), bf_hi(a.x), bf_lo(a.y), bf_hi(a.y));
            v[k][1] = make_float4(bf_lo(a.z), bf_hi(a.z), bf_lo(a.w), bf_hi(a.w));
            v[k][2 % Q] = make_float4(bf_lo(c.x), bf_hi(c.x), bf_lo(c.y), bf_hi(c.y));
        } else {
#pragma unroll
            for (int q = 0; q < Q; ++q) v[k][q] = head_ld4<B2>(h, src0 + (size_t)k * 32 * C + 4 * q);
        }
    };
#pragma unroll
    for (int k = 0; k < HR_LA && k < HR_PASS; ++k) ld_pass(k);
    // the lane's constants as 16-B loads (its 9 CL weights are contiguous in w_out[c][tap], its CL scale /
    // shift entries in the image's table rows): 9 Q + 2 Q vector loads instead of 11 CL scalar ones, which
    // were 5x the data loads' instruction count per block
    float wr[CL][9], scl[CL], shf[CL];
    {
        float4 wq[9 * Q], sq[Q], hq[Q];
        if constexpr (CM) {  // channels 8 sub .. + 7 (18 float4 of w_out), then 64 + 4 sub .. + 3 (9 float4)
            const float4* wa = reinterpret_cast<const float4*>(w_out + (size_t)(8 * sub) * 9);
            const float4* wb = reinterpret_cast<const float4*>(w_out + (size_t)(64 + 4 * sub) * 9);
#pragma unroll
            for (int i = 0; i < 18; ++i) wq[i] = wa[i];
#pragma unroll
            for (int i = 0; i < 9; ++i) wq[18 + i] = wb[i];
            const float* ts = tsc + (size_t)b * C;
            const float* th = tsh + (size_t)b * C;
            sq[0] = reinterpret_cast<const float4*>(ts + 8 * sub)[0];
            sq[1] = reinterpret_cast<const float4*>(ts + 8 * sub)[1];
            sq[2 % Q] = reinterpret_cast<const float4*>(ts + 64 + 4 * sub)[0];
            hq[0] = reinterpret_cast<const float4*>(th + 8 * sub)[0];
            hq[1] = reinterpret_cast<const float4*>(th + 8 * sub)[1];
            hq[2 % Q] = reinterpret_cast<const float4*>(th + 64 + 4 * sub)[0];
        } else {
            const float4* wp = reinterpret_cast<const float4*>(w_out + (size_t)c0 * 9);
#pragma unroll
            for (int i = 0; i < 9 * Q; ++i) wq[i] = wp[i];
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                sq[i] = reinterpret_cast<const float4*>(tsc + (size_t)b * C + c0)[i];
                hq[i] = reinterpret_cast<const float4*>(tsh + (size_t)b * C + c0)[i];
            }
        }
#pragma unroll
        for (int f = 0; f < 36 * Q; ++f) {
            const float4 v = wq[f >> 2];
            wr[f / 9][f % 9] = (f & 3) == 0 ? v.x : (f & 3) == 1 ? v.y : (f & 3) == 2 ? v.z : v.w;
        }
#pragma unroll
        for (int j = 0; j < CL; ++j) {
            const float4 a = sq[j >> 2], c = hq[j >> 2];
            scl[j] = (j & 3) == 0 ? a.x : (j & 3) == 1 ? a.y : (j & 3) == 2 ? a.z : a.w;
            shf[j] = (j & 3) == 0 ? c.x : (j & 3) == 1 ? c.y : (j & 3) == 2 ? c.z : c.w;
        }
    }
#pragma unroll
    for (int pass = 0; pass < HR_PASS; ++pass) {
        const int pg = p0 + pass * 32 + pl;
        if (pass + HR_LA < HR_PASS) ld_pass(pass + HR_LA);
        float acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float xs[4] = {v[pass][q].x, v[pass][q].y, v[pass][q].z, v[pass][q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q + e;
                const float yv = fmaf(xs[e], scl[j], shf[j]);
                const float x = yv * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * yv));
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[t] = fmaf(x, wr[j][t], acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if constexpr (SHFL) {
                acc[t] += __shfl_xor(acc[t], 1);
                acc[t] += __shfl_xor(acc[t], 2);
                acc[t] += __shfl_xor(acc[t], 4);
            } else {
                // quad_perm [1,0,3,2] and [2,3,0,1] are lanes ^ 1 and ^ 2.  Every lane of a quad then holds the
                // quad's sum, so lane 7 - i of the 8-lane group (row_half_mirror) carries what lane i ^ 4 does:
                // the operands of each add are those of the shuffles (an fp32 add commutes: the same bits)
                acc[t] = dpp_add<0xB1>(acc[t]);
                acc[t] = dpp_add<0x4E>(acc[t]);
                acc[t] = dpp_add<0x141>(acc[t]);
            }
        }
        const int p = pg - b * HW;
        float* dst = r + (size_t)b * 9 * HW + p;
        float mine = acc[0];
#pragma unroll
        for (int t = 1; t < 8; ++t)
            if (sub == t) mine = acc[t];
        dst[(size_t)sub * HW] = mine;  // lane sub writes tap sub; lane 0 also tap 8
        if (sub == 0) dst[(size_t)8 * HW] = acc[8];
    }
}

// ---------------------------------------------------------------- 8-lanes-per-pixel forms
// For C = 32*Q (every split-path net): a pixel's C channels are 8 contiguous runs of 4Q channels,
// one per lane of an 8-lane group, so a wave reads/writes 8 whole pixels (8*C*4 contiguous bytes)
// per instruction group and nothing goes through an LDS tile; per-pixel reductions are three
// xor-shuffles inside the group (fixed order).

// (A first-conv of this form measured slower than k_conv_first: its per-lane 48-B output runs
// leave every store instruction one-third coalesced, where the LDS tile writes 1 KB contiguous.)
// Head, 8-lane form: r[b][tap][p] = sum_c silu(gn(h))[b,p,c] * w_out[c][tap].  Block 256 threads =
// 32 pixels per pass, HP8 pixels per block (all in one image: HW % HP8 == 0).  w_out and the
// image's scale/shift rows are staged in LDS once per block.
constexpr int HP8 = 128;
template <int Q>
__global__ __launch_bounds__(256) void k_head8(const float* __restrict__ h, int HW, const float* __restrict__ tsc,
                                               const float* __restrict__ tsh, const float* __restrict__ w_out,
                                               float* __restrict__ r) {
    constexpr int C = 32 * Q;
    constexpr int CL = 4 * Q;  // channels per lane
    __shared__ __attribute__((aligned(16))) float ws[C * 12];  // [c][12]: taps 0-8 + pad: 3 ds_read_b128 per channel
    __shared__ __attribute__((aligned(16))) float ssc[C], ssh[C];
    const int p0 = blockIdx.x * HP8;  // first pixel (flat over b, p)
    const int b = p0 / HW;
    const int tid = threadIdx.x;
    const int sub = tid & 7, pl = tid >> 3;  // lane in the pixel group, pixel of the pass
    const int c0 = sub * CL;
    // the first pass's loads go out before the tables are staged
    float4 v[Q];
    {
        const float* src = h + (size_t)(p0 + pl) * C + c0;
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q] = *reinterpret_cast<const float4*>(src + 4 * q);
    }
    for (int i = tid; i < C * 12; i += 256) {
        const int c = i / 12, t = i - (i / 12) * 12;
        ws[i] = t < 9 ? w_out[c * 9 + t] : 0.f;
    }
    for (int i = tid; i < C; i += 256) {
        ssc[i] = tsc[(size_t)b * C + i];
        ssh[i] = tsh[(size_t)b * C + i];
    }
    __syncthreads();
    for (int pass = 0; pass < HP8 / 32; ++pass) {
        const int pg = p0 + pass * 32 + pl;
        float4 vn[Q];
        if (pass + 1 < HP8 / 32) {  // next pass's loads in flight during this pass's math
            const float* src = h + (size_t)(pg + 32) * C + c0;
#pragma unroll
            for (int q = 0; q < Q; ++q) vn[q] = *reinterpret_cast<const float4*>(src + 4 * q);
        }
        float acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = 0.f;
#pragma unroll 1
        for (int q = 0; q < Q; ++q) {
            float4 vq = v[0];  // register select (a runtime-indexed v[q] would go to scratch)
#pragma unroll
            for (int j = 1; j < Q; ++j)
                if (q == j) vq = v[j];
            const float xs[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + 4 * q + e;
                // SiLU as y rcp(1 + exp2(-y log2 e)) (hardware exp2 / rcp, as the conv prologues): the
                // IEEE expf + division form made this kernel VALU-bound (~25 instructions per element)
                const float yv = fmaf(xs[e], ssc[c], ssh[c]);
                const float x = yv * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * yv));
                const float4 w0 = *reinterpret_cast<const float4*>(&ws[c * 12]);
                const float4 w1 = *reinterpret_cast<const float4*>(&ws[c * 12 + 4]);
                const float w8 = ws[c * 12 + 8];
                acc[0] = fmaf(x, w0.x, acc[0]); acc[1] = fmaf(x, w0.y, acc[1]);
                acc[2] = fmaf(x, w0.z, acc[2]); acc[3] = fmaf(x, w0.w, acc[3]);
                acc[4] = fmaf(x, w1.x, acc[4]); acc[5] = fmaf(x, w1.y, acc[5]);
                acc[6] = fmaf(x, w1.z, acc[6]); acc[7] = fmaf(x, w1.w, acc[7]);
                acc[8] = fmaf(x, w8, acc[8]);
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            acc[t] += __shfl_xor(acc[t], 1);
            acc[t] += __shfl_xor(acc[t], 2);
            acc[t] += __shfl_xor(acc[t], 4);
        }
        const int p = pg - b * HW;
        float* dst = r + (size_t)b * 9 * HW + p;
        dst[(size_t)sub * HW] = acc[sub];  // lane sub writes tap sub; lane 0 also tap 8
        if (sub == 0) dst[(size_t)8 * HW] = acc[8];
        if (pass + 1 < HP8 / 32) {
#pragma unroll
            for (int q = 0; q < Q; ++q) v[q] = vn[q];
        }
    }
}

}  // namespace

int launch_head(const tcx_unet* net, const Plan& P, int fmt, hipStream_t st) {
    const int Bt = P.Bt, C = P.C;
    TCX_REQUIRE(C % 4 == 0, "head: C %% 4");
    // up1_1 wrote its output as 2-byte bf16 at fmt 2, which only k_head8r<3, true> reads: a
    // caller's out_w without 16-B alignment (that kernel's constant loads) is an error, never a
    // fall-through to a head that reads the tensor as fp32
    TCX_REQUIRE(fmt != 2 || (P.P0 % HPR == 0 && C == 96 && aligned16(net->out_w)),
                "tcx_unet: the 2-byte bf16 head needs out_w 16-byte aligned and H*W %% %d == 0", HPR);
    // register-weight head (r03_ag: 124 -> 118 us at 64^2); k_head8 for other widths / shapes
    if (P.P0 % HPR == 0 && (C == 96 || C == 64 || C == 32) && aligned16(net->out_w)) {  // (16-B constant loads)
        const dim3 gr(Bt * P.P0 / HPR);
        const bool shfl = (pass_forms() & 4) != 0;
#define TCX_HEAD8R(Q, B2)                                                                                        \
    do {                                                                                                         \
        if (shfl)                                                                                                \
            hipLaunchKernelGGL((k_head8r<Q, B2, true>), gr, dim3(256), 0, st, P.a64, P.P0, P.sc(10), P.sh(10),   \
                               net->out_w, P.r);                                                                 \
        else                                                                                                     \
            hipLaunchKernelGGL((k_head8r<Q, B2, false>), gr, dim3(256), 0, st, P.a64, P.P0, P.sc(10), P.sh(10),  \
                               net->out_w, P.r);                                                                 \
    } while (0)
        if (C == 96 && fmt == 2) TCX_HEAD8R(3, true);
        else if (C == 96) TCX_HEAD8R(3, false);
        else if (C == 64) TCX_HEAD8R(2, false);
        else TCX_HEAD8R(1, false);
#undef TCX_HEAD8R
        TCX_TRY(check_launch("k_head8r"));
    } else if (P.P0 % HP8 == 0 && (C == 96 || C == 64 || C == 128 || C == 32)) {
        const dim3 g8(Bt * P.P0 / HP8);
        if (C == 96) hipLaunchKernelGGL(k_head8<3>, g8, dim3(256), 0, st, P.a64, P.P0, P.sc(10), P.sh(10), net->out_w, P.r);
        else if (C == 64) hipLaunchKernelGGL(k_head8<2>, g8, dim3(256), 0, st, P.a64, P.P0, P.sc(10), P.sh(10), net->out_w, P.r);
        else if (C == 128) hipLaunchKernelGGL(k_head8<4>, g8, dim3(256), 0, st, P.a64, P.P0, P.sc(10), P.sh(10), net->out_w, P.r);
        else hipLaunchKernelGGL(k_head8<1>, g8, dim3(256), 0, st, P.a64, P.P0, P.sc(10), P.sh(10), net->out_w, P.r);
        TCX_TRY(check_launch("k_head8"));
    } else {
        const size_t shm = ((size_t)HEAD_PX * (C + 4) + 11 * (size_t)C) * sizeof(float);
        const dim3 grid(cdiv(P.P0, HEAD_PX), Bt);
        hipLaunchKernelGGL(k_head, grid, dim3(256), shm, st, P.a64, P.P0, C, P.sc(10), P.sh(10), net->out_w, P.r);
        TCX_TRY(check_launch("k_head"));
    }
    return TCX_OK;
}

}  // namespace tcx
