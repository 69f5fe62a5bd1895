// down1's first conv of CondUNetTiny (17 -> C0, 3x3 circular; the reference's sde_score_model.py:243-255): only
// the x_t channel is convolved, the 16 spatially-constant map channels arrive folded into a per-image bias
// (unet_cond.hip).  Kernels: k_conv_first (the LDS-tile form: fp32 output + GroupNorm partials, or records),
// k_first_acf + k_first_gnsum (GroupNorm_0's statistics without evaluating the conv), k_conv_first_rec and
// k_conv_first_rec96 (silu(GroupNorm_0(conv)) straight as down1.net.3's records); first_conv() picks.
#include "h2.hpp"
#include "passes.hpp"
#include "unet.hpp"

namespace tcx {
namespace {

// First conv of down1 (17 -> C0, 3x3 circular) with the 16 constant map channels already folded
// into bias_b: y[b,p,co] = bias_b[b][co] + sum_tap w0[co][tap] * x[b % bmod][wrap(p + tap)].
// Output-write bound (C0 floats per input float): a 64-pixel x C0 tile is built in LDS (small, so
// several blocks per CU overlap their load/compute/store phases) and written as one contiguous
// block; per-channel {sum, sumsq} (fp64) of the tile feed the following GroupNorm.
// grid (HW/64, Bt); block 256 = 64 pixels x 4 channel quarters; needs HW % 128 == 0, C0 % 16 == 0.
// MODE 0: fp32 output + GroupNorm partials per 64-pixel tile (the fp32 path / the f16x3 prologue form).
// MODE 2 (split path, round 3): silu(GroupNorm_0(conv)) written as the h2 / bf16 record of
//   down1.net.3's input (scale/shift tables of tcx_gn_finalize over the statistics of k_first_acf /
//   k_first_gnsum below; SiLU as the conv prologues: y rcp(1 + exp2(-y log2 e))), so that conv runs
//   without a prologue and the fp32 tensor is never written or re-read.
constexpr int FIRST_PX = 64;
template <int MODE>
__global__ __launch_bounds__(256) void k_conv_first(const float* __restrict__ x, int bmod, int H, int W, int C0,
                                                    const float* __restrict__ w0, int kpad,
                                                    const float* __restrict__ bias_b, float* __restrict__ y,
                                                    double* __restrict__ gn, CondTab ct, int Bimg, int cfg,
                                                    const float* __restrict__ tsc, const float* __restrict__ tsh,
                                                    unsigned* ovf, int bf) {
    extern __shared__ __attribute__((aligned(16))) float fs[];  // tile[64][C0+4] | w[9][C0] | red[4][C0][2] (dbl)
    const int LD = C0 + 4;
    float* tile = fs;
    float* w = fs + FIRST_PX * LD;
    double* red = reinterpret_cast<double*>(w + 9 * C0);
    const int HW = H * W;
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    for (int i = tid; i < 9 * C0; i += 256) {
        const int co = i / 9, k = i - (i / 9) * 9;  // w0 packed [co][kpad] with k = tap (Cin = 1)
        w[k * C0 + co] = w0[(size_t)co * kpad + k];
    }
    float* const tab = reinterpret_cast<float*>(red);  // MODE 2: this image's scale | shift (LDS)
    if constexpr (MODE == 2) {
        for (int c = tid; c < C0; c += 256) {
            tab[c] = tsc[(size_t)b * C0 + c];
            tab[C0 + c] = tsh[(size_t)b * C0 + c];
        }
    }
    const int px = tid & (FIRST_PX - 1), qtr = tid >> 6;
    const float* xb = x + (size_t)(b % bmod) * HW;
    const int cq = C0 / 4;
    const float* bb = ct.bias_img ? cond_bias_row(ct, b, Bimg, cfg, C0) : bias_b + (size_t)b * C0;
    constexpr int NT = 1;
    double as[2] = {0.0, 0.0}, aq[2] = {0.0, 0.0};  // this thread's (quarter, c) sums
    for (int tt = 0; tt < NT; ++tt) {
        const int p0 = (blockIdx.x * NT + tt) * FIRST_PX;
        __syncthreads();  // w staged / the previous tile consumed
        const int p = p0 + px;
        const int yy = p / W, xx = p - (p / W) * W;
        float xv[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) xv[dy * 3 + dx] = xb[wrap_idx(yy + dy - 1, H) * W + wrap_idx(xx + dx - 1, W)];
        for (int c = qtr * cq; c < (qtr + 1) * cq; c += 4) {
            float4 a = *reinterpret_cast<const float4*>(bb + c);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float4 wk = *reinterpret_cast<const float4*>(&w[k * C0 + c]);  // broadcast read
                a.x = fmaf(wk.x, xv[k], a.x);
                a.y = fmaf(wk.y, xv[k], a.y);
                a.z = fmaf(wk.z, xv[k], a.z);
                a.w = fmaf(wk.w, xv[k], a.w);
            }
            *reinterpret_cast<float4*>(&tile[px * LD + c]) = a;
        }
        __syncthreads();
        if constexpr (MODE == 0) {
            float* dst = y + ((size_t)b * HW + p0) * C0;
            const int C4 = C0 / 4;
            for (int i = tid; i < FIRST_PX * C4; i += 256) {
                const int r = i / C4, c = (i - (i / C4) * C4) * 4;
                *reinterpret_cast<float4*>(dst + (size_t)i * 4) = *reinterpret_cast<const float4*>(&tile[r * LD + c]);
            }
        } else if constexpr (MODE == 2) {
            // 8-channel groups, channel fastest: consecutive threads write consecutive 32-B records
            char* dst = reinterpret_cast<char*>(y) + ((size_t)b * HW + p0) * C0 * 4;
            const int C8 = C0 / 8;
            const float* s8 = tab;
            const float* h8p = tab + C0;
            bool bad = false;
            for (int i = tid; i < FIRST_PX * C8; i += 256) {
                const int r = i / C8, g = i - (i / C8) * C8;
                const float4 v0 = *reinterpret_cast<const float4*>(&tile[r * LD + 8 * g]);
                const float4 v1 = *reinterpret_cast<const float4*>(&tile[r * LD + 8 * g + 4]);
                const float4 s0 = *reinterpret_cast<const float4*>(s8 + 8 * g);
                const float4 s1 = *reinterpret_cast<const float4*>(s8 + 8 * g + 4);
                const float4 t0 = *reinterpret_cast<const float4*>(h8p + 8 * g);
                const float4 t1 = *reinterpret_cast<const float4*>(h8p + 8 * g + 4);
                auto sl = [](float v, float sc, float sh) {
                    const float q = fmaf(v, sc, sh);
                    return q * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * q));
                };
                const float4 a0 = make_float4(sl(v0.x, s0.x, t0.x), sl(v0.y, s0.y, t0.y), sl(v0.z, s0.z, t0.z),
                                              sl(v0.w, s0.w, t0.w));
                const float4 a1 = make_float4(sl(v1.x, s1.x, t1.x), sl(v1.y, s1.y, t1.y), sl(v1.z, s1.z, t1.z),
                                              sl(v1.w, s1.w, t1.w));
                uint2 hi0, lo0, hi1, lo1;
                split4x(a0, hi0, lo0, bf != 0);
                split4x(a1, hi1, lo1, bf != 0);
                if (!bf)
                    bad = bad || h2_bad(a0.x) || h2_bad(a0.y) || h2_bad(a0.z) || h2_bad(a0.w) || h2_bad(a1.x) ||
                          h2_bad(a1.y) || h2_bad(a1.z) || h2_bad(a1.w);
                char* gp = dst + (size_t)r * C0 * 4 + 32 * g;
                *reinterpret_cast<uint4*>(gp) = make_uint4(hi0.x, hi0.y, hi1.x, hi1.y);
                *reinterpret_cast<uint4*>(gp + 16) = make_uint4(lo0.x, lo0.y, lo1.x, lo1.y);
            }
            h2_flag(ovf, bad);
        }
        if constexpr (MODE != 2) {
            if (gn) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = tid + 256 * e;
                    if (i < 4 * C0) {
                        const int c = i % C0, part = i / C0;  // 4 row quarters of 16 pixels
                        double s = 0.0, q = 0.0;
                        for (int r = part * 16; r < part * 16 + 16; ++r) {
                            const double v = tile[r * LD + c];
                            s += v;
                            q += v * v;
                        }
                        as[e] += s;
                        aq[e] += q;
                    }
                }
            }
        }
    }
    if constexpr (MODE != 2) {
        if (gn) {  // 128-pixel GN split = 2 tiles (each half-split in its own slot, summed by the
                   // consumer's fold)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = tid + 256 * e;
                if (i < 4 * C0) {
                    red[i * 2] = as[e];
                    red[i * 2 + 1] = aq[e];
                }
            }
            __syncthreads();
            const int nsplit = HW / (FIRST_PX * NT);
            for (int c = tid; c < C0; c += 256) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int part = 0; part < 4; ++part) {
                    s += red[(part * C0 + c) * 2];
                    q += red[(part * C0 + c) * 2 + 1];
                }
                double* g = gn + (((size_t)b * nsplit + blockIdx.x) * C0 + c) * 2;
                g[0] = s;
                g[1] = q;
            }
        }
    }
}

// GroupNorm statistics of the first conv without evaluating it (split path, round 3).  The conv is
// out[p][c] = bias[c] + sum_k w[c][k] x[p + o_k] over the 9 circular taps o_k of ONE input channel, so
//   sum_p out   = HW bias + (sum_k w_k) S,                         S = sum_q x[q]
//   sum_p out^2 = HW bias^2 + 2 bias (sum_k w_k) S + sum_{k,l} w_k w_l R(o_l - o_k),  R(d) = sum_q x[q] x[q + d]
// (circular shifts preserve both sums): per image, S and the 25 circular autocorrelations R(d),
// d in [-2, 2]^2, then 96 channel sums from them.  Everything in fp64 from the fp32 inputs.
// k_first_acf: grid (HW / chunk, Bt) -> part[b][chunk][26] (chunk = 1024 pixels: at 64^2 a 4096-pixel
// chunk is one workgroup per image, one wave per SIMD with nothing to hide its fp64 chains and loads
// behind: 44 vs 31 us per launch, r03_af vs r03_z; equal at 256^2); k_first_gnsum: grid Bt -> the [Bt][1][C0][2]
// GroupNorm partials tcx_gn_finalize reads (one split).
constexpr int FIRST_ACF_PX = 1024;  // smallest chunk (HW % 1024 == 0)
__global__ __launch_bounds__(256) void k_first_acf(const float* __restrict__ x, int bmod, int H, int W, int chunk,
                                                   double* __restrict__ part) {
    __shared__ double wred[4][26];
    const int b = blockIdx.y, HW = H * W;
    const float* xb = x + (size_t)(b % bmod) * HW;
    double acc[26];
#pragma unroll
    for (int k = 0; k < 26; ++k) acc[k] = 0.0;
    for (int p = blockIdx.x * chunk + threadIdx.x; p < (blockIdx.x + 1) * chunk; p += 256) {
        const int yy = p / W, xx = p - (p / W) * W;
        const double v = xb[p];
        acc[25] += v;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const float* row = xb + wrap_idx(yy + dy, H) * W;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) acc[(dy + 2) * 5 + dx + 2] = fma(v, (double)row[wrap_idx(xx + dx, W)], acc[(dy + 2) * 5 + dx + 2]);
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        double t = acc[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) wred[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 26) {
        const int k = threadIdx.x;
        part[((size_t)b * gridDim.x + blockIdx.x) * 26 + k] = ((wred[0][k] + wred[1][k]) + wred[2][k]) + wred[3][k];
    }
}

__global__ __launch_bounds__(256) void k_first_gnsum(const double* __restrict__ part, int nchunk, int HW, int C0,
                                                     const float* __restrict__ w0, int kpad,
                                                     const float* __restrict__ bias_b, CondTab ct, int Bimg, int cfg,
                                                     double* __restrict__ gn) {
    __shared__ double a[26];
    const int b = blockIdx.x;
    if (threadIdx.x < 26) {
        double t = 0.0;
        // the CFG halves share x_t: k_first_acf ran over the Bimg distinct images only
        for (int j = 0; j < nchunk; ++j) t += part[((size_t)(b % Bimg) * nchunk + j) * 26 + threadIdx.x];
        a[threadIdx.x] = t;
    }
    __syncthreads();
    const float* bb = ct.bias_img ? cond_bias_row(ct, b, Bimg, cfg, C0) : bias_b + (size_t)b * C0;
    for (int c = threadIdx.x; c < C0; c += 256) {
        double w[9], ws = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            w[k] = w0[(size_t)c * kpad + k];
            ws += w[k];
        }
        const double bi = bb[c], S = a[25];
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int l = 0; l < 9; ++l) {
                const int dy = l / 3 - k / 3, dx = l % 3 - k % 3;
                q = fma(w[k] * w[l], a[(dy + 2) * 5 + dx + 2], q);
            }
        double* g = gn + ((size_t)b * C0 + c) * 2;
        g[0] = (double)HW * bi + ws * S;
        g[1] = (double)HW * bi * bi + 2.0 * bi * ws * S + q;
    }
}

// First conv + GroupNorm_0 + SiLU written straight as down1.net.3's h2 / bf16 records (round 3, the
// tile-free form of k_conv_first<2>): a workgroup takes FR_PX pixels of one image (one or more whole
// rows, or part of one); the x_t rows it touches (plus the wrapped row above / below) are staged in LDS
// once, with the 3x3 weights [tap][C0] and the image's bias / scale / shift rows; then each thread
// computes whole 8-channel records (item = pixel * C0/8 + group: consecutive lanes write consecutive
// 32-B records, as the tile form's store phase) from 9 broadcast x reads and 18 b128 weight reads.
// No fp32 tile, one barrier, ~5-8 KB of LDS (the tile form held 35 KB: 4 workgroups per CU).
// Needs HW % FR_PX == 0, and FR_PX % W == 0 or W % FR_PX == 0; C0 % 8 == 0.
// fpx (round 6): pixels per workgroup, FR_PX at 64^2; at config 5's 256^2 rows FR_PX_WIDE: the 128-pixel blocks
// (43,008 workgroups per 84-image pass) spent their time on the per-block prologue — three staged x rows,
// the 9 x C0 weight transpose, the bias / table rows — and wrote 1.06 GB at 2.0 TB/s (r06_b layers).
constexpr int FR_PX = 128;
constexpr int FR_PX_WIDE = 1024;
__global__ __launch_bounds__(256) void k_conv_first_rec(const float* __restrict__ x, int bmod, int H, int W, int C0,
                                                        const float* __restrict__ w0, int kpad,
                                                        const float* __restrict__ bias_b, char* __restrict__ y,
                                                        CondTab ct, int Bimg, int cfg, const float* __restrict__ tsc,
                                                        const float* __restrict__ tsh, unsigned* ovf, int bf, int fpx) {
    extern __shared__ __attribute__((aligned(16))) float fr[];  // w[9][C0] | bias[C0] | sc[C0] | sh[C0] | xr[nr][W]
    float* w = fr;
    float* bs = w + 9 * C0;
    float* sc = bs + C0;
    float* sh = sc + C0;
    float* xr = sh + C0;
    const int HW = H * W;
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * fpx;
    const int y0 = p0 / W;                                  // first row of the block's pixels
    const int nrow = (fpx >= W ? fpx / W : 1) + 2;         // staged rows y0-1 .. y0+rows
    const float* xb = x + (size_t)(b % bmod) * HW;
    for (int i = tid; i < nrow * W; i += 256) {
        const int r = i / W, c = i - (i / W) * W;
        xr[i] = xb[(size_t)wrap_idx(y0 - 1 + r, H) * W + c];
    }
    for (int i = tid; i < 9 * C0; i += 256) {
        const int co = i / 9, k = i - (i / 9) * 9;  // w0 packed [co][kpad], k = tap (Cin = 1)
        w[k * C0 + co] = w0[(size_t)co * kpad + k];
    }
    const float* bb = ct.bias_img ? cond_bias_row(ct, b, Bimg, cfg, C0) : bias_b + (size_t)b * C0;
    for (int c = tid; c < C0; c += 256) {
        bs[c] = bb[c];
        sc[c] = tsc[(size_t)b * C0 + c];
        sh[c] = tsh[(size_t)b * C0 + c];
    }
    __syncthreads();
    const int G8 = C0 / 8;
    char* dst = y + ((size_t)b * HW + p0) * C0 * 4;
    bool bad = false;
    for (int item = tid; item < fpx * G8; item += 256) {
        const int pl = item / G8, g = item - (item / G8) * G8;
        const int p = p0 + pl;
        const int yy = p / W, xx = p - (p / W) * W;
        const int ry = yy - y0;  // staged row of (yy - 1) is ry
        float xv[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) xv[dy * 3 + dx] = xr[(ry + dy) * W + wrap_idx(xx + dx - 1, W)];
        float4 a0 = *reinterpret_cast<const float4*>(bs + 8 * g);
        float4 a1 = *reinterpret_cast<const float4*>(bs + 8 * g + 4);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float4 u = *reinterpret_cast<const float4*>(w + k * C0 + 8 * g);
            const float4 v = *reinterpret_cast<const float4*>(w + k * C0 + 8 * g + 4);
            a0.x = fmaf(u.x, xv[k], a0.x); a0.y = fmaf(u.y, xv[k], a0.y);
            a0.z = fmaf(u.z, xv[k], a0.z); a0.w = fmaf(u.w, xv[k], a0.w);
            a1.x = fmaf(v.x, xv[k], a1.x); a1.y = fmaf(v.y, xv[k], a1.y);
            a1.z = fmaf(v.z, xv[k], a1.z); a1.w = fmaf(v.w, xv[k], a1.w);
        }
        const float4 s0 = *reinterpret_cast<const float4*>(sc + 8 * g);
        const float4 s1 = *reinterpret_cast<const float4*>(sc + 8 * g + 4);
        const float4 t0 = *reinterpret_cast<const float4*>(sh + 8 * g);
        const float4 t1 = *reinterpret_cast<const float4*>(sh + 8 * g + 4);
        auto sl = [](float v, float scl, float shf) {
            const float q = fmaf(v, scl, shf);
            return q * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * q));
        };
        const float4 o0 = make_float4(sl(a0.x, s0.x, t0.x), sl(a0.y, s0.y, t0.y), sl(a0.z, s0.z, t0.z),
                                      sl(a0.w, s0.w, t0.w));
        const float4 o1 = make_float4(sl(a1.x, s1.x, t1.x), sl(a1.y, s1.y, t1.y), sl(a1.z, s1.z, t1.z),
                                      sl(a1.w, s1.w, t1.w));
        uint2 hi0, lo0, hi1, lo1;
        split4x(o0, hi0, lo0, bf != 0);
        split4x(o1, hi1, lo1, bf != 0);
        if (!bf)
            bad = bad || h2_bad(o0.x) || h2_bad(o0.y) || h2_bad(o0.z) || h2_bad(o0.w) || h2_bad(o1.x) ||
                  h2_bad(o1.y) || h2_bad(o1.z) || h2_bad(o1.w);
        if (bf == 2) {  // 2-byte bf16 (h2.hpp "b2"): the hi halves only
            *reinterpret_cast<uint4*>(y + (((size_t)b * HW + p) * C0 + 8 * g) * 2) = make_uint4(hi0.x, hi0.y, hi1.x, hi1.y);
        } else {
            char* gp = dst + (size_t)pl * C0 * 4 + 32 * g;
            *reinterpret_cast<uint4*>(gp) = make_uint4(hi0.x, hi0.y, hi1.x, hi1.y);
            *reinterpret_cast<uint4*>(gp + 16) = make_uint4(lo0.x, lo0.y, lo1.x, lo1.y);
        }
    }
    h2_flag(ovf, bad);
}

// k_conv_first_rec at the 64^2 U-Net's shape (C0 = 96, W = 64, FR_PX pixels per workgroup, h2 records): the
// generic kernel's record loop spends half of its ~315 VALU per record on decoding the item (item / G8,
// p / W, three wrap_idx, the addresses of 9 x reads and 24 table reads) and is VALU-issue bound.  Here a
// thread's items tid + 256 k advance by 4 groups (mod 12) and 21 pixels plus the carry, so the loop holds no
// division or multiply; a wrapped column is an & 63 and every LDS read of a record is one of four bases
// plus an immediate.  The same fmaf chains in the same order on the same values: bit-identical records
// and range flag.
__global__ __launch_bounds__(256) void k_conv_first_rec96(const float* __restrict__ x, int bmod, int H,
                                                          const float* __restrict__ w0, int kpad,
                                                          const float* __restrict__ bias_b, char* __restrict__ y,
                                                          CondTab ct, int Bimg, int cfg, const float* __restrict__ tsc,
                                                          const float* __restrict__ tsh, unsigned* ovf) {
    constexpr int C0 = 96, W = 64, G8 = C0 / 8, NR = FR_PX / W + 2;
    static_assert(NR * W == 256 && (FR_PX * G8) % 256 == 0 && 256 % G8 == 4, "item stride of the record loop");
    __shared__ __attribute__((aligned(16))) float fr[12 * C0 + NR * W];  // w[9][C0] | bias | sc | sh | xr[NR][W]
    float* w = fr;
    float* bs = w + 9 * C0;
    float* sc = bs + C0;
    float* sh = sc + C0;
    float* xr = sh + C0;
    const int HW = H * W;
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * FR_PX;
    const int y0 = p0 / W;
    const float* xb = x + (size_t)(b % bmod) * HW;
    xr[tid] = xb[(size_t)wrap_idx(y0 - 1 + (tid >> 6), H) * W + (tid & (W - 1))];
    for (int i = tid; i < 9 * C0; i += 256) {
        const int co = i / 9, k = i - (i / 9) * 9;
        w[k * C0 + co] = w0[(size_t)co * kpad + k];
    }
    const float* bb = ct.bias_img ? cond_bias_row(ct, b, Bimg, cfg, C0) : bias_b + (size_t)b * C0;
    if (tid < C0) {
        bs[tid] = bb[tid];
        sc[tid] = tsc[(size_t)b * C0 + tid];
        sh[tid] = tsh[(size_t)b * C0 + tid];
    }
    __syncthreads();
    int g = tid % G8, pl = tid / G8;  // item = pl * G8 + g
    int wo = 8 * g;                   // the group's column of w / bias / sc / sh
    char* gp = y + ((size_t)b * HW + p0) * C0 * 4 + (size_t)tid * 32;
    bool bad = false;
#pragma unroll 1
    for (int it = 0; it < FR_PX * G8 / 256; ++it) {
        const int xx = pl & (W - 1), rb = pl - xx;  // pl = ry * W + xx: staged rows ry .. ry + 2
        const float* xc = xr + pl;
        const float* xl = xr + rb + ((xx - 1) & (W - 1));
        const float* xn = xr + rb + ((xx + 1) & (W - 1));
        float xv[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            xv[dy * 3 + 0] = xl[dy * W];
            xv[dy * 3 + 1] = xc[dy * W];
            xv[dy * 3 + 2] = xn[dy * W];
        }
        const float* wg = fr + wo;
        float4 a0 = *reinterpret_cast<const float4*>(wg + 9 * C0);
        float4 a1 = *reinterpret_cast<const float4*>(wg + 9 * C0 + 4);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float4 u = *reinterpret_cast<const float4*>(wg + k * C0);
            const float4 v = *reinterpret_cast<const float4*>(wg + k * C0 + 4);
            a0.x = fmaf(u.x, xv[k], a0.x); a0.y = fmaf(u.y, xv[k], a0.y);
            a0.z = fmaf(u.z, xv[k], a0.z); a0.w = fmaf(u.w, xv[k], a0.w);
            a1.x = fmaf(v.x, xv[k], a1.x); a1.y = fmaf(v.y, xv[k], a1.y);
            a1.z = fmaf(v.z, xv[k], a1.z); a1.w = fmaf(v.w, xv[k], a1.w);
            // opaque registers (no instruction) end the SLP tree here: packed, the chains became 36 v_pk_fma_f32
            // (two issue slots each) fed by ~70 v_mov that gather their operand pairs
            asm volatile("" : "+v"(a0.x), "+v"(a0.y), "+v"(a0.z), "+v"(a0.w), "+v"(a1.x), "+v"(a1.y), "+v"(a1.z), "+v"(a1.w));
        }
        const float4 s0 = *reinterpret_cast<const float4*>(wg + 10 * C0);
        const float4 s1 = *reinterpret_cast<const float4*>(wg + 10 * C0 + 4);
        const float4 t0 = *reinterpret_cast<const float4*>(wg + 11 * C0);
        const float4 t1 = *reinterpret_cast<const float4*>(wg + 11 * C0 + 4);
        auto sl = [](float v, float scl, float shf) {
            const float q = fmaf(v, scl, shf);
            return q * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * q));
        };
        const float4 o0 = make_float4(sl(a0.x, s0.x, t0.x), sl(a0.y, s0.y, t0.y), sl(a0.z, s0.z, t0.z),
                                      sl(a0.w, s0.w, t0.w));
        const float4 o1 = make_float4(sl(a1.x, s1.x, t1.x), sl(a1.y, s1.y, t1.y), sl(a1.z, s1.z, t1.z),
                                      sl(a1.w, s1.w, t1.w));
        uint2 hi0, lo0, hi1, lo1;
        split4x(o0, hi0, lo0, false);
        split4x(o1, hi1, lo1, false);
        bad = bad || h2_bad(o0.x) || h2_bad(o0.y) || h2_bad(o0.z) || h2_bad(o0.w) || h2_bad(o1.x) || h2_bad(o1.y) ||
              h2_bad(o1.z) || h2_bad(o1.w);
        *reinterpret_cast<uint4*>(gp) = make_uint4(hi0.x, hi0.y, hi1.x, hi1.y);
        *reinterpret_cast<uint4*>(gp + 16) = make_uint4(lo0.x, lo0.y, lo1.x, lo1.y);
        gp += 256 * 32;  // item + 256 = (pl + 21) * 12 + g + 4
        g += 4;
        pl += 21;
        wo += 32;
        if (g >= G8) {
            g -= G8;
            pl += 1;
            wo -= 8 * G8;
        }
    }
    h2_flag(ovf, bad);
}

}  // namespace

// x_t channel only, maps folded into bias0 (the conv bias is inside bias0).
// Split path (round 3): statistics pass + a second pass that recomputes the conv and writes
// silu(GroupNorm_0(.)) as down1.net.3's h2 / bf16 record (k_first_acf + k_first_gnsum, then a record kernel), so
// norm 0 needs neither a prologue nor an apply pass and the fp32 tensor is never written: *first_fused.  The
// record first conv beats the fp32 tensor + prologue form (r03_y).
int first_conv(const tcx_unet* net, const Plan& P, const float* x, int B, int cfg, const CondRows& ct, const H2Ctx& h2,
               hipStream_t st, int* ns, bool* first_fused) {
    const int Bt = P.Bt, H = P.H, W = P.W, C = P.C, fmt = h2.fmt;
    double* gn = P.gn;
    const tcx_conv& c0 = net->down1_0;
    const CondTab ctk{ct};
    *first_fused = false;
    if ((H * W) % FIRST_PX == 0 && C % 16 == 0 && C <= 128 && c0.kpad == 32) {
        const size_t shm = ((size_t)FIRST_PX * (C + 4) + 9 * (size_t)C) * sizeof(float) +
                           8 * (size_t)C * sizeof(double);
        // b2 (fmt 2) tensors are written only by the tile-free record kernel: a shape that would reach
        // k_conv_first<2> (4-byte records) or the fp32 first conv with fmt 2 fails here, loudly
        TCX_REQUIRE(fmt != 2 || (h2.on && (H * W) % FIRST_ACF_PX == 0 && C % 8 == 0 &&
                                 (H * W) % FR_PX == 0 && (FR_PX % W == 0 || W % FR_PX == 0)),
                    "tcx_unet: the 2-byte bf16 format needs the record first conv (H*W %% %d, W vs %d)", FR_PX, FR_PX);
        if (h2.on && (H * W) % FIRST_ACF_PX == 0 && C % 8 == 0) {
            const int chunk = FIRST_ACF_PX;
            const int nchunk = H * W / chunk;
            double* acf = gn + (size_t)Bt * C * 2;  // the autocorrelation partials, past the [Bt][1][C][2] sums
            hipLaunchKernelGGL(k_first_acf, dim3(nchunk, std::min(Bt, B)), dim3(256), 0, st, x, B, H, W, chunk, acf);
            TCX_TRY(check_launch("k_first_acf"));
            hipLaunchKernelGGL(k_first_gnsum, dim3(Bt), dim3(256), 0, st, acf, nchunk, H * W, C, c0.w, c0.kpad,
                               P.bias0, ctk, B, cfg, gn);
            TCX_TRY(check_launch("k_first_gnsum"));
            *ns = 1;
            TCX_TRY(gn_tab(net, P, 0, P.P0, C, gn, *ns, st));
            // tile-free record kernel (r03_af: 143 -> 114 us at 64^2); the LDS-tile form for other shapes
            if ((H * W) % FR_PX == 0 && (FR_PX % W == 0 || W % FR_PX == 0)) {
                static const int fr_env = env_int("TCX_FR_PX", FR_PX_WIDE);  // pixels per block at W >= 256 (A/B)
                const bool fr_ok = fr_env >= FR_PX && fr_env <= 4096 && (fr_env & (fr_env - 1)) == 0;
                const int fr_wide = fr_ok ? fr_env : FR_PX_WIDE;
                const int fpx = (W >= 256 && (H * W) % fr_wide == 0 && fr_wide % W == 0) ? fr_wide : FR_PX;
                const int nrow = (fpx >= W ? fpx / W : 1) + 2;
                const size_t shr = ((size_t)12 * C + (size_t)nrow * W) * sizeof(float);
                if (C == 96 && W == 64 && fpx == FR_PX && fmt == 0 && !(pass_forms() & 1))
                    hipLaunchKernelGGL(k_conv_first_rec96, dim3(H * W / FR_PX, Bt), dim3(256), 0, st, x, B, H, c0.w,
                                       c0.kpad, P.bias0, (char*)P.a64, ctk, B, cfg, P.sc(0), P.sh(0), h2.ovf);
                else
                    hipLaunchKernelGGL(k_conv_first_rec, dim3(H * W / fpx, Bt), dim3(256), shr, st, x, B, H, W, C,
                                       c0.w, c0.kpad, P.bias0, (char*)P.a64, ctk, B, cfg, P.sc(0), P.sh(0), h2.ovf,
                                       fmt, fpx);
            } else {
                hipLaunchKernelGGL(k_conv_first<2>, dim3(H * W / FIRST_PX, Bt), dim3(256), shm, st, x, B, H, W,
                                   C, c0.w, c0.kpad, P.bias0, P.a64, nullptr, ctk, B, cfg, P.sc(0), P.sh(0),
                                   h2.ovf, h2.bf ? 1 : 0);
            }
            TCX_TRY(check_launch("k_conv_first (GroupNorm+SiLU records)"));
            *first_fused = true;
        } else {
            hipLaunchKernelGGL(k_conv_first<0>, dim3(H * W / FIRST_PX, Bt), dim3(256), shm, st, x, B, H, W, C,
                               c0.w, c0.kpad, P.bias0, P.a64, gn, ctk, B, cfg, nullptr, nullptr, nullptr, 0);
            TCX_TRY(check_launch("k_conv_first"));
            *ns = H * W / FIRST_PX;
        }
    } else {
        TCX_REQUIRE(fmt != 2, "tcx_unet: the 2-byte bf16 format needs the record first conv");
        if (ct.bias_img) TCX_TRY(launch_fold_bias(ct, C, B, cfg, Bt, P.bias0, st));
        TCX_TRY(tcx_conv2d(x, nullptr, Bt, B, H, W, 1, 0, c0.w, nullptr, P.bias0, nullptr, P.a64, c0.cout,
                           c0.cout_pad, c0.kpad, 3, 1, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, st));
        *ns = std::max(1, H * W / 512);
        TCX_TRY(tcx_gn_partials(P.a64, Bt, H * W, C, *ns, gn, st));
    }
    return TCX_OK;
}

}  // namespace tcx
