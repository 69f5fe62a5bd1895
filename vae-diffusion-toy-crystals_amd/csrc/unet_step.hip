// Philox4x32-10 noise and the sampler step of CondUNetTiny's samplers (the reference's sde_score_model.py:507-569
// reverse SDE, :452-504 PF-ODE):
//   k_step — the out conv's 9-tap circular gather of the head partials r + bias, the CFG combine
//            eps_u + s (eps_c - eps_u), and the sampler update (EM / Heun stage / final x0 projection, or a
//            DPM-Solver++(2M) step, which the reference does not have) in one pass; noise either host-injected
//            or Philox in-kernel.
#include "unet.hpp"

namespace tcx {
namespace {

// ---------------------------------------------------------------- Philox4x32-10
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// N(0,1) for element `idx` of draw stream `sid` (Box-Muller on the first two Philox words).
__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t sid, uint64_t idx) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)sid, (uint32_t)(sid >> 32)};
    philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)c[0] + 1.0f) * 2.3283064365386963e-10f;  // (0, 1]
    const float u2 = (float)c[1] * 2.3283064365386963e-10f;
    return sqrtf(-2.0f * logf(u1)) * cosf(kTwoPi * u2);
}

__global__ void k_randn(float* out, size_t n, uint64_t seed, uint64_t sid, uint64_t e_off) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = philox_normal(seed, sid, e_off + i);
}

__device__ __forceinline__ float gather_eps(const float* __restrict__ rb, int HW, int W, int H, int y, int x,
                                            float ob) {
    // out[p] = b + sum_{dy,dx} r[tap=(dy*3+dx)][wrap(y+dy-1), wrap(x+dx-1)]
    float s = ob;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = wrap_idx(y + dy - 1, H);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xx = wrap_idx(x + dx - 1, W);
            s += rb[(size_t)(dy * 3 + dx) * HW + yy * W + xx];
        }
    }
    return s;
}

__global__ __launch_bounds__(256) void k_step(StepArgs a) {
    const int HW = a.H * a.W;
    const size_t n = (size_t)a.B * HW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / HW);
        const int p = (int)(i - (size_t)b * HW);
        const int y = p / a.W, x = p - (p / a.W) * a.W;
        float eps;
        if (a.cfg) {
            const float eu = gather_eps(a.r + (size_t)b * 9 * HW, HW, a.W, a.H, y, x, a.out_b);
            const float ec = gather_eps(a.r + (size_t)(a.B + b) * 9 * HW, HW, a.W, a.H, y, x, a.out_b);
            eps = eu + a.guidance * (ec - eu);
        } else {
            eps = gather_eps(a.r + (size_t)b * 9 * HW, HW, a.W, a.H, y, x, a.out_b);
        }
        if (a.mode == 0) {
            a.eps_out[i] = eps;
        } else if (a.mode == 1) {
            // reverse-SDE EM (sde_score_model.py:548-559)
            const float dt = a.scal[2], beta = a.scal[3], sigma = a.scal[4], g = a.scal[5], sq = a.scal[6];
            const float xv = a.x_inout[i];
            const float score = -eps / sigma;
            const float drift = ((-0.5f * beta) * xv) - (beta * score);
            const float z = a.z ? a.z[i] : philox_normal(a.seed, a.step + 1, a.e0 + i);
            a.x_inout[i] = (xv + drift * dt) + (g * sq) * z;
        } else if (a.mode == 2 || a.mode == 5) {
            // final projection (sde_score_model.py:562-569); mode 5 stops at x0_hat (:566), before
            // the (x0 + 1) / 2 map and the clamp (parity reads of the unsaturated trajectory)
            const float sigma = a.scal[4], alpha = a.scal[7];
            const float x0 = (a.x[i] - sigma * eps) / fmaxf(alpha, 1e-6f);
            const float v = (x0 + 1.0f) * 0.5f;
            a.eps_out[i] = a.mode == 5 ? x0 : fminf(fmaxf(v, 0.f), 1.f);
        } else if (a.mode == 3) {
            // Heun stage 1: d = -0.5 b x - 0.5 b score; x_e = x + d dt (sde_score_model.py:444-449,490-491)
            const float dt = a.scal[2], beta = a.scal[3], sigma = a.scal[4];
            const float xv = a.x_inout[i];
            const float score = -eps / sigma;
            const float d = ((-0.5f * beta) * xv) - ((0.5f * beta) * score);
            a.eps_out[i] = d;
            a.x2[i] = xv + d * dt;
        } else if (a.mode >= 6) {
            // DPM-Solver++(2M) step (Lu et al. 2022, Algorithm 2; tcx.h: tcx_dpmpp_sample): mode 6 first order
            // (writes the history), mode 7 second order (reads and rewrites it)
            const float sigma = a.coef[0], alpha = a.coef[1], cx = a.coef[2], cd = a.coef[3];
            const float xv = a.x_inout[i];
            const float x0 = (xv - sigma * eps) / alpha;
            const float D = a.mode == 7 ? (a.coef[4] * x0) + (a.coef[5] * a.hist[i]) : x0;
            a.hist[i] = x0;
            a.x_inout[i] = (cx * xv) + (cd * D);
        } else {
            // Heun stage 2 at t_next on x_e: x += 0.5 (d + d_next) dt  (sde_score_model.py:492-493)
            const float dt = a.scal[2];
            const float beta = a.scal[TCX_SCAL + 3], sigma = a.scal[TCX_SCAL + 4];
            const float xe = a.x[i];
            const float score = -eps / sigma;
            const float dn = ((-0.5f * beta) * xe) - ((0.5f * beta) * score);
            a.x_inout[i] = a.x_inout[i] + (0.5f * (a.eps_out[i] + dn)) * dt;
        }
    }
}

}  // namespace

int launch_step(const StepFields& a, hipStream_t st) {
    const size_t n = (size_t)a.B * a.H * a.W;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 16384);
    hipLaunchKernelGGL(k_step, dim3(blocks), dim3(256), 0, st, StepArgs{a});
    return check_launch("k_step");
}

}  // namespace tcx

using namespace tcx;

extern "C" int tcx_randn_at(float* out, size_t n, uint64_t seed, uint64_t stream_id, uint64_t e_off, void* stream) {
    TCX_REQUIRE(out, "tcx_randn: null pointer");
    if (n == 0) return TCX_OK;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_randn, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, n, seed, stream_id, e_off);
    return check_launch("tcx_randn");
}

extern "C" int tcx_randn(float* out, size_t n, uint64_t seed, uint64_t stream_id, void* stream) {
    return tcx_randn_at(out, n, seed, stream_id, 0, stream);
}
