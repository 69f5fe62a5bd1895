// Split-precision self-attention of SelfAttention2d (sde_score_model.py:136-167) at the WIDE head dims 80, 96 and
// 128 (base_ch 160 / 192 / 256 at four heads), for ANY token count N >= 1: qkv and out in the three storage
// formats of attention_split.hip (h2.hpp), which k_attention_split and k_attention_split_ragged serve only up to
// head dim 64.
//   FMT 0  h2 records, three v_mfma_f32_32x32x16_f16 per product (hi lo + lo hi + hi hi, f32 accumulation)
//   FMT 1  bf16 records, one v_mfma_f32_32x32x16_bf16 of the hi halves; the output with both halves
//   FMT 2  2-byte bf16 qkv and out
// The register scheme is k_attention_split's, which store4_h2x / store4_b2 and the gates of tests/attn_ref.py
// assume:
//   S^T = K Q^T : A = K rows from LDS (key on the lane, the 8 dims of step s on lane half h), B = Q^T
//                 fragments in registers (query on the lane);
//   P           : the S accumulators (keys (r&3) + 8(r>>2) + 4h of the 32-key tile) are exponentiated, scaled by
//                 2^10 and split (f16 hi + lo) or rounded (bf16); register 8s+e is k-slot 8h+e of the tile's
//                 16-key step s;
//   O^T = V^T P^T: A = V^T staged TRANSPOSED as [d][slot] rows with the keys in that slot order
//                 (slot 16s+8h+e <-> key 16s+8(e>>2)+4h+(e&3)), so a lane's eight slots are one b128 read.
// Its own: the split, the staging and the tails.
//   budget   at D = 128 in h2 a lane keeps 64 registers of Q fragments (hi + lo) and 64 of O^T accumulators for
//            the whole kernel.  The 64-key tile of k_attention_split_ragged would add 32 score registers and a
//            70 KB stage (two stages: 140 KB, one workgroup per CU).  So ONE 32-key score tile is live at a time
//            and a stage is 32 K rows + DP V^T rows of 32 slots: 37,376 B at D = 128 in h2, 74,752 B for the two
//            stages, two workgroups per CU; the bf16 forms take half of that (no lo plane, K rows of hi pieces).
//   split    grid (ceil(N/128), heads, Bt), 4 waves x 32 queries; every wave reads the same staged tile.  A tile
//            is D/16 score steps and 2 ceil(D/32) PV steps of 3 (h2) or 1 (bf16) MFMAs: 48 at D = 128 in h2.
//   staging  32-key tiles in two LDS stages: K rows copied (bf16 forms: the hi pieces only), V transposed with
//            b32 writes (two keys per dword).  The global loads of tile t+1 go to registers BEFORE the MFMAs of
//            tile t and to the other stage after them; one barrier per tile (a stage is rewritten only after
//            the barrier that ends the iteration that read it).  K rows are D*4 (h2) or D*2 (bf16) bytes + 16,
//            V^T rows 80 B: both strides are an odd number of 16-B units, so the b128 row reads (one row per
//            lane) are conflict-free.  A thread's V item is a key pair x 8 dims, the 16 key pairs fastest over
//            the threads, so a 32-lane half holds two dim groups whose rows lie 8 x 20 = 160 dwords = 0 banks
//            (mod 32) apart: the odd dim group writes its rows rotated by four (row e ^ 4 in write i = e), which
//            puts its 16 dwords 80 = 16 banks (mod 32) beside the even group's 16: conflict-free.
//   d = 80   five 16-deep score steps and three 32-row O^T tiles (DP = 96).  V^T rows 80..95 of both stages are
//            written once and never staged over: zeros, and in the bf16 forms row 80 all ones, so O^T row 80
//            accumulates the row sum l of the rounded P on the MFMA (as at D = 16 and 48 in the siblings).  At
//            D = 96 and 128 there is no spare row: l sums the same rounded p in VALU (v_dot2c_f32_bf16), as at
//            D = 32 and 64 in the siblings.  Either way the bf16 output is a convex combination of V rows.
//   key tail only the last tile can be ragged; it is peeled, so the main loop has no masking VALU.  Its source
//            rows are clamped to N-1: nothing is read past the tensor and every staged K / V value is a real,
//            finite one (a dead slot's p is 0, and 0 x garbage could be NaN).  Only its ceil(rem/16) live PV
//            k-steps run (wave-uniform), and the scores of keys >= N are -inf before the row maximum:
//            p = exp2(-inf) = 0 exactly, also after the bf16 rounding.  Key 0 of every tile is live and sits in
//            lane half 0, so after the xor-32 exchange the tile maximum is finite.
//   deferred maximum (bf16 forms, as k_attention_split): the offset m moves only when a tile's maximum passes
//            it by more than defer2 log2 units.  First tile, peeled or not: m = -inf, (mt - m) = +inf passes
//            any threshold, m becomes the finite tile maximum and alpha = exp2(-inf) = 0 multiplies the zero
//            accumulators.
//   query tail lanes with q >= N compute on the clamped row N-1; only their stores are guarded.  No wave
//            leaves before the last barrier: every wave stages, whatever its queries.
// Fixed-order sums and no atomics: two runs are bit-equal.  The output is a convex combination of V rows, so
// |O| <= max|V|: no range flag, as tcx_attention_split.
#include "common.hpp"
#include "h2.hpp"

namespace tcx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));

constexpr int SQ = 128;  // queries per workgroup (4 waves x 32)
constexpr int SK = 32;   // keys per staged tile (one 32-key score tile, 2 PV k-steps of 16)

template <int D, int FMT>
struct SplitWide {
    static_assert(D == 80 || D == 96 || D == 128, "wide split attention: head dim 80, 96 or 128");
    static constexpr bool BF = FMT >= 1, B2 = FMT == 2;
    static constexpr int ESZ = B2 ? 2 : 4;          // bytes per element of qkv / out
    static constexpr int DS = D / 16;               // 16-deep steps of Q.K
    static constexpr int DT = (D + 31) / 32;        // 32-row tiles of O^T
    static constexpr int DP = DT * 32;
    // staged K row: the h2 pieces (D * 4 B) or the bf16 hi pieces (D * 2 B), + 16 B pad; V^T row: 32 slots +
    // 16 B pad.  Both strides are an odd number of 16-B units: conflict-free b128 row reads
    static constexpr int KSB = (BF ? D * 2 : D * 4) + 16;
    static constexpr int VSW = SK / 2 + 4;          // dwords per V^T row (two slots each)
    static_assert((KSB / 16) % 2 == 1 && (VSW / 4) % 2 == 1, "row strides: an odd number of 16-B units");
    static constexpr int VPL = BF ? 1 : 2;          // V^T planes: hi (and lo)
    static constexpr int STAGE = SK * KSB + VPL * DP * VSW * 4;   // bytes: K | V^T hi | V^T lo
    static constexpr size_t LDS = 2 * (size_t)STAGE;
    static constexpr int KPL = BF ? D / 8 : D / 4;  // 16-B pieces staged per K row
    static constexpr int KITEMS = SK * KPL;
    static constexpr int KI = (KITEMS + 255) / 256; // K pieces per thread (the stash guarded when ragged)
    static constexpr int VITEMS = (SK / 2) * (D / 8);   // (key pair, 8-dim group) items: at most one per thread
    static_assert(VITEMS <= 256, "one V item per thread");
    // bf16, D < DP (D = 80): V^T row D is all ones, so O^T row D accumulates the row sum of the rounded P
    static constexpr bool ONES = BF && DP > D;
};

// One 32-key tile against the wave's 32 queries.  TAIL: the peeled last tile with `rem` (1..32) live keys.
template <int D, int FMT, bool TAIL>
__device__ __forceinline__ void split_wide_tile(const char* __restrict__ Ks, const unsigned* __restrict__ Vh,
                                                const unsigned* __restrict__ Vl, const h8 (&qh)[D / 16],
                                                const h8 (&ql)[D / 16], int li, int lh, int rem, float scale2,
                                                float defer2, float& m, float& l, f32x16 (&oacc)[(D + 31) / 32]) {
    using G = SplitWide<D, FMT>;
    constexpr bool BF = G::BF, ONES = G::ONES;
    const int nks = TAIL ? (rem + 15) >> 4 : 2;   // live 16-key PV k-steps
    f32x16 sacc = (f32x16){};
    const char* kr = Ks + li * G::KSB;
#pragma unroll
    for (int s = 0; s < G::DS; ++s) {
        const h8 kh = *reinterpret_cast<const h8*>(kr + (2 * s + lh) * (BF ? 16 : 32));
        if constexpr (BF) {
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, kh), __builtin_bit_cast(bf8, qh[s]),
                                                           sacc, 0, 0, 0);
        } else {
            const h8 kl = *reinterpret_cast<const h8*>(kr + (2 * s + lh) * 32 + 16);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[s], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[s], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[s], sacc, 0, 0, 0);
        }
    }
    // two chains of eight, combined below (one 16-long chain stalls on VALU latency)
    float mx0 = -INFINITY, mx1 = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (TAIL && (r & 3) + 8 * (r >> 2) + 4 * lh >= rem) sacc[r] = -INFINITY;
        if (r & 1) mx1 = fmaxf(mx1, sacc[r]);
        else mx0 = fmaxf(mx0, sacc[r]);
    }
    float mt = fmaxf(mx0, mx1);
    mt = fmaxf(mt, __shfl_xor(mt, 32));   // finite: key 0 of the tile is live
    const float mn = BF ? ((mt - m) * scale2 > defer2 ? mt : m) : fmaxf(m, mt);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale2);   // 0 on the first tile (m = -inf)
    const float mb = fmaf(-mn, scale2, 10.f);   // + 10: p is produced pre-scaled by 2^10
    m = mn;
    // bf16: rescale only when some lane's offset moved (x 1 is exact)
    if (!BF || __builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int t = 0; t < G::DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
    }
    float lt = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (TAIL && s >= nks) continue;
        const int c0 = 8 * s + 4 * lh;   // dword of the lane's eight slots in a V^T row
        if constexpr (BF) {
            bf8 pb;
#pragma unroll
            for (int e = 0; e < 8; ++e)   // a masked key: exp2(-inf) = 0
                pb[e] = (__bf16)__builtin_amdgcn_exp2f(fmaf(sacc[8 * s + e], scale2, mb));
            // D = 96, 128 (no ONES row): l sums the ROUNDED p the MFMA multiplies, as the ONES row does, so the
            // output stays a convex combination of V rows (v_dot2c_f32_bf16 against packed ones)
            if constexpr (!ONES) {
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    bf2 pp, one;
                    pp[0] = pb[e];
                    pp[1] = pb[e + 1];
                    one[0] = one[1] = (__bf16)1.0f;
                    lt = __builtin_amdgcn_fdot2_f32_bf16(pp, one, lt, false);
                }
            }
#pragma unroll
            for (int t = 0; t < G::DT; ++t) {
                const h8 vh = *reinterpret_cast<const h8*>(&Vh[(t * 32 + li) * G::VSW + c0]);
                oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, vh), pb, oacc[t], 0, 0, 0);
            }
        } else {
            h8 ph, pl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = __builtin_amdgcn_exp2f(fmaf(sacc[8 * s + e], scale2, mb));
                lt += v;   // l, like the P operand, carries the 2^10 scale
                const _Float16 hh = (_Float16)v;
                ph[e] = hh;
                pl[e] = (_Float16)(v - (float)hh);
            }
#pragma unroll
            for (int t = 0; t < G::DT; ++t) {
                const h8 vh = *reinterpret_cast<const h8*>(&Vh[(t * 32 + li) * G::VSW + c0]);
                const h8 vl = *reinterpret_cast<const h8*>(&Vl[(t * 32 + li) * G::VSW + c0]);
                oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, oacc[t], 0, 0, 0);
                oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, oacc[t], 0, 0, 0);
                oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, oacc[t], 0, 0, 0);
            }
        }
    }
    if constexpr (!ONES) {
        lt += __shfl_xor(lt, 32);
        l = l * alpha + lt;
    }
}

// 2 waves per SIMD (two workgroups per CU): 256 registers per lane
template <int D, int FMT>
__global__ __launch_bounds__(256, 2) void k_attention_split_wide(const char* __restrict__ qkv, char* __restrict__ out,
                                                                 int N, int C, float scale2, float defer2) {
    using G = SplitWide<D, FMT>;
    constexpr bool BF = G::BF, B2 = G::B2, ONES = G::ONES;
    constexpr int ESZ = G::ESZ;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // stage 0 | stage 1
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x;
    const size_t rs = 3 * ESZ * (size_t)C;   // bytes per token row of qkv
    const char* base = qkv + (size_t)b * N * rs + (size_t)h * D * ESZ;   // the head's q columns of the image
    const int lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const unsigned last = (unsigned)N - 1u;
    const unsigned q = blockIdx.x * (unsigned)SQ + w * 32 + li;   // unsigned: below N + 127 < 2^32
    auto Vhb = [&](int st) { return reinterpret_cast<unsigned*>(smem + st * G::STAGE + SK * G::KSB); };
    auto Vlb = [&](int st) { return Vhb(st) + (BF ? 0 : G::DP * G::VSW); };   // bf16: no lo plane, never read
    // D = 80: the V^T rows 80..95 of both stages, never staged over: zero, or the ONES row.  Ahead of the Q loads:
    // with the Q fragments live around this loop <80, 0> went over its 256 registers (8 B of scratch)
    if (G::DP > D) {
        constexpr int PADW = (G::DP > D ? G::DP - D : 1) * G::VSW;
        for (int i = tid; i < 2 * G::VPL * PADW; i += 256) {
            const int st = i / (G::VPL * PADW), k = i - st * (G::VPL * PADW);
            const int pl = k / PADW, e = k - pl * PADW;
            (pl ? Vlb(st) : Vhb(st))[D * G::VSW + e] = (ONES && e < G::VSW) ? 0x3F803F80u : 0u;   // two bf16 ones
        }
    }
    h8 qh[G::DS], ql[G::DS];
    {
        const char* qr = base + (size_t)min(q, last) * rs;
#pragma unroll
        for (int s = 0; s < G::DS; ++s) {
            qh[s] = *reinterpret_cast<const h8*>(qr + (2 * s + lh) * 8 * ESZ);
            if constexpr (BF) ql[s] = qh[s];   // never read
            else ql[s] = *reinterpret_cast<const h8*>(qr + (2 * s + lh) * 32 + 16);
        }
    }
    // staging: thread `tid` owns K pieces tid, tid + 256, .. and V item tid of a tile; native vectors (arrays of
    // HIP's float4 / uint4 structs stayed in scratch in the sibling kernels)
    f4 kreg[G::KI];
    u4 vreg[4];   // key 2 jp: hi, lo; key 2 jp + 1: hi, lo
    const int vg = tid / (SK / 2), vjp = tid - vg * (SK / 2);
    // every thread loads: an item past the tile's last (D = 80, 96) re-reads the last one and is not stashed, so
    // no load sits under a branch
    const int vgl = min(vg, D / 8 - 1);
    auto fetch = [&](unsigned k0) __attribute__((always_inline)) {   // rows clamp to N-1 (the last tile only)
#pragma unroll
        for (int u = 0; u < G::KI; ++u) {
            const int i = min(tid + 256 * u, G::KITEMS - 1);
            const int j = i / G::KPL, pc = i - j * G::KPL;
            const char* src = base + (size_t)min(k0 + j, last) * rs + (size_t)C * ESZ;
            kreg[u] = *reinterpret_cast<const f4*>(src + ((BF && !B2) ? 2 * pc : pc) * 16);
        }
        const char* v0 = base + (size_t)min(k0 + 2 * vjp, last) * rs + (size_t)(2 * C) * ESZ + vgl * 8 * ESZ;
        const char* v1 = base + (size_t)min(k0 + 2 * vjp + 1, last) * rs + (size_t)(2 * C) * ESZ + vgl * 8 * ESZ;
        vreg[0] = *reinterpret_cast<const u4*>(v0);
        vreg[2] = *reinterpret_cast<const u4*>(v1);
        if constexpr (!BF) {
            vreg[1] = *reinterpret_cast<const u4*>(v0 + 16);
            vreg[3] = *reinterpret_cast<const u4*>(v1 + 16);
        }
    };
    auto stash = [&](int st) __attribute__((always_inline)) {
        char* Ks = smem + st * G::STAGE;
        unsigned* Vh = Vhb(st);
        unsigned* Vl = Vlb(st);
#pragma unroll
        for (int u = 0; u < G::KI; ++u) {
            const int i = tid + 256 * u;
            if (G::KITEMS % 256 == 0 || i < G::KITEMS) {
                const int j = i / G::KPL, pc = i - j * G::KPL;
                *reinterpret_cast<f4*>(Ks + j * G::KSB + pc * 16) = kreg[u];
            }
        }
        if (G::VITEMS == 256 || tid < G::VITEMS) {
            // slot of the even key j of the pair: j = 16s + 8(e>>2) + 4h + (e&3) -> 16s + 8h + e; key j + 1
            // takes slot + 1, the other half of the dword
            const int j = 2 * vjp, r16 = j & 15;
            const int slot = (j & 16) + 8 * ((r16 >> 2) & 1) + ((r16 & 3) | ((r16 >> 3) << 2));
            const int col = slot >> 1;
            // the odd dim group writes row e ^ 4 in write e (header: the bank rotation): its dim quads swapped
            const bool odd = vg & 1;
            const int rot = odd ? 4 : 0;
            auto swapped = [&](const u4 v) { return odd ? (u4){v[2], v[3], v[0], v[1]} : v; };
            const u4 a4 = swapped(vreg[0]), c4 = swapped(vreg[2]);
            u4 al4 = a4, cl4 = c4;
            if constexpr (!BF) {
                al4 = swapped(vreg[1]);
                cl4 = swapped(vreg[3]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int sh = 16 * (i & 1), row = vg * 8 + (i ^ rot);
                const unsigned a = (a4[i >> 1] >> sh) & 0xffffu, c = (c4[i >> 1] >> sh) & 0xffffu;
                Vh[row * G::VSW + col] = a | (c << 16);
                if constexpr (!BF) {
                    const unsigned al = (al4[i >> 1] >> sh) & 0xffffu, cl = (cl4[i >> 1] >> sh) & 0xffffu;
                    Vl[row * G::VSW + col] = al | (cl << 16);
                }
            }
        }
    };
    const unsigned nt = last / SK + 1;   // key tiles; the last has rem = N - (nt-1)*32 in 1..32 live keys
    fetch(0);
    stash(0);
    __syncthreads();
    f32x16 oacc[G::DT];
#pragma unroll
    for (int t = 0; t < G::DT; ++t) oacc[t] = (f32x16){};
    float m = -INFINITY, l = 0.f;
    for (unsigned t = 0; t + 1 < nt; ++t) {
        const int cur = t & 1;
        fetch((t + 1) * SK);
        __builtin_amdgcn_sched_barrier(0);   // keep every load ahead of the tile's MFMAs
        split_wide_tile<D, FMT, false>(smem + cur * G::STAGE, Vhb(cur), Vlb(cur), qh, ql, li, lh, SK, scale2, defer2, m,
                                       l, oacc);
        stash(cur ^ 1);
        __syncthreads();   // the other stage complete for the next iteration; cur free to be rewritten in it
    }
    {
        const int cur = (nt - 1) & 1;
        split_wide_tile<D, FMT, true>(smem + cur * G::STAGE, Vhb(cur), Vlb(cur), qh, ql, li, lh,
                                      (int)(N - (nt - 1) * SK), scale2, defer2, m, l, oacc);
    }
    if constexpr (ONES) {
        // row D of O^T: tile D / 32, register 4 ((D % 32) / 8) + (D % 4), held by lane half 0 (D % 8 == 0);
        // the other half takes it across the wave
        constexpr int TD = D / 32, RD = 4 * ((D % 32) / 8) + (D % 4);
        const float own = oacc[TD][RD];
        const float other = __shfl_xor(own, 32);
        l = lh == 0 ? own : other;
    }
    if (q >= (unsigned)N) return;   // after the last barrier and the last cross-lane exchange
    const float inv = 1.f / l;
#pragma unroll
    for (int t = 0; t < G::DT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = t * 32 + 8 * i + 4 * lh;
            if (d < D) {
                const float4 v = make_float4(oacc[t][4 * i] * inv, oacc[t][4 * i + 1] * inv, oacc[t][4 * i + 2] * inv,
                                             oacc[t][4 * i + 3] * inv);
                if constexpr (B2) store4_b2(out, ((size_t)b * N + q) * C, (h * D + d) >> 2, v);
                else store4_h2x(out, ((size_t)b * N + q) * C * 4, (h * D + d) >> 2, v, BF);
            }
        }
}

template <int D, int FMT>
int launch_split_wide(const void* qkv, void* out, int Bt, int N, int C, int heads, hipStream_t st) {
    using G = SplitWide<D, FMT>;
    // log2(e) / sqrt(D): the logits in exp2 units
    const float scale2 = (float)(1.0 / std::sqrt((double)D)) * 1.4426950408889634f;
    static bool attr_set = false;   // 73 KB at D = 128 in h2: above 64 KB dynamic LDS needs the explicit opt-in
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_split_wide<D, FMT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS) != hipSuccess) {
            set_error("tcx_attention_split_wide: cannot enable %zu B of dynamic LDS", G::LDS);
            return TCX_EHIP;
        }
        attr_set = true;
    }
    static const float defer2 = [] {   // TCX_ATTN_DEFER, as k_attention_split: 0 = the exact running maximum
        const char* e = getenv("TCX_ATTN_DEFER");
        return e ? std::max(0.f, std::min(16.f, (float)atof(e))) : 8.f;
    }();
    hipLaunchKernelGGL((k_attention_split_wide<D, FMT>), dim3((N - 1) / SQ + 1, heads, Bt), dim3(256), G::LDS, st,
                       (const char*)qkv, (char*)out, N, C, scale2, defer2);
    return check_launch("tcx_attention_split_wide");
}

}  // namespace
}  // namespace tcx

using namespace tcx;

extern "C" int tcx_attention_split_wide(const void* qkv, void* out, int fmt, int Bt, int N, int C, int heads,
                                        void* stream) {
    TCX_REQUIRE(qkv && out, "tcx_attention_split_wide: null pointer");
    TCX_REQUIRE(heads > 0 && C > 0 && C % heads == 0,
                "tcx_attention_split_wide: bad args (need heads > 0, C %% heads == 0)");
    TCX_REQUIRE(N > 0, "tcx_attention_split_wide: N must be >= 1");
    TCX_REQUIRE(fmt >= 0 && fmt <= 2,
                "tcx_attention_split_wide: fmt must be 0 (h2 records), 1 (bf16 records) or 2 (2-byte bf16)");
    TCX_REQUIRE(aligned16(qkv) && aligned16(out), "tcx_attention_split_wide: pointers must be 16-B aligned");
    TCX_REQUIRE(Bt >= 0 && Bt <= 65535, "tcx_attention_split_wide: Bt must be in [0, 65535] (one grid row per image)");
    TCX_REQUIRE(heads <= 65535, "tcx_attention_split_wide: heads must be in [1, 65535] (one grid row per head)");
    const int D = C / heads;
    if (!(D == 80 || D == 96 || D == 128)) {
        set_error("tcx_attention_split_wide: head dim %d unsupported (80, 96 or 128)", D);
        return TCX_EUNSUP;
    }
    if (Bt == 0) return TCX_OK;
    hipStream_t st = (hipStream_t)stream;
#define TCX_SW_D(D_)                                                                 \
    case D_:                                                                         \
        return fmt == 2 ? launch_split_wide<D_, 2>(qkv, out, Bt, N, C, heads, st)   \
             : fmt == 1 ? launch_split_wide<D_, 1>(qkv, out, Bt, N, C, heads, st)   \
                        : launch_split_wide<D_, 0>(qkv, out, Bt, N, C, heads, st);
    switch (D) {
        TCX_SW_D(80)
        TCX_SW_D(96)
        default:
        TCX_SW_D(128)
    }
#undef TCX_SW_D
}
