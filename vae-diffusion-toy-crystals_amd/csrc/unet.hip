// CondUNetTiny forward, natively (the reference's models/sde_score_model.py:170-266 forward, :402-423 CFG).
//
// Per U-Net evaluation the host issues ONE call (tcx_unet_eval); the samplers' loops (sampler.hip) are one
// call too, so no Python runs between kernels.  This unit is host code: the workspace plan of one pass, the
// body that enqueues a pass layer by layer, and the (possibly chunked) evaluation around it.  Its kernels
// live by stage: unet_cond.hip (conditioning -> first-conv bias), unet_first.hip (first conv), unet_head.hip
// (head partials r), unet_step.hip (out conv gather + CFG + sampler update); the convs, GroupNorm passes and
// attention are the library's own (conv*.hip, norm.hip, attention*.hip, attn_block.hip).
#include "conv_common.hpp"
#include "passes.hpp"
#include "unet.hpp"

namespace tcx {
namespace {

Plan make_plan(const tcx_unet* net, int Bt, int H, int W, char* base) {
    Plan p{};
    p.Bt = Bt; p.H = H; p.W = W;
    p.C = net->base_ch; p.C2 = 2 * net->base_ch;
    p.P0 = H * W; p.P1 = (H / 2) * (W / 2); p.P2 = (H / 4) * (W / 4);
    size_t off = 0;
    auto take = [&](size_t bytes) -> char* {
        char* ptr = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return ptr;
    };
    const size_t f = sizeof(float);
    p.bias0 = (float*)take((size_t)Bt * p.C * f);
    p.a64 = (float*)take((size_t)Bt * p.P0 * p.C * f);
    p.b64 = (float*)take((size_t)Bt * p.P0 * p.C * f);
    p.h1 = (float*)take((size_t)Bt * p.P0 * p.C * f);
    p.a32 = (float*)take((size_t)Bt * p.P1 * p.C2 * f);
    p.b32 = (float*)take((size_t)Bt * p.P1 * p.C2 * f);
    p.h2 = (float*)take((size_t)Bt * p.P1 * p.C2 * f);
    p.a16 = (float*)take((size_t)Bt * p.P2 * p.C2 * f);
    p.b16 = (float*)take((size_t)Bt * p.P2 * p.C2 * f);
    p.qkv = (float*)take((size_t)Bt * p.P2 * 3 * p.C2 * f);
    p.r = (float*)take((size_t)Bt * 9 * p.P0 * f);
    const int maxsplit = std::max(1, p.P0 / 128);
    p.gn = (double*)take((size_t)Bt * maxsplit * std::max(p.C2, 2 * p.C2) * 2 * sizeof(double));
    p.tab = (float*)take((size_t)22 * Bt * p.C2 * f);
    p.bytes = off;
    return p;
}

// One conv layer of the body.  Sources x1 (C1 channels) and, for a concat conv, x2 (C2); sc/sh{1,2}: fused
// GroupNorm+SiLU prologue tables of the sources (null: the source is already normalised).  gn: the GroupNorm
// partials of the output are wanted, *nsplit receives their split count (written in the conv's epilogue when
// the tile geometry allows it, else by the partials kernel afterwards).
struct ConvGn {
    const float *x1, *x2;
    int C1, C2, Bt, H, W, stride, pad;
    const float* resid;
    float* y;
    double* gn;
    int* nsplit;
    const float *sc1, *sh1, *sc2, *sh2;
    H2Ctx h2;
    int out_h2;
};

int conv_gn(const tcx_conv& cv, hipStream_t st, const ConvGn& a) {
    const int Ho = (a.H + 2 * a.pad - cv.ks) / a.stride + 1, Wo = (a.W + 2 * a.pad - cv.ks) / a.stride + 1;
    const int HoWo = Ho * Wo;
    const bool fused = a.gn && HoWo % 128 == 0;
    if (a.h2.on) {
        // split path: sc/sh tables here are the GroupNorm+SiLU prologue of k_conv3g (fp32 source)
        TCX_REQUIRE(cv.wh && cv.wscale, "tcx_unet: split path needs packed h2 weights");
        TCX_TRY(tcx_conv2d_h2_pro(a.x1, a.x2, a.Bt, 0, a.H, a.W, a.C1, a.C2, cv.wh, cv.whf, cv.wscale, cv.b, nullptr,
                                  a.resid, a.y, a.out_h2, cv.cout, cv.cout_pad, cv.kpad, cv.ks, a.stride, a.pad, 1, 0,
                                  fused ? a.gn : nullptr, a.sc1, a.sh1, a.sc2, a.sh2, a.h2.fmt, a.h2.ovf, st));
    } else {
        TCX_TRY(tcx_conv2d(a.x1, a.x2, a.Bt, 0, a.H, a.W, a.C1, a.C2, cv.w, cv.b, nullptr, a.resid, a.y, cv.cout,
                           cv.cout_pad, cv.kpad, cv.ks, a.stride, a.pad, 1, 0, 0, fused ? a.gn : nullptr, a.sc1, a.sh1,
                           a.sc2, a.sh2, st));
    }
    if (a.gn) {
        *a.nsplit = fused ? HoWo / 128 : std::max(1, HoWo / 512);
        if (!fused) TCX_TRY(tcx_gn_partials(a.y, a.Bt, HoWo, cv.cout, *a.nsplit, a.gn, st));
    }
    return TCX_OK;
}

// a skip tensor (H x W x C) can be chunk-major when both readers take it: the downsample on k_conv4s2g
// (fragment-ordered 4x4 weights, Wo in {16, 32, 64}) and the concat conv on k_conv3m (fragment-ordered 3x3
// weights, rows of 16 / 32 / 64 px, Cin = 2 C <= 384, Cout a multiple of 96), neither with a prologue
bool skip_cm_ok(const tcx_conv& ds, const tcx_conv& cat, int H, int W, int C) {
    return gn_apply_cm_ok(H * W, C) && ds.whf && cat.whf && ds.ks == 4 && cat.ks == 3 && H % 2 == 0 &&
           (W == 32 || W == 64) && (H * W / 4) % 128 == 0 && ds.cout_pad % 96 == 0 && 2 * C <= 384 &&
           C % 16 == 0 && cat.cout_pad % 96 == 0 && cat.cout % 96 == 0 && (H * W) % 256 == 0;
}

// config 5 (b2, round 6): a skip tensor can be chunk-major b2 planes when its downsample runs on k_conv4s2g's
// slim form and its concat conv on k_conv3lb (rows of 128 / 256 px), the apply pass tiles the image
bool skip_cm_b2_ok(const tcx_conv& ds, const tcx_conv& cat, int H, int W, int C) {
    return gn_apply_cm_ok(H * W, C) && ds.whf && cat.whf && ds.ks == 4 && cat.ks == 3 && H % 2 == 0 &&
           (W == 128 || W == 256) && (H * W / 4) % 128 == 0 && ds.cout_pad % 96 == 0 && C % 16 == 0 &&
           cat.cout_pad % 96 == 0 && (H * W) % 256 == 0;
}

// The U-Net body (everything up to and including the head partials r).  Input x [B][H][W] (C=1).
// GroupNorm+SiLU outputs are materialised once each (an apply pass), except where the consuming conv's
// staging prologue applies them from [Bt][C] scale/shift tables (tcx_gn_finalize; pro[] below); the
// statistics come from the producing conv's epilogue.
int unet_body(const tcx_unet* net, const Plan& P, const float* x, int B, const float* t, int t_per_sample,
              const int64_t* y_cat, const float* y_cont, int cfg, hipStream_t st, const CondRows& ct) {
    const int Bt = P.Bt, H = P.H, W = P.W, C = P.C, C2 = P.C2;
    const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4;
    // conditioning -> per-batch first-conv bias (sampler calls: rows precomputed once per call,
    // make_cond_maps, and read by the first conv itself)
    if (!ct.bias_img) TCX_TRY(launch_cond(net, t, t_per_sample, y_cat, y_cont, B, cfg, Bt, P.bias0, st));
    int ns = 1;
    double* gn = P.gn;
    // fp32 path: no prologue.  Measured (profiles/r01_*): on gfx950 fp32 MFMA shares the fp32 VALU rate, so a
    // SiLU recomputed for every im2col tap (9x per element) costs the conv ~25 %, more than the separate
    // HBM-bound GroupNorm pass it removes.  (The prologue stays in the ABI: tcx_conv2d pro_*.)
    // Split path: a GroupNorm+SiLU whose only consumer is a 3x3 conv on k_conv3g (rows of 16/32/64/128
    // pixels) is applied by that conv's halo staging from the fp32 tensor (tcx_conv2d_h2_pro), so the
    // normalised tensor is never written: norms 0, 2, 4, 7, 9 (down1.net.1, down2.net.1, mid.net.1,
    // up2.net.1, up1.net.1 feeding the .net.3 conv of their block; every GroupNorm as an apply pass instead
    // measured 2-3 % slower).  The skip tensors h1/h2 (norms 1, 3: read by a 4x4/s2 conv AND an up-path
    // concat) keep an apply pass.
    // Not for bf16 at rows of 64/128/256 pixels: the h2-source conv there is the LDS-DMA k_conv3lb, which has
    // no prologue form; an apply pass + k_conv3lb beats k_conv3g's register-staged prologue form, whose
    // transform (7 halo units per thread at 256-px rows, 3x redundant over the tiles of a row) is not
    // hidden behind a bf16 tap's 6 MFMAs (r03_y).
    bool pro[11] = {};
    auto pro_ok = [&](const tcx_conv& cv, int h, int w, int cin) {
        const bool bf = net->precision == 2;
        return cv.whf && conv3g_covers(h, w, cin, cv.cout_pad, bf) && !(bf && (w == 64 || w == 128 || w == 256));
    };
    if (net->precision >= 1) {
        pro[0] = pro_ok(net->down1_1, H, W, C);
        pro[2] = pro_ok(net->down2_1, H1, W1, C2);
        pro[7] = pro_ok(net->up2_1, H1, W1, C);
        pro[9] = pro_ok(net->up1_1, H, W, C);
        pro[4] = pro_ok(net->mid_1, H2, W2, C2);  // mid.net.1 -> mid.net.3
    }
    // split path: every conv source is h2 (h2.hpp) — GroupNorm applies feeding a conv write h2
    // in place, convs feeding only convs (ds1, ds2, us2, us1) write h2, the rest stay fp32
    // Config 5 (bf16 at 256^2): every conv there runs on an LDS-DMA kernel that reads 2-byte bf16 (k_conv3lb
    // at 256 / 128 / 64-px rows, k_conv4s2g's slim slots at Wo 128 / 64, k_lin1x1, the split attention), so
    // the tensors are 2-byte bf16 ("b2", h2.hpp) instead of 4-byte records whose lo halves a bf16 product never
    // reads, and the pre-GroupNorm conv outputs are bf16 too (the GroupNorm statistics are taken on the fp32
    // values in the conv epilogue; the apply pass normalises the stored bf16 in place, 2 B read + 2 B written
    // per element).  fp32 stays where a consumer needs it: the attention input / residual (mid_1) and up2_1's
    // output (the upsample applies its GroupNorm from fp32).  TCX_BF_B2=0 keeps the 4-byte records (A/B).
    static const bool b2_on = env_on("TCX_BF_B2");
    // TCX_SKIP_CM=0: the skip tensors h1 / h2 as pixel-major records (the in-place apply pass), A/B;
    // 1 / 2: h1 / h2 only chunk-major (default 3: both)
    static const int skip_cm_env = env_int("TCX_SKIP_CM", 3);
    const int skip_cm = (skip_cm_env >= 0 && skip_cm_env <= 3) ? skip_cm_env : 3;
    // TCX_ATTN_PREP=0: the attention input as four passes (apply, partials, finalize, apply) instead of
    // k_attn_prep (its statistics are summed in another fp64 order: not bit-identical; A/B and parity test)
    static const bool attn_prep_on = env_on("TCX_ATTN_PREP");
    // TCX_ATTN_SPLIT=0 keeps the split evaluator's attention on fp32 MFMA (A/B measurements)
    static const bool attn_split_on = env_on("TCX_ATTN_SPLIT");
    // TCX_ATTN_BLOCK=0: the bottleneck attention as three launches (qkv conv, k_attention_split, proj conv)
    // instead of k_attn_block + proj (bit-identical; A/B measurements and parity tests)
    static const bool attn_block_on = env_on("TCX_ATTN_BLOCK");
    const int fmt = net->precision == 2 ? ((b2_on && W == 256 && H % 4 == 0 && C == 96) ? 2 : 1) : 0;
    const H2Ctx h2{net->precision >= 1, net->h2_ovf, net->precision == 2, fmt};
    const int pre_b2 = fmt == 2 ? 1 : 0;  // out_h2 of a conv whose output only a GroupNorm apply reads
    // finalize the table of norm i, and normalise `y` in place unless a prologue consumes the table
    auto norm = [&](int i, float* y, int HW, int Cn, bool to_h2 = true) -> int {
        TCX_TRY(gn_tab(net, P, i, HW, Cn, gn, ns, st));
        if (pro[i]) return TCX_OK;
        if (h2.on && to_h2 && fmt == 2) return gn_apply_b2_inplace(y, Bt, HW, Cn, P.sc(i), P.sh(i), 1, st);
        if (h2.on && to_h2) return gn_apply_tab_h2(y, y, Bt, HW, Cn, P.sc(i), P.sh(i), 1, h2.ovf, h2.bf, st);
        return tcx_gn_apply_tab(y, y, Bt, HW, Cn, P.sc(i), P.sh(i), 1, st);
    };
    // a 3x3 / stride 1 conv layer at h x w from x1 (C1 channels) to y (out_h2: y's format, tcx_conv2d_h2_pro) in
    // the evaluation's format; the call sites below set what else their layer has.  with_gn: the output's
    // GroupNorm partials; with_pro: norm i applied by the conv's prologue on source 1 where pro[i] says so
    auto layer = [&](const float* x1, int C1, int h, int w, float* y, int out_h2 = 0) {
        ConvGn a{};
        a.x1 = x1; a.C1 = C1; a.Bt = Bt; a.H = h; a.W = w; a.stride = 1; a.pad = 1; a.y = y; a.h2 = h2; a.out_h2 = out_h2;
        return a;
    };
    auto with_gn = [&](ConvGn a) { a.gn = gn; a.nsplit = &ns; return a; };
    auto with_pro = [&](ConvGn a, int i) { if (pro[i]) { a.sc1 = P.sc(i); a.sh1 = P.sh(i); } return a; };
    // down1
    bool first_fused = false;
    TCX_TRY(first_conv(net, P, x, B, cfg, ct, h2, st, &ns, &first_fused));
    if (first_fused) pro[0] = false;
    else TCX_TRY(norm(0, P.a64, P.P0, C));
    // Chunk-major skip tensors (round 5, TCX_SKIP_CM=0 off): silu(gn(h1)) / silu(gn(h2)) are written as
    // [C/8][Bt*HW][32 B] record planes (gn_apply_cm) for their two readers, the 4x4/s2 downsample (source 1,
    // whose halo DMA re-fetched pixel-major lines) and the up-path concat conv on k_conv3m (source 2).  The
    // raw conv output goes to a buffer that is free at that point (b64 / a32) and the apply writes h1 / h2.
    // (config 5, round 6: the b2 skip tensors as chunk-major b2 planes, gn_apply_b2cm, same readers' roles)
    const bool cm1 = h2.on && (skip_cm & 1) &&
                     ((fmt == 0 && skip_cm_ok(net->ds1, net->up1_0, H, W, C)) ||
                      (fmt == 2 && skip_cm_b2_ok(net->ds1, net->up1_0, H, W, C)));
    const bool cm2 = h2.on && (skip_cm & 2) &&
                     ((fmt == 0 && skip_cm_ok(net->ds2, net->up2_0, H1, W1, C2)) ||
                      (fmt == 2 && skip_cm_b2_ok(net->ds2, net->up2_0, H1, W1, C2)));
    auto apply_cm = [&](const float* raw, float* dst, int HWn, int Cn, int i) -> int {
        TCX_TRY(gn_tab(net, P, i, HWn, Cn, gn, ns, st));
        if (fmt == 2) return gn_apply_b2cm(raw, dst, Bt, HWn, Cn, P.sc(i), P.sh(i), st);
        return gn_apply_cm(raw, dst, Bt, HWn, Cn, P.sc(i), P.sh(i), h2.ovf, st);
    };
    // the 4x4 / stride 2 downsample of a skip tensor (source 1 chunk-major: format bit 16) and the up-path
    // concat conv of [x1, skip] (source 2 chunk-major: format bit 32)
    auto downsample = [&](const float* skip, int Cn, int h, int w, float* y, bool cm) {
        ConvGn a = layer(skip, Cn, h, w, y, 1);
        a.stride = 2; a.h2.fmt |= cm ? 16 : 0;
        return a;
    };
    auto concat = [&](const float* x1, const float* skip, int Cn, int h, int w, float* y, bool cm) {
        ConvGn a = with_gn(layer(x1, Cn, h, w, y, pre_b2));
        a.x2 = skip; a.C2 = Cn; a.h2.fmt |= cm ? 32 : 0;
        return a;
    };
    TCX_TRY(conv_gn(net->down1_1, st, with_pro(with_gn(layer(P.a64, C, H, W, cm1 ? P.b64 : P.h1, pre_b2)), 0)));
    if (cm1) TCX_TRY(apply_cm(P.b64, P.h1, P.P0, C, 1));
    else TCX_TRY(norm(1, P.h1, P.P0, C));
    // ds1: 4x4/s2 circular on silu(gn(h1))
    TCX_TRY(conv_gn(net->ds1, st, downsample(P.h1, C, H, W, P.a32, cm1)));
    // down2
    TCX_TRY(conv_gn(net->down2_0, st, with_gn(layer(P.a32, C, H1, W1, P.b32, pre_b2))));
    TCX_TRY(norm(2, P.b32, P.P1, C2));
    TCX_TRY(conv_gn(net->down2_1, st, with_pro(with_gn(layer(P.b32, C2, H1, W1, cm2 ? P.a32 : P.h2, pre_b2)), 2)));
    if (cm2) TCX_TRY(apply_cm(P.a32, P.h2, P.P1, C2, 3));
    else TCX_TRY(norm(3, P.h2, P.P1, C2));
    // ds2
    TCX_TRY(conv_gn(net->ds2, st, downsample(P.h2, C2, H1, W1, P.a16, cm2)));
    // mid
    TCX_TRY(conv_gn(net->mid_0, st, with_gn(layer(P.a16, C2, H2, W2, P.b16, pre_b2))));
    TCX_TRY(norm(4, P.b16, P.P2, C2));
    TCX_TRY(conv_gn(net->mid_1, st, with_pro(with_gn(layer(P.b16, C2, H2, W2, P.a16)), 4)));
    // the attention block needs the normalised tensor itself (input of attn.norm and residual): fp32
    TCX_TRY(gn_tab(net, P, 5, P.P2, C2, gn, ns, st));
    // attention: x_in = a16; b16 = GN(x_in); qkv = 1x1; b16 = attn; a16 = x_in + proj(b16)
    {
        if (h2.on && attn_prep_on && attn_prep_ok(P.P2, C2, groups_of(C2), fmt)) {
            // one pass per image: GN5+SiLU in place, attn.norm statistics, tables and h2 records (round 5)
            TCX_TRY(attn_prep_h2(P.a16, P.b16, Bt, P.P2, C2, P.sc(5), P.sh(5), net->gn_w[6], net->gn_b[6],
                                 groups_of(C2), h2.ovf, fmt, st));
        } else {
            TCX_TRY(tcx_gn_apply_tab(P.a16, P.a16, Bt, P.P2, C2, P.sc(5), P.sh(5), 1, st));
            const int ns_a = std::max(1, P.P2 / 256);
            TCX_TRY(tcx_gn_partials(P.a16, Bt, P.P2, C2, ns_a, gn, st));
            TCX_TRY(gn_tab(net, P, 6, P.P2, C2, gn, ns_a, st));
            if (h2.on) TCX_TRY(gn_apply_tab_h2(P.a16, P.b16, Bt, P.P2, C2, P.sc(6), P.sh(6), 0, h2.ovf, fmt, st));
            else TCX_TRY(tcx_gn_apply_tab(P.a16, P.b16, Bt, P.P2, C2, P.sc(6), P.sh(6), 0, st));
        }
        const tcx_conv& q = net->qkv;
        const tcx_conv& pr = net->proj;
        // split path with N % 256 == 0 and a supported head dim: the qkv conv writes h2 and the
        // attention runs on f16x3 MFMA (attention_split.hip); else fp32 qkv + fp32-MFMA attention
        const int D = C2 / net->heads;
        const bool split_attn = h2.on && attn_split_on && P.P2 % 256 == 0 && C2 % net->heads == 0 &&
                                (D == 16 || D == 32 || D == 48 || D == 64);
        // f16x3 at N = 256, C2 = 192, 4 heads: the qkv conv runs inside the attention workgroup
        // (attn_block.hip; its output goes to the free qkv buffer, since the heads of an image read b16
        // while others already write), then the proj launch as below
        if (h2.on && split_attn && attn_block_on &&
            attn_block_ok(fmt, Bt, P.P2, C2, net->heads, q, pr, P.b16, P.a16, P.qkv)) {
            TCX_TRY(tcx_attn_block_h2(P.b16, P.a16, P.qkv, q.wh, q.wscale, q.b, q.cout_pad, pr.wh, pr.wscale, pr.b,
                                      pr.cout_pad, Bt, P.P2, C2, net->heads, h2.ovf, st));
        } else {
            ConvGn qa = layer(P.b16, C2, H2, W2, P.qkv, split_attn ? 1 : 0);  // 1x1
            qa.pad = 0;
            TCX_TRY(conv_gn(q, st, qa));
            TCX_REQUIRE(split_attn || !h2.bf, "tcx_unet: bf16 precision needs the split attention (N %% 256 == 0)");
            if (split_attn) TCX_TRY(attention_split(P.qkv, P.b16, Bt, P.P2, C2, net->heads, fmt, st));
            else if (h2.on) TCX_TRY(tcx_attention_h2(P.qkv, P.b16, Bt, P.P2, C2, net->heads, h2.ovf, st));
            else TCX_TRY(tcx_attention(P.qkv, P.b16, Bt, P.P2, C2, net->heads, st));
            ConvGn pa = layer(P.b16, C2, H2, W2, P.a16);  // 1x1, + x_in
            pa.pad = 0; pa.resid = P.a16;
            TCX_TRY(conv_gn(pr, st, pa));
        }
    }
    // us2: bilinear x2 (edge-clamped) into the free b32 buffer, then the circular 3x3 conv -> a32.
    // (The upsample-on-load conv variant re-reads 4 source taps per im2col element and measured
    // slower than this separate 250 MB pass.)
    if (h2.on) TCX_TRY(upsample2x_h2(P.a16, P.b32, Bt, H2, W2, C2, nullptr, nullptr, h2.ovf, fmt, st));
    else TCX_TRY(tcx_upsample2x(P.a16, P.b32, Bt, H2, W2, C2, nullptr, nullptr, st));
    TCX_TRY(conv_gn(net->us2, st, layer(P.b32, C2, H1, W1, P.a32, 1)));
    // up2 on cat[a32, silu(gn(h2))]
    TCX_TRY(conv_gn(net->up2_0, st, concat(P.a32, P.h2, C2, H1, W1, P.b32, cm2)));
    TCX_TRY(norm(7, P.b32, P.P1, C));
    TCX_TRY(conv_gn(net->up2_1, st, with_pro(with_gn(layer(P.b32, C, H1, W1, P.a32)), 7)));
    // us1: GN+SiLU of up2's output, bilinear x2 into the free b64, conv.  Split path: the banded
    // upsample applies the GroupNorm+SiLU once per source element while staging (no apply pass);
    // fp32 path: the apply pass in place, then the plain upsample
    // (r03_o, one lane, alternating: 72.7 vs 72.3 images/s against the separate apply pass)
    if (h2.on && upsample_fused_ok(H1, W1, C)) {
        TCX_TRY(gn_tab(net, P, 8, P.P1, C, gn, ns, st));
        TCX_TRY(upsample2x_h2(P.a32, P.b64, Bt, H1, W1, C, P.sc(8), P.sh(8), h2.ovf, fmt, st));
    } else {
        TCX_TRY(norm(8, P.a32, P.P1, C, false));
        if (h2.on) TCX_TRY(upsample2x_h2(P.a32, P.b64, Bt, H1, W1, C, nullptr, nullptr, h2.ovf, fmt, st));
        else TCX_TRY(tcx_upsample2x(P.a32, P.b64, Bt, H1, W1, C, nullptr, nullptr, st));
    }
    TCX_TRY(conv_gn(net->us1, st, layer(P.b64, C, H, W, P.a64, 1)));
    // up1 on cat[a64, silu(gn(h1))]
    TCX_TRY(conv_gn(net->up1_0, st, concat(P.a64, P.h1, C, H, W, P.b64, cm1)));
    TCX_TRY(norm(9, P.b64, P.P0, C));
    // (b2: the head reads up1_1's output as bf16)
    TCX_TRY(conv_gn(net->up1_1, st, with_pro(with_gn(layer(P.b64, C, H, W, P.a64, pre_b2)), 9)));
    // head: GN(up1.net.4)+SiLU fused with the out conv's channel reduction
    TCX_TRY(gn_tab(net, P, 10, P.P0, C, gn, ns, st));
    return launch_head(net, P, fmt, st);
}

// Batch chunking: one evaluation of B images can run as ceil(B / Bc) passes of Bc images (2*Bc
// U-Net rows with CFG; per-image arithmetic unchanged: GroupNorm is per sample, CFG pairs stay in
// one pass, in-kernel noise is keyed by the global element index).  Meant to keep a pass's
// producer -> consumer hand-offs inside the 256 MB Infinity Cache; measured at B = 128
// (profiles/r01_w_chunk_ab.txt) it LOSES: 59.9 img/s unchunked vs 56.6 / 49.3 / 37.2 at
// Bc = 64 / 32 / 16 (the smaller conv grids lose more than the memory-bound passes gain), so the
// default is one pass (the chunking knob was removed in round 3).
// A pass is capped so that its largest activation (2*Bc*H*W*C fp32)
// stays below 2 GiB: the conv kernels address their operands with 32-bit buffer offsets (the
// 256x256 configuration at base_ch 96: at most 84 images, i.e. 2*42 with CFG, per pass).
int max_pass_rows(const tcx_unet* net, int H, int W) {
    const long long per_row = (long long)H * W * net->base_ch * 4;
    const long long rows = ((1ll << 31) - 1) / per_row;
    return (int)std::max(2ll, rows & ~1ll);
}

int chunk_images(int B, int cap_images) { return std::max(1, std::min(B, cap_images)); }

// workspace of one evaluation of Bt = B or 2B (CFG) rows: sized for the largest pass of either reading
size_t single_ws_bytes(const tcx_unet* net, int Bt, int H, int W) {
    const int cap = max_pass_rows(net, H, W);
    const int Btc = std::min(std::min(Bt, 2 * chunk_images(Bt, cap)), cap);
    return make_plan(net, Btc, H, W, nullptr).bytes + 256;
}

}  // namespace

int validate(const tcx_unet* net, int B, int H, int W) {
    TCX_REQUIRE(net, "tcx_unet: null net");
    TCX_REQUIRE(B > 0 && H % 4 == 0 && W % 4 == 0 && H >= 8 && W >= 8, "tcx_unet: need B>0 and H,W multiples of 4 (>=8)");
    TCX_REQUIRE(net->base_ch % 4 == 0 && net->base_ch >= 4, "tcx_unet: base_ch must be a multiple of 4");
    TCX_REQUIRE(net->emb_dim <= 256 && net->emb_dim % 2 == 0, "tcx_unet: emb_dim must be even and <= 256");
    TCX_REQUIRE(net->time_ch + net->cond_ch <= 64 && net->y_cont_dim >= 3 && net->y_cont_dim <= 16, "tcx_unet: bad cond dims");
    TCX_REQUIRE((H / 4) * (W / 4) <= 256 || ((H / 4) * (W / 4)) % 256 == 0,
                "tcx_unet: bottleneck attention needs N <= 256 or N %% 256 == 0 tokens");
    TCX_REQUIRE(net->precision >= 0 && net->precision <= 2,
                "tcx_unet: precision must be 0 (fp32), 1 (f16x3) or 2 (bf16)");
    TCX_REQUIRE(net->precision == 0 || (net->base_ch % 32 == 0 && ((H / 4) * (W / 4)) % 32 == 0),
                "tcx_unet: the split paths need base_ch %% 32 == 0 and (H/4)*(W/4) %% 32 == 0");
    TCX_REQUIRE(net->precision != 2 || ((H / 4) * (W / 4)) % 256 == 0,
                "tcx_unet: bf16 precision needs (H/4)*(W/4) %% 256 == 0 (the split attention)");
    return TCX_OK;
}

// workspace of one sampling lane (rows 2*ceil(Bt/(2L)) >= ceil(Bt/L): an upper bound for B or 2B rows)
size_t lane_ws_bytes(const tcx_unet* net, int Bt, int H, int W, int L) {
    const int rows = 2 * ((Bt + 2 * L - 1) / (2 * L));
    return align_up(single_ws_bytes(net, rows, H, W), 256);
}

int unet_eval_impl(const EvalArgs& e) {
    const tcx_unet* net = e.net;
    const int B = e.B, H = e.H, W = e.W, mode = e.mode;
    TCX_TRY(validate(net, B, H, W));
    TCX_TRY(injected_failure());
    TCX_REQUIRE(e.x && e.t && e.y_cat && e.y_cont && e.ws, "tcx_unet_eval: null pointer");
    TCX_REQUIRE(mode >= 0 && mode <= 7, "tcx_unet_eval: bad mode");
    TCX_REQUIRE(mode == 0 || e.scal, "tcx_unet_eval: sampler modes need the step table row");
    TCX_REQUIRE(mode == 1 || mode >= 6 || e.eps_out, "tcx_unet_eval: eps_out needed");
    TCX_REQUIRE((mode != 1 && mode != 3 && mode != 4 && mode < 6) || e.x_inout, "tcx_unet_eval: x_inout needed");
    TCX_REQUIRE(mode < 6 || (e.coef && e.hist), "tcx_unet_eval: DPM-Solver++ steps need the coefficient row and history");
    TCX_REQUIRE(mode != 3 || e.x2, "tcx_unet_eval: Heun stage 1 needs x2");
    const int cfg = e.guidance > 0.f ? 1 : 0;
    const int Bc = chunk_images(B, max_pass_rows(net, H, W) / (cfg ? 2 : 1));
    const int Btc = cfg ? 2 * Bc : Bc;
    char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(e.ws), 256));
    const size_t need = make_plan(net, Btc, H, W, nullptr).bytes;
    TCX_REQUIRE(need + (base - (char*)e.ws) <= e.ws_bytes, "tcx_unet_eval: workspace too small (%zu < %zu)", e.ws_bytes,
                need + 256);
    const size_t HW = (size_t)H * W;
    for (int c0 = 0; c0 < B; c0 += Bc) {
        const int bc = std::min(Bc, B - c0);
        const int Bt = cfg ? 2 * bc : bc;
        Plan P = make_plan(net, Bt, H, W, base);
        const size_t e0 = (size_t)c0 * HW;
        CondRows ctc = e.ct;
        if (ctc.bias_img) ctc.bias_img += (size_t)c0 * net->base_ch;
        TCX_TRY(unet_body(net, P, e.x + e0, bc, e.t_per_sample ? e.t + c0 : e.t, e.t_per_sample, e.y_cat + c0,
                          e.y_cont + (size_t)c0 * net->y_cont_dim, cfg, e.stream, ctc));
        StepFields a{};
        a.r = P.r; a.out_b = net->out_b; a.B = bc; a.H = H; a.W = W; a.cfg = cfg; a.guidance = e.guidance;
        a.mode = mode; a.scal = e.scal; a.x = e.x + e0; a.x_inout = e.x_inout ? e.x_inout + e0 : nullptr;
        a.x2 = e.x2 ? e.x2 + e0 : nullptr; a.eps_out = e.eps_out ? e.eps_out + e0 : nullptr;
        a.z = e.z ? e.z + e0 : nullptr;
        a.seed = e.seed; a.step = e.step; a.e0 = e.e_base + e0;
        a.coef = e.coef; a.hist = e.hist ? e.hist + e0 : nullptr;
        TCX_TRY(launch_step(a, e.stream));
    }
    return TCX_OK;
}

}  // namespace tcx

using namespace tcx;

extern "C" size_t tcx_unet_workspace_size(const tcx_unet* net, int Bt, int H, int W) {
    if (!net) return 0;
    const int L = lanes_setting();
    const size_t one = single_ws_bytes(net, Bt, H, W);
    return L > 1 ? std::max(one, (size_t)L * lane_ws_bytes(net, Bt, H, W, L) + 256) : one;
}

extern "C" int tcx_unet_eval(const tcx_unet* net, const float* x, float* x2, const float* t, int t_per_sample,
                             const int64_t* y_cat, const float* y_cont, int B, int H, int W, float guidance, int mode,
                             const float* scal, const float* z, uint64_t seed, uint64_t step, float* x_inout,
                             float* eps_out, void* ws, size_t ws_bytes, void* stream) {
    // modes 6 / 7 (the DPM-Solver++ steps) exist only inside tcx_dpmpp_sample
    TCX_REQUIRE(mode >= 0 && mode <= 5, "tcx_unet_eval: bad mode");
    EvalArgs a{};
    a.net = net; a.x = x; a.x2 = x2; a.t = t; a.t_per_sample = t_per_sample; a.y_cat = y_cat; a.y_cont = y_cont;
    a.B = B; a.H = H; a.W = W; a.guidance = guidance; a.mode = mode; a.scal = scal; a.z = z; a.seed = seed; a.step = step;
    a.x_inout = x_inout; a.eps_out = eps_out; a.ws = ws; a.ws_bytes = ws_bytes; a.stream = (hipStream_t)stream;
    return unet_eval_impl(a);
}
