// The memory passes and attention helpers that the U-Net evaluator (unet.hip and its units) calls in norm.hip,
// attention_split.hip and attn_block.hip.  The defining files include this too, so the compiler checks each
// definition against the one declaration.  (conv3g_covers is declared in conv_common.hpp.)
#pragma once
#include "common.hpp"

namespace tcx {

// h2 / bf16 record writers (norm.hip, attention_split.hip): bf != 0 writes bf16 halves
bool upsample_fused_ok(int H, int W, int C);  // norm.hip: band / segmented band
bool attn_prep_ok(int HW, int C, int groups, int bf);  // norm.hip: the attention input pass
int attn_prep_h2(float* a, void* y, int Bt, int HW, int C, const float* sc, const float* sh, const float* gamma,
                 const float* beta, int groups, unsigned* ovf, int bf, hipStream_t st);
int pass_forms();  // norm.hip: tcx_debug_pass_forms' mask (bit 0 first conv, 1 upsample, 2 head: the older form)
int upsample2x_h2(const float* x, void* y, int Bt, int H, int W, int C, const float* scale, const float* shift,
                  unsigned* ovf, int bf, hipStream_t st);
int gn_apply_tab_h2(const float* x, void* y, int Bt, int HW, int C, const float* scale, const float* shift, int silu,
                    unsigned* ovf, int bf, hipStream_t st);
int gn_apply_b2_inplace(void* x, int Bt, int HW, int C, const float* scale, const float* shift, int silu,
                        hipStream_t st);
bool gn_apply_cm_ok(int HW, int C);  // norm.hip: chunk-major skip-tensor records
int gn_apply_b2cm(const void* x, void* y, int Bt, int HW, int C, const float* scale, const float* shift,
                  hipStream_t st);  // norm.hip: config 5's chunk-major b2 skip planes
int gn_apply_cm(const float* x, void* y, int Bt, int HW, int C, const float* scale, const float* shift,
                unsigned* ovf, hipStream_t st);
int attention_split(const void* qkv, void* out, int Bt, int N, int C, int heads, int bf, hipStream_t st);
// attn_block.hip: the qkv conv inside the attention workgroup (f16x3, N = 256, C = 192, 4 heads)
bool attn_block_ok(int fmt, int Bt, int N, int C, int heads, const tcx_conv& qkv, const tcx_conv& proj, const void* x,
                   const void* a, const void* o);

}  // namespace tcx
