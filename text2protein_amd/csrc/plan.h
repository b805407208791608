// The plan switches: the state behind t2p_debug_set (include/t2p.h; the key table is next to it in capi.cpp).  Tests and A/B
// measurements use them to choose between kernel forms that ALL give correct results (the ablation bits of `dbg` excepted); the
// product path never sets one.  Process-wide and unsynchronised; read per launch unless the comment names another moment.
#pragma once

namespace t2p {

struct Plan {
  // ---- GEMM / implicit-GEMM convolution (gemm.hip, gemm_dma.hip, rowgemm.hip) ----
  bool dma = true;             // 0: 16-bit products on the LDS-DMA kernels where eligible (else the register-staged kernel)
  int dbg = 0;                 // 1: mask of the LDS-DMA kernels: 128 / 256 DMA issue order, 4096 LDS-staged instead of register epilogue, 8192 general
                               //    instead of specialised register epilogue (same results); timing-only ablations of the -DT2P_ABLATION build (results
                               //    are wrong): 1 no epilogue, 2 no DMA in loop, 4 no reads/MFMA
  int dma_geom = 0;            // 2: tile geometry: 0 auto, 1 force 256x128x3, 2 force 128x128x2, 3 force 256x256x2, 4 force 512x128x2; 5 the former
                               //    policy (256x256 where N % 256 == 0, else 256x128), 6 auto without the tall tile for narrow outputs (kept for A/B)
  bool splitk = true;          // 3: K loop split over workgroups where the tile grid cannot fill the chip (needs a workspace)
  int dma_ring = 2;            // 8: 128 x 64 wave-tile geometries: 2 = 2 + 2 ring stages with v_mfma_16x16x32 (default: +5 % over the 32x32x16 shape,
                               //    it sustains a higher clock); 1 = 2 + 2 stages, 32x32x16; 0 = 3 A + 2 B stages (160 KiB; measured equal to 1)
  int op_ws_mib = 0;           // 10: split-K workspace of the op entries (t2p_op_*), in MiB; 0 none
  int force_nsplit = 0;        // 11: development: > 0 forces that split-K factor wherever a workspace is attached
  bool midsplit = false;       // 12: mid-size problems: 256x256 tiles + split-K instead of 128x128 tiles (round 1 default; with the 4-stage 128x128
                               //     ring the unsplit plan is as fast and saves the second pass: -0.27 ms at cfg2)
  bool thin_conv = true;       // 15: thin-output head convolution on its own kernel
  bool up4 = true;             // 21: up-sampling 3x3 convolutions as four 2x2 phase convolutions where the caller supplies Bw4
  bool deep_ring = true;       // 22: small launches of the 128 x 128 geometry on a 4-stage ring
  bool fuse_shortcut = true;   // 23: 1x1 shortcut of a residual block folded into its second convolution (gemm_can_fuse_shortcut)
  bool post_gn = true;         // 28: the GroupNorm that follows a product applied by the split-K second pass (gemm_fuses_post_gn)
  int split_tiles = 192;       // 30: development: split-K where the tile grid has fewer tiles than this (values <= 0 are ignored)
  int split_target = 256;      // 31: development: workgroups (tiles x splits) a split-K launch aims at (values <= 0 are ignored)
  bool a_norm = true;          // 34: GroupNorm + SiLU of the head inside the head convolution's halo staging
  bool dxs = true;             // 47: full-resolution 3x3 convolutions on the dx-shared-stage kernel (gemm_dxs_kernel) where eligible
  int rowres = 1;              // 49: row-resident K = 512 GEMM: 0 off, 1 the planner's choice (gemm_rowres_planned), 2 wherever gemm_rowres_eligible
  // ---- norms, input convolution, attention, small maps, row chains (kernels.hip, attention.hip, smallconv.hip, stfuse.hip) ----
  bool gn_small = true;        // 13: engine / op API: single-launch GroupNorm for maps of <= 64 pixels
  bool gn_apply16 = true;      // 17: GroupNorm apply on 16-bit maps: 16-byte accesses, 4 pixels in flight
  bool layernorm16 = true;     // 20: LayerNorm of 16-bit rows of 512 / 1024 channels: the row is read once
  bool pre_conv_mfma = true;   // 26: input convolution on the fp32 matrix pipe
  bool gn_apply_cols = true;   // 27: GroupNorm finalize inside the apply launch on maps of <= 4096 pixels
  bool attn_strip = true;      // 29: one-launch wide-head attention (AttnBlockpp)
  bool small_conv = true;      // 36: one-launch convolution + GroupNorm of the 8x8 / 4x4 levels
  bool pre_conv_split = true;  // 38: input convolution on the 16-bit matrix pipe, every fp32 operand split into two f16 terms
  bool st_fuse = true;         // 39: row-block chains of a SpatialTransformer block in one launch
  // ---- engine (engine.cpp) ----
  bool raw_copies = true;      // 4: feed 1x1 shortcut / proj_out GEMMs with compute-dtype copies
  bool flash_attention = true; // 5: engine / op API: fused attention kernel where eligible
  bool fuse_gn_stats = true;   // 6: GroupNorm statistics from the producing GEMM epilogue
  bool fuse_geglu = true;      // 7: GEGLU gating inside the ff1 GEMM epilogue
  bool lowp_h1 = true;         // 9: block-internal conv0 output stored in the compute dtype
  bool lowp_residual = true;   // 14: residual stream between blocks in the compute dtype (f16 mode)
  bool qkv_fused = true;       // 25: self-attention: one q | k | v projection, V read row-major by the fused kernel
  bool attn_merged = true;     // 32: AttnBlockpp: NIN_2 . NIN_3 as one projection, output epilogue in the attention kernel
  bool ffpo_merged = true;     // 33: SpatialTransformer: ff.net.2 and proj_out as one GEMM over [g | t]
  bool st_tail = true;         // 40: the chain after the cross-attention (to_out + residual -> LayerNorm_3 -> ff.net.0 with GEGLU) on the row-block
                               //     kernel too (Engine::st_block)
  bool small_conv_fm = true;   // 41: the small-map convolution kernel reads fragment-major weight copies
  bool st_ffpo = true;         // 42: the merged ff.net.2 / proj_out product inside the chain after the cross-attention
  int st_tail_rows = 4096;     // 43: development: fewest rows for which the block's last chain (with the third product) is taken; without the
                               //     third product (42 off) the chain needs twice as many
  bool attn_fm = true;         // 45: fragment-major K / V^T for the wide-head attention kernel (where the shapes allow it)
  bool attn_proj = true;       // 46: the projections of an AttnBlockpp in one launch at C = 256 (attn_proj_kernel)
  // ---- trainer (train.cpp) ----
  bool train_plumbing16 = false;  // 48: read when a trainer is CREATED: an f32 trainer runs the 16-bit step's plumbing (fixed-order reductions,
                                  //     scaled backward seed, overflow guard) on its own products
};

inline Plan g_plan;

}  // namespace t2p
