/* mgdt.h - C ABI of the MI355X-native MGDT-YOLO detection hot path (libmgdt_hip.so).
 *
 * Every entry point: plain pointers/sizes, no torch types, asynchronous on the caller's hipStream_t,
 * never allocates or frees device memory (the caller owns inputs, outputs, packed weights and
 * workspaces), returns 0 on success or a negative mgdt_status; mgdt_last_error() gives the text
 * (thread-local).  No host synchronisation inside, except where noted.
 *
 * Activations are addressed through `mgdt_view`: an NHWC-ordered 4-d view with explicit element
 * strides, so channel slices of a wider tensor (the reference's chunk()/split()/cat() on dim 1) and
 * torch channels_last tensors are passed without copies.
 *
 * Each function cites the reference interface (paths relative to the reference repo root) it replaces.
 */
#ifndef MGDT_H
#define MGDT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mgdt_stream; /* hipStream_t */

typedef enum { MGDT_OK = 0, MGDT_BAD_SHAPE = -1, MGDT_BAD_DTYPE = -2, MGDT_LAUNCH_FAIL = -3, MGDT_BAD_ARG = -4,
               MGDT_WORKSPACE = -5 } mgdt_status;
typedef enum { MGDT_F32 = 0, MGDT_BF16 = 1, MGDT_U8 = 2 /* image input of mgdt_conv2d_direct_fwd only */ } mgdt_dtype;
typedef enum { MGDT_ACT_NONE = 0, MGDT_ACT_SILU = 1, MGDT_ACT_RELU = 2, MGDT_ACT_GELU = 3 } mgdt_act;

/* 4-d activation view; sizes in elements, strides in elements of `dtype`. p may be NULL for "absent". */
typedef struct {
  void* p;
  int32_t n, h, w, c;
  int64_t sn, sh, sw, sc;
} mgdt_view;

const char* mgdt_last_error(void);
const char* mgdt_version(void);

/* ---- weight packing: nn.Conv2d weight (OIHW fp32) [+ BatchNorm2d fold] -> MFMA fragment order ----------
 * Replaces yolo/utils/torch_utils.py:114-135 (fuse_conv_and_bn) + the implicit weight layout of ATen conv2d.
 * bn_* may all be NULL (no BN; conv_bias optional).  With BN: W' = diag(g/sqrt(var+eps)) W,
 * b' = beta - g*mean/sqrt(var+eps) (+ scaled conv bias).  Outputs: packed weights (size from
 * mgdt_conv_packed_bytes) and bias_out[cout_pad] fp32 (cout rounded up to 16).                          */
size_t mgdt_conv_packed_bytes(int cin, int cout, int k, int dtype);
int mgdt_conv_pack(const float* w_oihw, const float* conv_bias, const float* bn_gamma, const float* bn_beta,
                   const float* bn_mean, const float* bn_var, float bn_eps, int cin, int cout, int k, int dtype,
                   void* packed_out, float* bias_out, mgdt_stream s);
/* Weights of the stride-1 data-gradient convolution: dx = mgdt_conv2d_fwd(x = dy, packed, k, stride 1, y = dx) with
 * w'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx] (what autograd's conv backward computes for stride 1, same padding).  cin / cout are
 * those of the original conv; size the buffer with mgdt_conv_packed_bytes(cout, cin, k, dtype); bias_out: fp32[cin rounded up to 16], zeroed. */
int mgdt_conv_pack_dgrad(const float* w_oihw, int cin, int cout, int k, int phase, int dtype, void* packed_out, float* bias_out, mgdt_stream s);
/* Many packs in a few launches (a training step re-packs every convolution after the optimizer moved the weights; the reference has no counterpart:
 * ATen convolutions read nn.Conv2d.weight in place).  One descriptor = the arguments of one mgdt_conv_pack (mode 0) or mgdt_conv_pack_dgrad
 * (mode 1 = stride-1 data gradient, mode 2 + phase = stride-2 phase) or mgdt_conv_pack_stem6 (mode 5 + cin, k = 3, w = the 6x6 weight) or
 * mgdt_conv_pack_deconv2x2 (mode 10 + phase, k = 1, w = the (cin, cout, 2, 2) weight, conv_bias = its bias) or mgdt_conv_pack_deconv2x2_dgrad (mode 14 + phase) call; cin / cout are those of the ORIGINAL
 * convolution. */
typedef struct mgdt_pack_desc {
  const float* w; const float* conv_bias; const float* bn_gamma; const float* bn_beta; const float* bn_mean; const float* bn_var;
  float bn_eps; int32_t cin, cout, k, dtype, mode;
  void* packed; float* bias_out;
} mgdt_pack_desc;
int mgdt_conv_pack_batch(const mgdt_pack_desc* descs, int n, mgdt_stream s);
/* phase = -1: stride 1 (above).  phase = 2*py + px in 0..3 (k = 3, stride 2, even input size): the data gradient at input pixels
 * (2a + py, 2b + px) is a 3x3 same-padding convolution over dy with the taps w[py + 1 - 2*dy'][px + 1 - 2*dx'] that exist:
 * dx[:, py::2, px::2] = mgdt_conv2d_fwd(x = dy, packed(phase), k = 3, stride 1, y = that strided view). */

/* ---- fused convolution (implicit GEMM on MFMA) ------------------------------------------------------------
 * Replaces nn/modules/conv.py:25-42 Conv.forward/forward_fuse (conv2d + folded BN + act), the Bottleneck
 * shortcut add (nn/modules/block.py:514-526), the MSPA pre-add `sp + spx[i]` (block.py:252-254), the
 * channel-slice reads/writes that stand in for chunk()/cat() (block.py:203-207,250-266), nn.Linear on NHWC
 * tokens (convnextv2.py:59,62) and GRN's per-(image,channel) affine on the input (utils.py:171-182).
 *   y = act( conv(k, stride, pad=k/2)( (x [+ x2]) [* in_scale[n,c] + in_shift[c]] ) + bias ) [+ r1] [+ r2]
 * groups == 1, k in {1,3}, stride in {1,2}, cin % (4 fp32 | 8 bf16) == 0, all views sc == 1.               */
int mgdt_conv2d_fwd(const mgdt_view* x, const mgdt_view* x2, const float* in_scale, const float* in_shift,
                    const void* packed_w, const float* bias, int k, int stride, int act, const mgdt_view* r1,
                    const mgdt_view* r2, const mgdt_view* y, int dtype, mgdt_stream s);
/* ---- fp8 (OCP e4m3fn) variant of the fused convolution - BASELINE configs[4] ("fp8 inference: CDNA4 fp8-MFMA implicit-GEMM convs"; the
 * reference has no fp8 path: yolo/engine/trainer.py:223 is fp16 autocast only, so the numerics are checked against an e4m3 emulation of
 * nn/modules/conv.py:25-42 and, end to end, against the fp32 fixtures with a stated tolerance).
 * W8A8, fp32 accumulation: activations stay bf16 in HBM and are converted in registers, x_q = e4m3(clamp(x * x_qscale, +-448)) (per-tensor
 * x_qscale, calibrated by the caller); weights are packed once as e4m3(w' / w_scale[co]) with w' the BN-folded weight and
 * w_scale[co] = max|w'[co]| / 448; y = act(acc * oscale[co] + bias[co]) [+ r1] [+ r2], oscale[co] = w_scale[co] / x_qscale.
 * mgdt_conv_pack_fp8 writes the panel (mgdt_conv_packed_bytes_fp8), bias_out[cout_pad] and oscale_out[cout_pad] (cout rounded up to 16);
 * mgdt_conv2d_fp8_fwd takes the same views / fused extras as mgdt_conv2d_fwd with dtype MGDT_BF16.  cin % 8 == 0, cout % 4 == 0, k in {1, 3}. */
size_t mgdt_conv_packed_bytes_fp8(int cin, int cout, int k);
int mgdt_conv_pack_fp8(const float* w_oihw, const float* conv_bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                       const float* bn_var, float bn_eps, int cin, int cout, int k, float x_qscale, void* packed_out, float* bias_out,
                       float* oscale_out, mgdt_stream s);
int mgdt_conv2d_fp8_fwd(const mgdt_view* x, const mgdt_view* x2, const float* in_scale, const float* in_shift, const void* packed_w,
                        const float* bias, const float* oscale, float x_qscale, int k, int stride, int act, const mgdt_view* r1,
                        const mgdt_view* r2, const mgdt_view* y, mgdt_stream s);
/* Host-only route query: the plan mgdt_conv2d_fwd (or, with MGDT_ROUTE_FP8, mgdt_conv2d_fp8_fwd) would launch for these views and fused extras.  It
 * launches nothing, needs no device and never looks at a pointer (p may be NULL); sizes, strides, k, stride, dtype and act are checked as the launch
 * checks them.  The launch and this query call the same planning functions, experiment knobs (environment) included.
 *   flags: which optional operands are present.
 *   family MGDT_ROUTE_IGEMM (conv_igemm_kernel<T, NT, MT, D, extra, nseg > 1>): NT cout blocks of 16 per workgroup, MT pixel groups of 16 per wave,
 *     D = register sets of the K pipeline, nseg x seg_chunks = the staged weight panel, grid gx x gy workgroups of `waves` waves walking numTiles pixel
 *     tiles (persistent when numTiles > gx), ragged = the last cout block is partly padding (cout % 16 != 0).
 *   family MGDT_ROUTE_LDS3X3 (conv3x3_lds_kernel): NBW cout blocks per workgroup, tiles of tile_rows x 16 output pixels, ncg cout groups, nwg
 *     workgroups of `waves` waves over ntiles tiles.
 *   nchunks (K chunks of 4 pieces), waves and lds_bytes (dynamic LDS of the launch) are filled for both; the other family's fields are 0. */
enum { MGDT_ROUTE_X2 = 1, MGDT_ROUTE_IN_SCALE = 2, MGDT_ROUTE_IN_SHIFT = 4, MGDT_ROUTE_R1 = 8, MGDT_ROUTE_R2 = 16, MGDT_ROUTE_FP8 = 32 };
enum { MGDT_ROUTE_IGEMM = 0, MGDT_ROUTE_LDS3X3 = 1 };
typedef struct {
  int32_t family, nchunks, waves, lds_bytes;
  int32_t NT, MT, D, extra, nseg, seg_chunks, gx, gy, numTiles, ragged; /* igemm */
  int32_t NBW, tile_rows, ncg, nwg, ntiles;                             /* lds3x3 */
} mgdt_conv_route;
int mgdt_conv2d_route(const mgdt_view* x, const mgdt_view* y, int k, int stride, int dtype, int flags, int act, mgdt_conv_route* out);
/* One phase (py, px) = phase >> 1, phase & 1 of the data gradient of a stride-2 3x3 convolution: dx[:, 2i+py, 2j+px] as a stride-1 convolution of dy
 * whose K holds only the taps that phase uses (packed by mgdt_conv_pack_dgrad(phase)); replaces the four 9-tap convolutions over mostly-zero weights.
 * Reference: the autograd of the stride-2 nn.Conv2d layers (backbone rows 0, 1, 3, 5, 7 of models/v8/*.yaml). */
int mgdt_conv2d_phase_fwd(const mgdt_view* x, const void* packed_w, const float* bias, int phase, const mgdt_view* r1, const mgdt_view* r2,
                          const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- ConvNeXtV2 block MLP, hidden map kept on chip (nn/modules/convnextv2.py:62-77: pwconv1 -> GELU -> GRN -> pwconv2 -> + input).
 * t = LayerNorm output, res = the block input, y = res + pwconv2(GRN(gelu(pwconv1(t)))).  Two launches: GRN statistics, then
 * apply (both compute pwconv1 + GELU).  w1 [4c][c], w2 [c][4c] row-major as nn.Linear.weight; gamma/beta [4c] (GRN).
 * Covered: bf16 with c in {32, 64, 96} (both weight panels in LDS); mgdt_cnx_mlp_packed_bytes returns 0 otherwise and the caller
 * keeps the mgdt_conv2d_fwd / mgdt_grn_stats_fwd chain. */
size_t mgdt_cnx_mlp_packed_bytes(int c, int dtype);
int mgdt_cnx_mlp_pack(const float* w1, const float* b1, const float* w2, const float* b2, int c, void* packed, int dtype, mgdt_stream s);
size_t mgdt_cnx_mlp_workspace_bytes(int n, int h, int w, int c);
int mgdt_cnx_mlp_fwd(const mgdt_view* t, const mgdt_view* res, const void* packed, const float* gamma, const float* beta, void* ws,
                     const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- a whole ConvNeXtV2 block in ONE launch, bf16 inference (nn/modules/convnextv2.py:48-77): dw 7x7 + bias + LayerNorm, pwconv1 + GELU with the
 * 4c-wide hidden tile kept in registers, GRN (the workgroups of an image meet at a per-image barrier for sum_hw h^2), pwconv2 + residual.
 * x, y: N x H x W x c NHWC views (y may not alias x: neighbouring tiles read x's halo), dw_w49c [49][c] fp32 (tap-major), packed: the blob of
 * mgdt_cnx_mlp_pack.  ws (mgdt_cnx_block_workspace_bytes, 16-byte aligned): its first 4096 bytes are the per-image barrier words (arrival
 * counter + generation) that MUST BE ZERO at the first call and belong to this function from then on (the counters are back at zero when a
 * call ends, so hipGraph replays and calls with other shapes need no reset; at most 512 images per call).  mgdt_cnx_block_supported: c in {32, 64, 96}, bf16, a tile decomposition with at most as many tiles per image as the chip has
 * compute units (every workgroup of a launch is resident at once; larger batches run as several launches of whole images).
 * tail_w / tail_b / tail_act (NULL / NULL / 0 for none): a 1x1 Conv + BN + act applied to the block's output inside the launch - the IFM's closing
 * Conv (nn/modules/block.py:336-338) - packed with mgdt_conv_pack(c, cout, 1, bf16) over input channels in the accumulator order of
 * mgdt_conv1x1_inject_conv_fwd's note (j < c / 32); y then has cout <= c channels and the block's own output is never stored. */
int mgdt_cnx_block_supported(int n, int h, int w, int c, int dtype);
/* mgdt_cnx_block_geometry: the tiling mgdt_cnx_block_fwd uses for an h x w map of c channels (no device needed): out[7] = {TH, TW, SEGS (5-pixel
 * segments per tile row), tiles_x, tiles per image, 16-pixel groups per tile (one per wave, <= 16), dynamic LDS bytes}.  MGDT_BAD_SHAPE when c is
 * not 32 / 64 / 96 or no tile exists; a map with more tiles than the chip has compute units still has a geometry (mgdt_cnx_block_supported refuses it). */
size_t mgdt_cnx_block_workspace_bytes(int n, int h, int w, int c);
int mgdt_cnx_block_geometry(int h, int w, int c, int* out);
int mgdt_cnx_block_fwd(const mgdt_view* x, const float* dw_w49c, const float* dw_b, const float* ln_w, const float* ln_b, float eps, const void* packed,
                       const float* gamma, const float* beta, const void* tail_w, const float* tail_b, int tail_act, void* ws, size_t ws_bytes,
                       const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- layers 0 and 1 of every YOLOv8 graph (Conv 3->16 k3 s2, Conv 16->32 k3 s2, both + BN + SiLU; models/v8/*.yaml rows 0-1) in one
 * launch, bf16 path: the image patch is staged in LDS with 16-byte row loads, layer 0 runs on MFMA out of LDS, its map never leaves the
 * CU.  x: N x 3 x H x W NCHW image (any strides), x_dtype MGDT_BF16 / MGDT_F32 / MGDT_U8 (u8 is divided by 255 like
 * yolo/engine/predictor.py:129); y: N x H/4 x W/4 x 32 bf16 NHWC.  packed0 = mgdt_stem2_pack(W' of layer 0, fp32 [16][3][3][3] with the
 * BatchNorm scale folded in as fuse_conv_and_bn does), bias0[16]; packed1 / bias1 = mgdt_conv_pack(16, 32, 3, MGDT_BF16). */
size_t mgdt_stem2_packed_bytes(void);
int mgdt_stem2_pack(const float* w_folded, void* packed, mgdt_stream s);
int mgdt_stem2_fwd(const mgdt_view* x, int x_dtype, const void* packed0, const float* bias0, const void* packed1, const float* bias1,
                   const mgdt_view* y, mgdt_stream s);
/* Debug: the launch geometry of mgdt_stem2_fwd for an n x 3 x h x w image on a device with cu_count compute units (<= 0: the current device's).
 * The kernel is persistent: out[0] = tiles (8 x 16 output pixels each), out[1] = workgroups launched (<= tiles, <= out[3] * out[4]; the experiment
 * knob MGDT_STEM_WGS=<n> in the environment caps it), out[2] = LDS bytes per workgroup, out[3] = workgroups per compute unit, out[4] = compute units. */
int mgdt_stem2_geometry(int n, int h, int w, int cu_count, int* out);
/* Host-side route query: what mgdt_stem2_fwd would launch for the image view x (x_dtype) and the output view y on a device with cu_count compute units
 * (<= 0: the current device's), without launching.  The launch and this query run the same planning function, MGDT_STEM_WGS included.  Pointers are only
 * tested for alignment.  out[7] = {fast loader (1: bf16 image with contiguous, 16-byte aligned rows and W % 8 == 0 - 16-byte loads, next patch
 * prefetched; 0: the element-wise loader), tiles_x, tiles_y, tiles, workgroups, tiles per XCD range, status}: status is MGDT_OK, or what the launch
 * fails with before launching anything (the other entries are then 0). */
int mgdt_stem2_route(const mgdt_view* x, int x_dtype, const mgdt_view* y, int cu_count, int* out);

/* ---- Detect head tail in one launch, bf16 (nn/modules/head.py:150-177): the two final 1x1 convs with bias (box c2 -> 16, cls c3 -> nc), the raw
 * (N, 16+nc, H, W) map and its decode (DFL expectation, dist2bbox, stride, sigmoid) into y[N][4+nc][a_total] at anchor offset a_off.
 * wb/bb, wc/bc: mgdt_conv_pack(c2, 16, 1, bf16) / mgdt_conv_pack(c3, nc, 1, bf16) with the conv biases.  reg_max must be 4 (this fork's
 * Detect); other heads keep mgdt_conv2d_fwd + mgdt_detect_decode_fwd.  best_keys: NULL, or [N][a_total] - per anchor the NMS key of its
 * best class (first maximal score, ops.py:225-226), see mgdt_nms_fwd.  wb3 / bb3: NULL, or mgdt_conv_pack(16, 16, 3, bf16) of the box branch's second
 * Conv (cv2[i][1], head.py:150: 3x3, BN, SiLU) - tb is then THAT conv's input and the conv runs inside this launch; wb must then be packed from the
 * final 1x1's weight zero-padded to 32 input channels (its 16 real ones in the accumulator order of mgdt_conv1x1_inject_conv_fwd's note). */
int mgdt_detect_tail_supported(int c2, int c3, int nc, int reg_max, int dtype);
int mgdt_detect_tail_fwd(const mgdt_view* tb, const mgdt_view* tc, const void* wb, const float* bb, const void* wc, const float* bc, int nc,
                         float stride, int a_off, int a_total, const mgdt_view* feat, float* y, unsigned long long* best_keys,
                         const void* wb3, const float* bb3, mgdt_stream s);
/* The same launch with the test-time augmentation epilogue (nn/tasks.py:276-285 _descale_pred): the decoded xywh are divided by aug_scale,
 * then x = aug_img_w - x when aug_flip (the pass ran on the left-right flipped image; aug_img_w = the ORIGINAL image width).  y / best_keys are
 * the merged buffer of all passes: a_off is the level's offset in it, a_total its anchor count. */
int mgdt_detect_tail_aug_fwd(const mgdt_view* tb, const mgdt_view* tc, const void* wb, const float* bb, const void* wc, const float* bc, int nc,
                             float stride, int a_off, int a_total, const mgdt_view* feat, float* y, unsigned long long* best_keys,
                             const void* wb3, const float* bb3, float aug_scale, int aug_flip, float aug_img_w, mgdt_stream s);

/* ---- test-time augmentation input (yolo/utils/torch_utils.py:261-270 scale_img, after x.flip(3) when flip): x = N x 3 x H x W image (any
 * strides; MGDT_F32 / MGDT_BF16 / MGDT_U8, u8 divided by 255), y = N x 3 x Hp x Wp (y_dtype MGDT_F32 / MGDT_BF16; 16-byte runs along W when
 * W is contiguous).  Rows / columns below hs x ws are the bilinear resize of the (flipped) image to hs x ws (align_corners=False, PyTorch's
 * CPU index and weight arithmetic), the rest is `pad`. */
int mgdt_scale_img_fwd(const mgdt_view* x, int x_dtype, int flip, int hs, int ws, float pad, const mgdt_view* y, int y_dtype, mgdt_stream s);

/* ---- a whole CSP block (MSPA_C2f / C2f) in one launch, bf16 inference (nn/modules/block.py:187-287, :514-526):
 *   mode 0 (MSPA_C2f): front = the three chained 1x1 convs of mgdt_pw_chain3_fwd (blob of mgdt_pw_chain_pack), bottleneck input
 *                      sp2 + x[3wd:4wd]; concat = [sp0 | sp1 | sp2 | b_0 .. b_{n-1}]
 *   mode 1 (C2f):      x = cv1's output (2wd channels, computed by mgdt_conv2d_fwd), front / front_bias unused (NULL); bottleneck
 *                      input = its second half; concat = [x | b_0 .. b_{n-1}]
 *   then n bottlenecks (two 3x3 convs wd -> wd each, mgdt_conv_pack panels mid[2n] in execution order, residual add when `shortcut`)
 *   and the 1x1 conv `back` over the concat -> y.  One workgroup computes one spatial tile of one image with the halo (2n pixels)
 *   recomputed; nothing but x is read from and nothing but y written to HBM.  All convs share `act`.
 *   pool: NULL, or fp32 [n][slots][cout]: channel sums of y per tile (slot = tile * (slots / tiles) + k, tiles in row-major order);
 *   slots = mgdt_csp_block_tiles(...), which also reports {TH, TW, RH, RW, lds bytes, workgroups, tiles_x, tiles_y} in geom8 when
 *   non-NULL; feed it to mgdt_spr_attn_scale_fwd(pool, slots, tiles_x, tiles_y, ...).  mode 0 needs even h, w and picks an even
 *   tile grid (every tile lies inside one adaptive_avg_pool2d(2) bin).
 *   mgdt_csp_block_supported: 1 when covered (bf16; wd in {8,16,32,64}; n in {1,2}; mode 0: cin == 4wd; mode 1: cin == 2wd,
 *   wd >= 16); otherwise callers keep the per-conv launches.
 *   mode 2 (C3, nn/modules/block.py:434-447): x = [a | b] = the output of ONE 1x1 launch over cat(cv1, cv2) (cin == 2wd, wd in {16,32,64}, 16-byte
 *   aligned pixels), front NULL, mid[2*nbtl] = per bottleneck the 1x1 then the 3x3 panel (wd -> wd), back = cv3 over [m_n(a) | b] (K = 2wd, cout % 4 == 0,
 *   cout <= 512), pool NULL; halo n, tiles must divide the map (mgdt_csp_block_tiles == 0: none, e.g. a 37-row map). */
int mgdt_csp_block_supported(int mode, int cin, int cout, int wd, int nbtl, int h, int w, int dtype);
int mgdt_csp_block_tiles(int mode, int n, int cin, int cout, int wd, int nbtl, int h, int w, int* geom8);
int mgdt_csp_block_fwd(int mode, const mgdt_view* x, const void* front, const float* front_bias, const void* const* mid,
                       const float* const* mid_bias, int nbtl, int shortcut, const void* back, const float* back_bias, int wd, int act,
                       const mgdt_view* y, float* pool, int dtype, mgdt_stream s);

/* ---- MSPA_C2f hierarchical point-wise front in one launch (nn/modules/block.py:250-259, scale = 4):
 *   sp0 = act(conv0(x[0:wd])), sp1 = act(conv1(sp0 + x[wd:2wd])), sp2 = act(conv2(sp1 + x[2wd:3wd])), y[i*wd:(i+1)*wd] = sp_i
 * conv_i = 1x1 conv (wd -> wd) with BN folded.  x, y: N x H x W x 3*wd views (slices of the block input / concat buffer).
 * Pack the three convs with idx = 0, 1, 2 into one blob.  Covered: bf16, wd % 4 == 0, wd <= 64 (packed_bytes returns 0 otherwise
 * and the caller keeps three mgdt_conv2d_fwd launches). */
size_t mgdt_pw_chain_packed_bytes(int wd, int dtype);
int mgdt_pw_chain_pack(int idx, const float* w_oi, const float* conv_bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                       const float* bn_var, float bn_eps, int wd, int dtype, void* packed, mgdt_stream s);
int mgdt_pw_chain3_fwd(const mgdt_view* x, const void* packed, int wd, int act, const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- InjectionMultiSum_Auto_pool, up-sampling branch, in one launch (nn/modules/block.py:376-399):
 *   y = local_embedding(x) * bilinear(h_sigmoid(ga)) + bilinear(gf)      (align_corners=False, gate applied before interpolation)
 * packed_w / bias: the 1x1 local_embedding conv packed by mgdt_conv_pack (BN folded, no activation); ga, gf: equally laid out
 * N x Hg x Wg x cout maps with Hg <= H, Wg <= W.  mgdt_conv1x1_inject_supported tells whether the shapes are covered (bf16,
 * cin <= 128, cout in {128, 256}); otherwise the caller runs mgdt_conv2d_fwd + mgdt_inject_fwd. */
int mgdt_conv1x1_inject_supported(int cin, int cout, int h, int w, int hg, int wg, int dtype);
int mgdt_conv1x1_inject_fwd(const mgdt_view* x, const void* packed_w, const float* bias, const mgdt_view* ga, const mgdt_view* gf,
                            const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- injection + the NEXT layer's 1x1 Conv+BN+act in one launch (models/v8/mspa_c2f_gd_yolov8.yaml head rows 4-5: the injection's 256-channel
 * output has one consumer, C2f.cv1, nn/modules/block.py:199-201): y2 = act2(conv1x1(injection(x, ga, gf)) + bias2), the 256-channel map never
 * leaves the chip.  packed_w2 / bias2: mgdt_conv_pack(256, cout2, 1, bf16) of the second conv with its INPUT channels permuted to the first
 * conv's accumulator order: packed input channel (j*4 + g)*8 + e <- channel (2*j + e/4)*16 + 4*g + e%4 (j < 8, g < 4, e < 8).
 * Global maps: either ga / gf (computed by the caller; gsrc NULL) or gsrc = their common 32-channel input (block.py:377-381: x_g.split(...)[flag])
 * with packed_wg / bias_g = mgdt_conv_pack(32, 2 * cmid, 1, bf16) of [global_act | global_embedding] (cmid = 256): both 1x1 convs are then
 * evaluated on each tile's source pixels inside this launch and the 2 x cmid-channel maps never reach HBM either (ga / gf NULL). */
int mgdt_conv1x1_inject_conv_supported(int cin, int cmid, int cout2, int h, int w, int hg, int wg, int dtype);
int mgdt_conv1x1_inject_conv_fwd(const mgdt_view* x, const void* packed_w, const float* bias, const mgdt_view* ga, const mgdt_view* gf,
                                 const mgdt_view* gsrc, const void* packed_wg, const float* bias_g, int cmid,
                                 const void* packed_w2, const float* bias2, int act2, const mgdt_view* y2, int dtype, mgdt_stream s);

/* ---- SimFusion_3in / LAF with cv2 = cv3 = Identity in one launch, bf16 (nn/modules/block.py:309-329, eval):
 *   y = act2(cv_fuse([act1(cv1(p0)) | x1 | bilinear(x2)]))        (align_corners=False, x2 resampled to x1's size whatever its own)
 * p0 (N, h, w, c0): the avg-pooled first input; x1 (N, h, w, oc): the second input (in the model: channel slice [oc, 2 oc) of the concat buffer);
 * x2 (N, h2, w2, oc); y (N, h, w, oc).  All NHWC views with any 16-byte aligned pixel / row strides.  packed_w1 / bias1 = mgdt_conv_pack(c0, oc, 1,
 * bf16) of cv1, packed_w2 / bias2 = mgdt_conv_pack(3 * oc, oc, 1, bf16) of cv_fuse.  The values are those of mgdt_conv2d_fwd into concat slot 0,
 * mgdt_bilinear_fwd into slot 2 and mgdt_conv2d_fwd over the buffer, bit for bit; slots 0 and 2 are never written.
 * mgdt_laf_fuse_supported: bf16, c0 % 8 == 0 and <= 64, oc in {32, 64}, oc2 == oc, activations none / SiLU / ReLU. */
int mgdt_laf_fuse_supported(int c0, int oc, int oc2, int h, int w, int h2, int w2, int act1, int act2, int dtype);
int mgdt_laf_fuse_fwd(const mgdt_view* p0, const mgdt_view* x1, const mgdt_view* x2, const void* packed_w1, const float* bias1, int act1,
                      const void* packed_w2, const float* bias2, int act2, const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- SPPF / SPP in one launch, bf16 (nn/modules/block.py:121-153, eval):
 *   y = act2(cv2([x0 | y1 | y2 | y3]))        x0 = act1(cv1(x)); y1, y2, y3 = three chained MaxPool2d(5, 1, 2) of x0 (-inf padding)
 * x (N, h, w, c1) and y (N, h, w, c2): NHWC views, x with 16-byte and y with 8-byte aligned pixel / row / image strides (either may be a channel
 * slice of a wider buffer).  packed_w1 / bias1 = mgdt_conv_pack(c1, c1 / 2, 1, bf16) of cv1, packed_w2 / bias2 = mgdt_conv_pack(2 * c1, c2, 1, bf16)
 * of cv2.  The values are those of mgdt_conv2d_fwd into concat slot 0, mgdt_sppf_pool_fwd into slots 1..3 and mgdt_conv2d_fwd over the buffer,
 * bit for bit; the 2 * c1 channel buffer does not exist.
 * mgdt_sppf_fuse_supported: bf16, cm == c1 / 2, (c1, c2) in {(64, 64), (64, 96), (256, 256)}, activations none / SiLU / ReLU. */
int mgdt_sppf_fuse_supported(int c1, int cm, int c2, int h, int w, int act1, int act2, int dtype);
int mgdt_sppf_fuse_fwd(const mgdt_view* x, const void* packed_w1, const float* bias1, int act1, const void* packed_w2, const float* bias2, int act2,
                       const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- TOODHead (nn/modules/head.py:466-572; parity unpinned: mmcv's ModulatedDeformConv2d is not shipped with the reference) --------
 * GroupNorm + activation (Conv_GN head.py:67-81, DyDCNv2's norm block.py:427-431): y = act(group_norm(x, groups, gamma, beta, eps)).
 * ws: mgdt_groupnorm_workspace_bytes(n, c) bytes, 8-byte aligned (it holds the double partial sums; MGDT_BAD_ARG otherwise); x, y: 4-aligned NHWC views,
 * c <= 4096, h*w < 2^31 - 2^16 (MGDT_BAD_SHAPE otherwise). */
size_t mgdt_groupnorm_workspace_bytes(int n, int c);
int mgdt_groupnorm_fwd(const mgdt_view* x, const float* gamma, const float* beta, int groups, float eps, int act, void* ws, const mgdt_view* y,
                       int dtype, mgdt_stream s);
/* TaskDecomposition layer attention (head.py:107-123): sums[n][c] = sum_hw feat (mgdt_nc_reduce); w1 [hid][c], w2 [stacked][hid];
 * scale[n][k*feat + j] = sigmoid(w2 relu(w1 avg + b1) + b2)[k] - the per-(image, input channel) scale that turns the reduction
 * conv into mgdt_conv2d_fwd(in_scale = scale). */
int mgdt_tood_layer_attn_fwd(const float* sums, int n, int c, int hw, const float* w1, const float* b1, const float* w2, const float* b2, int hid,
                             int stacked, float* scale, mgdt_stream s);
/* DCNv2 3x3, stride 1, pad 1, one deform group (block.py:401-432, mmcv modulated_deform_conv): offset_mask = N x H x W x (>=27):
 * 18 offsets (dy, dx per kernel point) then 9 mask logits (sigmoid applied inside, head.py:525).  w_gemm [9*cin][cout] fp32
 * (mgdt_conv_pack_direct layout), bias fp32[cout] or NULL.  The weight tile of 16 output channels (9 * cin * 64 B) is held in LDS: cin <= 284,
 * MGDT_BAD_SHAPE beyond that before any launch. */
int mgdt_dcnv2_fwd(const mgdt_view* x, const mgdt_view* offset_mask, const float* w_gemm, const float* bias, const mgdt_view* y, int dtype,
                   mgdt_stream s);
/* The same on the MFMA path (bf16, cin % 8 == 0, cout in {16,32,48,64}, no bias): packed_w = mgdt_conv_pack(w, no BN, cin, cout, k = 3, bf16). */
int mgdt_dcnv2_mfma_fwd(const mgdt_view* x, const mgdt_view* offset_mask, const void* packed_w, const mgdt_view* y, int dtype, mgdt_stream s);
/* y = x * sigmoid(gate[n,h,w]) (cls_feat * cls_prob, head.py:536); gate: N x H x W x 1 logits. */
int mgdt_pixel_gate_fwd(const mgdt_view* x, const mgdt_view* gate, const mgdt_view* y, int dtype, mgdt_stream s);

/* ---- direct convolution (any strides/groups/cin; used for the 3-channel stem and odd shapes) ------------
 * Same math as above without the fused extras; x may be fp32 NCHW (x_dtype) while y is `dtype` NHWC.
 * Stem (k=3, cin<=4, cout%16==0): x_dtype may also be MGDT_U8 - the uint8 image is divided by 255 on the fly exactly as the
 * reference's preprocess does (yolo/engine/predictor.py:129, yolo/v8/detect/val.py:34, train.py:64), in fp32.
 * w_gemm: [k*k*cin/groups][cout] fp32 from mgdt_conv_pack_direct; bias fp32[cout].                         */
int mgdt_conv_pack_direct(const float* w_oihw, const float* conv_bias, const float* bn_gamma, const float* bn_beta,
                          const float* bn_mean, const float* bn_var, float bn_eps, int cin_g, int cout, int k,
                          float* w_out, float* bias_out, mgdt_stream s);
int mgdt_conv2d_direct_fwd(const mgdt_view* x, int x_dtype, const float* w_gemm, const float* bias, int k, int stride,
                           int groups, int act, const mgdt_view* y, int dtype, mgdt_stream s);
/* Host-side route query: what mgdt_conv2d_direct_fwd would launch for these views, without launching and without a device; the launch executes the plan
 * this reports.  Pointers are only tested for alignment (y's).  out[4] = {family, grid x, grid y, status}.  MGDT_DIRECT_STEM: k = 3, groups = 1,
 * cin <= 4, cout % 16 == 0, y NHWC with 16-byte aligned pixels (y->p % 16 == 0 and sw, sh, sn multiples of 4 fp32 / 8 bf16 elements), x_dtype fp32 /
 * uint8, or bf16 with a bf16 y; MGDT_DIRECT_GENERIC: everything else the call accepts; MGDT_DIRECT_REFUSED: status is what the call fails with. */
enum { MGDT_DIRECT_STEM = 0, MGDT_DIRECT_GENERIC = 1, MGDT_DIRECT_REFUSED = 2 };
int mgdt_conv2d_direct_route(const mgdt_view* x, int x_dtype, const mgdt_view* y, int dtype, int k, int stride, int groups, int* out);

/* ---- MSPA attention: SPRModule pooling + MLP + softmax over the 4 groups + scale ------------------------
 * nn/modules/spr_module.py:8-31, nn/modules/block.py:268-287.
 * pool: x (n,h,w,c) -> pooled fp32 [n][MGDT_SPR_SPLITS][c][5]: per row-band partial SUMS of {whole map, the four
 *       adaptive_avg_pool2d(2) bins (row-major)} (fixed reduction order: results are run-to-run identical);
 * attn: finishes the means, runs fc1/ReLU/fc2/sigmoid on each of the `groups` channel groups (shared weights,
 *       fc1_w [cw/4][5cw], fc2_w [cw][cw/4], cw = c/groups), softmax over the groups (softmax = 1; 0 = the bare sigmoid weights of
 *       SPRModule.forward, spr_module.py:20-31) -> attn fp32 [n][c];
 * scale: y = x * attn[n,c].                                                                               */
#define MGDT_SPR_SPLITS 16
int mgdt_spr_pool_fwd(const mgdt_view* x, float* pooled, int dtype, mgdt_stream s);
int mgdt_spr_attn_fwd(const float* pooled, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                      const float* fc2_b, int n, int c, int groups, int h, int w, int softmax, float* attn, mgdt_stream s);
int mgdt_scale_channels_fwd(const mgdt_view* x, const float* attn, const mgdt_view* y, int dtype, mgdt_stream s);
/* spr_attn + scale_channels in one launch: every workgroup recomputes its image's attention (same order, same bits) and scales
 * a share of the pixels: y = x * softmax_groups(SPR(pooled)).  `pooled` as written by mgdt_spr_pool_fwd (nsplit = MGDT_SPR_SPLITS, or 0)
 * with tiles_x = tiles_y = 0: fp32 [n][nsplit][c][5]; or the per-tile sums of mgdt_csp_block_fwd: fp32 [n][nsplit][c], tiles_x x tiles_y
 * its tile grid.  pool_a / pool_b (NULL or NHWC views of the same n, c with h = H / F, w = W / F, F integer): F x F average pools of y, bit-equal
 * to mgdt_adaptive_avgpool_fwd(y) - the SimFusion_4in / SimFusion_3in inputs of the GD neck (nn/modules/block.py:289-329), written by the
 * pass that has the map in hand instead of by pooling launches of their own. */
int mgdt_spr_attn_scale_fwd(const float* pooled, int nsplit, int tiles_x, int tiles_y, const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, int groups,
                            const mgdt_view* x, const mgdt_view* y, const mgdt_view* pool_a, const mgdt_view* pool_b, int dtype, mgdt_stream s);

/* ---- SPPF pooling: y1,y2,y3 = maxpool5(x), maxpool5(y1), maxpool5(y2) (nn/modules/block.py:138-153) ----- */
int mgdt_sppf_pool_fwd(const mgdt_view* x, const mgdt_view* y1, const mgdt_view* y2, const mgdt_view* y3, int dtype,
                       mgdt_stream s);

/* ---- resamplers (nn/modules/block.py:292,304,316,328,393-394; nn.Upsample in models/v8/yolov8.yaml) ---- */
int mgdt_adaptive_avgpool_fwd(const mgdt_view* x, const mgdt_view* y, int dtype, mgdt_stream s);
int mgdt_bilinear_fwd(const mgdt_view* x, const mgdt_view* y, int dtype, mgdt_stream s); /* align_corners=False */
int mgdt_nearest_fwd(const mgdt_view* x, const mgdt_view* y, int dtype, mgdt_stream s);
int mgdt_copy_fwd(const mgdt_view* x, int x_dtype, const mgdt_view* y, int y_dtype, mgdt_stream s);
/* The 1-3 channel image (any strides; MGDT_U8 is divided by 255: detect/train.py:64) as a 4-channel NHWC map whose remaining channels are zero - the input the
 * stem's weight-gradient kernel reads.  Writes all four channels of y. */
int mgdt_image_pad4_fwd(const mgdt_view* x, int x_dtype, const mgdt_view* y, int y_dtype, mgdt_stream s); /* cat / layout / cast */

/* ---- the 6x6 / stride 2 / padding 2 stem of the YOLOv5 graphs (models/v5/yolov5.yaml row 0) as space-to-depth + a 3x3 / stride 1 convolution:
 *   S[b, (dy*2+dx)*C + ci, i, j] = x[b, ci, 2i+dy, 2j+dx],  W3[co, (dy*2+dx)*C + ci, a, b] = W6[co, ci, 2a+dy, 2b+dx],
 *   conv2d(x, W6, stride 2, pad 2) == conv2d(S, W3, stride 1, pad 1)  (exact).
 * mgdt_space_to_depth2_fwd: x = N x C x H x W image, C <= 4, H and W even, any strides, x_dtype MGDT_F32 / MGDT_BF16 / MGDT_U8 (u8 divided by 255 like
 *   the other stem kernels); y = N x H/2 x W/2 x Cp NHWC, y_dtype MGDT_F32 / MGDT_BF16 (a bf16 image goes to bf16 only), 16-byte aligned, with
 *   Cp = mgdt_space_to_depth2_channels(C, y_dtype) = 4C rounded up to whole 16-byte stores (C = 3: 12 fp32, 16 bf16); channels 4C.. are written zero.
 * mgdt_stem6_wgrad_unpack: dw6 (fp32 [cout][cin][6][6], overwritten) <- dw3 (fp32 [cout][cp][3][3], cp >= 4 cin): the FINAL sums of the 3x3
 *   weight-gradient kernel over S, permuted back (rows 4 cin.. of dw3 - the pad channels - are not read).
 * mgdt_conv_pack_stem6: the panel of that 3x3 convolution (+ folded bias, as mgdt_conv_pack) read straight from the live 6x6 weight w6 fp32 [cout][c6][6][6],
 *   zero rows for the pad channels; sized by mgdt_conv_packed_bytes(mgdt_space_to_depth2_channels(c6, dtype), cout, 3, dtype); refreshed in place by
 *   mgdt_conv_pack_batch descriptors of mode 5 + c6. */
int mgdt_space_to_depth2_channels(int c, int y_dtype);
int mgdt_conv_pack_stem6(const float* w6, const float* conv_bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                         float bn_eps, int c6, int cout, int dtype, void* packed_out, float* bias_out, mgdt_stream s);
int mgdt_space_to_depth2_fwd(const mgdt_view* x, int x_dtype, const mgdt_view* y, int y_dtype, mgdt_stream s);
int mgdt_stem6_wgrad_unpack(const float* dw3, int cout, int cin, int cp, float* dw6, mgdt_stream s);

/* ---- ConvNeXtV2 block pieces (nn/modules/convnextv2.py:48-77, nn/modules/utils.py:145-182) -------------
 * dwln: y = LayerNorm_c(dwconv7x7(x) + b) * ln_w + ln_b   (eps 1e-6), dw_w is [49][c] fp32.
 * grn_stats: t (n,h,w,c) -> scale[n][c] = gamma[c]*Nx[n,c] + 1, with Nx = ||t||_2(h,w) / (mean_c + 1e-6);
 *            ws: fp32 [n][MGDT_GRN_SPLITS][c] scratch (per pixel-band partial sums, fixed reduction order).
 *            (shift[c] = beta[c] is passed to mgdt_conv2d_fwd directly.)                                   */
#define MGDT_GRN_SPLITS 8
int mgdt_dwconv7_ln_fwd(const mgdt_view* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                        float eps, const mgdt_view* y, int dtype, mgdt_stream s);
int mgdt_grn_stats_fwd(const mgdt_view* t, const float* gamma, float* ws, float* scale, int dtype, mgdt_stream s);
/* mgdt_dwconv7_ln_route: the launch mgdt_dwconv7_ln_fwd / mgdt_dwconv7_ln_train_fwd would make for an n x h x w map of c channels, without launching
 * anything (no device needed): out[5] = {family, tile side (0: generic), workgroups, dynamic LDS bytes, threads per workgroup}.  Families: the row
 * kernel with 8x8 or 10x10 tiles (bf16 c <= 100, fp32 c <= 60; 10x10 where 8x8 tiles need another round of workgroups over the chip, or do not fit),
 * the generic one-pixel-per-thread-row kernel otherwise.  MGDT_BAD_SHAPE for a shape the forward call refuses. */
enum { MGDT_DW_ROW8 = 0, MGDT_DW_ROW10 = 1, MGDT_DW_GENERIC = 2 };
int mgdt_dwconv7_ln_route(int n, int h, int w, int c, int dtype, int* out);

/* ---- InjectionMultiSum_Auto_pool tail (nn/modules/block.py:381-399) --------------------------------------
 * up branch  (local >= global size): y = local * bilinear(relu6(ga+3)/6) + bilinear(gf)
 * pool branch (local <  global size): y = local * avgpool(ga) + avgpool(gf)   (no h_sigmoid, as written)  */
int mgdt_inject_fwd(const mgdt_view* local, const mgdt_view* ga, const mgdt_view* gf, const mgdt_view* y, int dtype,
                    mgdt_stream s);

/* ---- Detect eval tail (nn/modules/head.py:165-177; DFL block.py:36-54; tal.py:476-500) ------------------
 * feat: one level (n,h,w,4R+nc) raw head map; writes y[n][4+nc][a_total] at anchor offset a_off:
 * xywh = dist2bbox(softmax_R . arange(R), anchor(+0.5)) * stride, cls = sigmoid.  y is fp32.              */
int mgdt_detect_decode_fwd(const mgdt_view* feat, int reg_max, int nc, float stride, int a_off, int a_total, float* y,
                           int dtype, mgdt_stream s);
/* The same decode with the test-time augmentation epilogue of mgdt_detect_tail_aug_fwd (xywh /= aug_scale, x = aug_img_w - x when aug_flip);
 * best_keys: NULL, or [N][a_total] - the NMS key of every anchor's best class, as mgdt_detect_tail_fwd writes it. */
int mgdt_detect_decode_aug_fwd(const mgdt_view* feat, int reg_max, int nc, float stride, int a_off, int a_total, float* y,
                               unsigned long long* best_keys, float aug_scale, int aug_flip, float aug_img_w, int dtype, mgdt_stream s);

/* ---- batched NMS (yolo/utils/ops.py:136-266 incl. the torchvision.ops.nms call at :249) -----------------
 * pred fp32 [n][4+nc][a].  Outputs per image: out[n][max_det][6] fp32 rows (x1,y1,x2,y2,conf,cls),
 * kept_anchor[n][max_det] int32 (anchor index of each kept row), counts[n] int32.  classes: optional int32
 * list (NULL = all).  Ties in score: lower candidate index first.  ws from mgdt_nms_workspace_bytes.
 * best_keys: NULL, or [n][a] 64-bit keys ((0xFFFFFFFF - bits(best score)) << 32 | anchor * nc + first best class) of EVERY anchor as
 * mgdt_detect_tail_fwd writes them next to pred: the best-class scan over pred (ops.py:225-226) is then skipped (ignored for multi_label). */
size_t mgdt_nms_workspace_bytes(int n, int nc, int a, int multi_label, int max_nms);
int mgdt_nms_fwd(const float* pred, int n, int nc, int a, float conf_thres, float iou_thres, const int32_t* classes,
                 int n_classes, int agnostic, int multi_label, int max_det, int max_nms, float max_wh, float* out,
                 int32_t* kept_anchor, int32_t* counts, const unsigned long long* best_keys, void* ws, size_t ws_bytes, mgdt_stream s);

/* The same selection on a prediction that carries nm mask-coefficient rows behind the class rows (yolo/utils/ops.py:136-266 with nm > 0):
 * pred fp32 [n][4+nc+nm][a]; candidates, ordering and suppression read rows 0 .. 4+nc only (the code of mgdt_nms_fwd with another image stride);
 * out[n][max_det][6+nm]: columns 6.. are the kept anchor's coefficients, copied.  nm = 0 is mgdt_nms_fwd. */
int mgdt_nms_masks_fwd(const float* pred, int n, int nc, int nm, int a, float conf_thres, float iou_thres, const int32_t* classes,
                       int n_classes, int agnostic, int multi_label, int max_det, int max_nms, float max_wh, float* out,
                       int32_t* kept_anchor, int32_t* counts, const unsigned long long* best_keys, void* ws, size_t ws_bytes, mgdt_stream s);

/* ---- instance segmentation inference (nn/modules/head.py:189-212 Segment, nn/modules/block.py:57-69 Proto, yolo/utils/ops.py:541-636) -----------
 * deconv2x2: nn.ConvTranspose2d(cin, cout, 2, 2, 0) + bias (Proto.upsample; kernel == stride, so y[2i+dy][2j+dx] = W[:, :, dy, dx]^T x[i][j] + b):
 *   packed4[2*dy + dx] = mgdt_conv_pack of the (cout, cin, 1, 1) matrix W[:, :, dy, dx]^T, bias = any of the four packs' bias_out (the conv bias);
 *   four launches of the MFMA kernel of mgdt_conv2d_fwd, each writing one stride-2 phase of y (N x 2H x 2W x cout NHWC).  Other geometries are
 *   not built.
 * seg_concat: y fp32 [n][rows][a] (rows = 4 + nc, as Detect writes it) + the per-level cv4 maps mc[l] (n x h_l x w_l x nm NHWC, `dtype`) ->
 *   out fp32 [n][rows+nm][a]: rows 0..rows copied, row rows+k of anchor a_off_l + pixel = mc[l][pixel][k] (head.py:208,212).
 * seg_masks: crop_mask / process_mask / process_mask_upsample / process_mask_native for a whole batch in one launch.  protos: n x mh x mw x nm
 *   NHWC (nm = 32), rows [n][max_det][6+nm] + counts[n] as mgdt_nms_masks_fwd writes them, offsets[n] = exclusive scan of counts (device);
 *   out [sum(counts)][out_h][out_w] of 0 / 1, uint8 (out_u8) or fp32, every element written, nothing past it.
 *     masks = sigmoid(rows[:, 6:] @ protos[top:top+win_h, left:left+win_w])          (MFMA; bf16: coefficients rounded to bf16, fp32 accumulation)
 *     crop_before: zero where the proto pixel (x, y) fails x >= x1*box_sx, x < x2*box_sx, y >= y1*box_sy, y < y2*box_sy     (fp32, ops.py:541-557)
 *     bilinear resample of the window to out_h x out_w (align_corners=False, PyTorch's CPU arithmetic; identity when the sizes agree)
 *     crop_after: zero where the output pixel fails the same test on the unscaled box;  then > 0.5.
 *   process_mask(upsample=False): window = whole map, out = mh x mw, crop_before with (mw/iw, mh/ih);  (upsample=True): the same with out = ih x iw;
 *   process_mask_upsample: out = ih x iw, crop_after;  process_mask_native: window from the letter-box gain / pad (ops.py:628-632), crop_after.
 *   no_skip: compute every (detection, tile) pair even when its crop box misses the tile (tests: the skip changes no byte).
 *   mgdt_seg_mask_geometry: geom4 = {tile_h, tile_w, tiles_y, tiles_x} of that launch; 0 when the resampling ratio is not covered. */
int mgdt_deconv2x2_fwd(const mgdt_view* x, const void* const* packed4, const float* bias, const mgdt_view* y, int dtype, mgdt_stream s);
/* nn.ConvTranspose2d(cin, cout, 2, 2, 0) as a layer that trains (models/v6/yolov6.yaml rows 11, 16), weight w fp32 [cin][cout][2][2] in place:
 * mgdt_conv_pack_deconv2x2: panel `phase` = 2*ky + kx of mgdt_deconv2x2_fwd (+ bias_out = the bias, padded) read straight from the live weight, sized by
 *   mgdt_conv_packed_bytes(cin, cout, 1, dtype); refreshed in place by mgdt_conv_pack_batch descriptors of mode 10 + phase.
 * mgdt_conv_pack_deconv2x2_dgrad: panel `phase` of the layer's data gradient as a 1x1 convolution cout -> cin over the stride-2 phase view of dy (the composed
 *   route: dx = sum over the phases of mgdt_conv2d_fwd(x = dy[:, ky::2, kx::2], packed(phase), k 1, y = dx, r1 = dx from the second phase on)), read from the
 *   live weight, bias_out zeroed; sized by mgdt_conv_packed_bytes(cout, cin, 1, dtype); refreshed by mgdt_conv_pack_batch descriptors of mode 14 + phase.
 * mgdt_deconv2x2_dgrad: dx[b, y, x, ci] = sum_{ky, kx, co} w[ci][co][ky][kx] * dy[b, 2y+ky, 2x+kx, co] [+ r1] [+ r2]: one GEMM with K = 4 cout on the
 *   fp32 matrix cores (bf16 values widened exactly, fp32 accumulation, one fixed summation order).  dy = N x 2H x 2W x cout, dx / r1 / r2 = N x H x W x cin,
 *   all NHWC of `dtype` with channels % 4 == 0; dy's strides % 4 == 0 and its base aligned to 4 elements.  r1 may be dx itself (accumulate).
 *   MGDT_BAD_SHAPE when w's tile for 16 input channels exceeds 64 KB of LDS (cout > 240).
 * mgdt_deconv2x2_wgrad: dw[ci][co][ky][kx] = sum_{b, y, x} x[b, y, x, ci] * dy[b, 2y+ky, 2x+kx, co], fp32, in the parameter's layout.  Pixel splits leave
 *   partial sums in ws (fp32 [mgdt_deconv2x2_wgrad_splits][cin][cout][2][2], mgdt_deconv2x2_wgrad_workspace_bytes); dw != NULL: their sum is written
 *   (accumulate: added) by one mgdt_wgrad_final_batch job; dw == NULL: partial sums only, for a later mgdt_wgrad_final_batch with n = 4 cin cout and
 *   nsplit = mgdt_deconv2x2_wgrad_splits(cin, cout) - the same bits.  x and dy as above, both with strides % 4 == 0 and aligned bases. */
int mgdt_conv_pack_deconv2x2(const float* w, const float* bias, int cin, int cout, int phase, int dtype, void* packed_out, float* bias_out, mgdt_stream s);
int mgdt_conv_pack_deconv2x2_dgrad(const float* w, int cin, int cout, int phase, int dtype, void* packed_out, float* bias_out, mgdt_stream s);
int mgdt_deconv2x2_dgrad(const mgdt_view* dy, const float* w, const mgdt_view* r1, const mgdt_view* r2, const mgdt_view* dx, int dtype, mgdt_stream s);
int mgdt_deconv2x2_wgrad_splits(int cin, int cout);
size_t mgdt_deconv2x2_wgrad_workspace_bytes(int cin, int cout);
int mgdt_deconv2x2_wgrad(const mgdt_view* x, const mgdt_view* dy, float* dw, int accumulate, void* ws, int dtype, mgdt_stream s);
int mgdt_seg_concat_fwd(const float* y, int n, int rows, int a_total, const mgdt_view* const* mc, int n_levels, int nm, float* out, int dtype,
                        mgdt_stream s);
int mgdt_seg_mask_geometry(int win_h, int win_w, int out_h, int out_w, int* geom4);
int mgdt_seg_masks_fwd(const mgdt_view* protos, const float* rows, const int32_t* counts, const int32_t* offsets, int max_det, int nm,
                       int top, int left, int win_h, int win_w, int out_h, int out_w, int crop_before, float box_sx, float box_sy,
                       int crop_after, int no_skip, void* out, int out_u8, int dtype, mgdt_stream s);

/* ---- pose-estimation inference (nn/modules/head.py:215-253 Pose, yolo/v8/pose/predict.py:16-41, yolo/utils/ops.py:636-666) -----------------------
 * pose_concat: y fp32 [n][rows][a] (rows = 4 + nc, as Detect writes it) + the per-level cv4 maps kpt[l] (n x h_l x w_l NHWC of `dtype`, at least nk
 *   channels per pixel - the pixel stride may exceed nk: the zero-padded MFMA route leaves 52 channels for nk = 51) and the levels' strides[l] (host) ->
 *   out fp32 [n][rows+nk][a]: rows 0..rows copied, row rows+k of anchor a_off_l + pixel (x, y) decoded from v = kpt[l][pixel][k] as kpts_decode's
 *   non-export branch does in fp32: k % ndim == 0: (v*2 + ((x + 0.5) - 0.5)) * stride, == 1: the same with y, == 2 (ndim 3): sigmoid(v);
 *   kpt_raw fp32 [n][nk][a] = the v themselves (the `kpt` the head returns next to the feature maps).  nk <= 240, ndim in {2, 3}, <= 4 levels.
 * pose_scale: PosePredictor.postprocess after the NMS, in place on rows [n][max_det][lead+nk] for the first min(counts[i], max_det) rows of image i;
 *   lead = 6: the layout mgdt_nms_masks_fwd writes, lead = 0: bare keypoint coordinates (scale_coords / clip_coords alone).  meta fp32 [n][8] =
 *   {gain, kpt_pad_x, kpt_pad_y, h0, w0, box_pad_x, box_pad_y, normalize} (device), gain / pads from the host exactly as scale_coords (fractional pads)
 *   and scale_boxes (rounded pads) compute them.  Columns 0..4 (lead = 6): clip((v - box_pad) / gain, 0, w0 | h0), then round half-to-even (torch.round);
 *   columns lead + k with k % ndim == 0 / 1: clip((v - kpt_pad) / gain, 0, w0 | h0), divided by w0 | h0 when normalize != 0; every other column untouched. */
int mgdt_pose_concat_fwd(const float* y, int n, int rows, int a_total, const mgdt_view* const* kpt, const float* strides, int n_levels, int nk,
                         int ndim, float* out, float* kpt_raw, int dtype, mgdt_stream s);
int mgdt_pose_scale_fwd(float* rows, const int32_t* counts, const float* meta, int n, int max_det, int lead, int nk, int ndim, mgdt_stream s);

/* ---- instance-segmentation validation (reference yolo/v8/segment/val.py:131-166, yolo/utils/metrics.py:131-147 mask_iou) -------------
 * mask_iou: iou [n][max_lab][max_det] fp32 of every (label, detection) pair of a batch in one call (a clear of the workspace, the i8 MFMA kernel,
 *   a small final pass).  pred: uint8 0 / 1 masks [sum(counts)][hw] exactly as mgdt_seg_masks_fwd writes them, with its device counts[n] / offsets[n]
 *   (counts are clamped to max_det).  Ground truth, gt_index_map != 0 (the reference's overlap_mask=True): gt uint8 [n][hw], pixel value j + 1 belongs to
 *   label j of that image, 0 is background (lab_offsets may be NULL); gt_index_map == 0: instance masks uint8 [sum(nlab)][hw] with nlab[n] and
 *   lab_offsets[n].  Intersections and areas are exact integers; iou = inter / ((area_gt + area_pred) - inter + eps) in fp32 with an IEEE division.
 *   Entries with label >= nlab[i] or detection >= counts[i] are WRITTEN as 0.  ws: mgdt_mask_iou_workspace_bytes(n, max_det, max_lab) bytes.
 *   Limits (MGDT_BAD_SHAPE before any launch): n <= 65535, max_det <= 1024, max_lab <= 256 (255 as an index map), hw <= 2^24,
 *   n * max_lab * max_det < 2^31.
 * gt_masks_resample: the ground truth of either form resampled to out_h x out_w as the reference does when the sizes differ (each binary mask:
 *   bilinear, align_corners=False, > 0.5), written as instance masks uint8 [sum(nlab)][out_h][out_w] at lab_offsets.  Same limits; h*w, out_h*out_w <= 2^24.
 * val_match_iou: the matching rule of mgdt_val_match_fwd on a given iou [n][max_lab][max_det]: det_cls / lab_cls point at the class of detection /
 *   label 0 of image 0, consecutive rows det_stride / lab_stride floats apart (images max_det * det_stride / max_lab * lab_stride apart), so the
 *   rows of mgdt_nms_masks_fwd (class at column 5) and [cls, box] labels (column 0) are read in place.  correct [n][max_det][n_iou] uint8. */
size_t mgdt_mask_iou_workspace_bytes(int n, int max_det, int max_lab);
int mgdt_mask_iou_fwd(const uint8_t* pred, const int32_t* counts, const int32_t* offsets, int n, int max_det, const uint8_t* gt, int gt_index_map,
                      const int32_t* nlab, const int32_t* lab_offsets, int max_lab, int hw, float eps, float* iou, void* ws, size_t ws_bytes,
                      mgdt_stream s);
int mgdt_gt_masks_resample_fwd(const uint8_t* gt, int gt_index_map, const int32_t* nlab, const int32_t* lab_offsets, int n, int max_lab, int h, int w,
                               int out_h, int out_w, uint8_t* out, mgdt_stream s);
int mgdt_val_match_iou_fwd(const float* iou, int n, int max_lab, int max_det, const float* det_cls, int det_stride, const int32_t* ndet,
                           const float* lab_cls, int lab_stride, const int32_t* nlab, const float* iouv, int n_iou, uint8_t* correct, mgdt_stream s);

/* ---- pose validation (reference yolo/utils/metrics.py:150-169 kpt_iou, yolo/v8/pose/val.py:110-141) ------------------------------------
 * kpt_iou: oks [n][max_lab][max_det] fp32, the object keypoint similarity of every (label, detection) pair of a batch in one launch, laid out like
 *   mgdt_mask_iou_fwd's matrix (mgdt_val_match_iou_fwd consumes it unchanged).  pred: keypoint 0 of detection 0 of image 0; detection d of image i
 *   starts (i * max_det + d) * pred_stride floats further and holds nkpt keypoints of pred_ndim (2 or 3) floats [x, y(, visibility)]: for the rows
 *   [n][max_det][6 + nk] of mgdt_nms_masks_fwd pass rows + 6 and 6 + nk, for a dense [n][max_det][nkpt][pred_ndim] tensor nkpt * pred_ndim.  Only the
 *   keypoint floats of the first min(counts[i], max_det) detections are read.  gt_kpts fp32 [n][max_lab][nkpt][3] (x, y, visibility; zero-padded),
 *   area fp32 [n][max_lab], nlab int32 [n], sigma fp32 [nkpt].  With d = dx^2 + dy^2 of label and detection keypoint k (each operation rounded):
 *   oks = sum_k exp(-d / (2 sigma_k)^2 / (area + eps) / 2) [vis_k != 0] / (sum_k [vis_k != 0] + eps), computed as exp(-d * coef) with
 *   coef = 1 / ((2 sigma_k)^2 (area + eps) 2) and multiplied by 1 / (count + eps).  A label without a visible keypoint gives 0; a zero-area label gives
 *   no NaN for eps > 0 (0 where d > 0, a term of 1 where d = 0).  Entries with label >= nlab[i] or detection >= counts[i] are WRITTEN as 0.
 *   Limits (MGDT_BAD_SHAPE before any launch): n <= 65535, max_det <= 1024, max_lab <= 256, nkpt <= 120, pred_ndim in {2, 3},
 *   nkpt * pred_ndim <= pred_stride <= 2^20, n * max_lab * max_det < 2^31. */
int mgdt_kpt_iou_fwd(const float* pred, int pred_stride, int pred_ndim, const int32_t* counts, int n, int max_det, const float* gt_kpts,
                     const float* area, const int32_t* nlab, int max_lab, int nkpt, const float* sigma, float eps, float* oks, mgdt_stream s);

/* ---- validator matching: DetectionValidator._process_batch, yolo/v8/detect/val.py:152-175, for a batch ----------
 * det [n][max_det][6] (x1,y1,x2,y2,conf,cls; the layout mgdt_nms_fwd writes) with ndet[n] valid rows, labels [n][max_lab][5]
 * (cls,x1,y1,x2,y2 in the same pixel frame) with nlab[n] valid rows, iouv[n_iou] ascending IoU levels (n_iou <= 16).
 * correct [n][max_det][n_iou] uint8: 1 where the detection is a true positive at that level (rows past ndet are 0). */
int mgdt_val_match_fwd(const float* det, const int32_t* ndet, int n, int max_det, const float* labels, const int32_t* nlab, int max_lab,
                       const float* iouv, int n_iou, uint8_t* correct, mgdt_stream s);

/* ---- validator statistics beyond mAP: confusion matrix + counting metrics, one launch per batch ----------------------------------------
 * det / ndet / labels / nlab as mgdt_val_match_fwd takes them, in one native pixel frame.  Both outputs are ADDED to with integer atomics (the caller
 * clears them once per validation run; replays are bit-equal); either may be NULL, not both.
 * matrix int32 [(nc+1)][(nc+1)], row = predicted class, column = true class, index nc = background: ConfusionMatrix.process_batch
 *   (yolo/utils/metrics.py:209-253) per image.  Detections with conf > cm_conf; pairs with box_iou > cm_iou (fp32, the operation order of
 *   mgdt_val_match_fwd); each detection keeps its highest-IoU label, each label the highest-IoU detection among those that chose it (the two
 *   np.unique of the reference, NOT a greedy matching).  A label with a winner adds matrix[cls(det)][cls(label)], another matrix[nc][cls(label)];
 *   a kept detection that won no label adds matrix[cls(det)][nc], but only in an image with at least one match (the reference's `if n:`).
 * counts int64 [nc][MGDT_COUNT_SLOTS]: nn/cal_counting_metrics.py:70-121 for nc classes.  Per image and class c: t labels, p detections with
 *   conf > cnt_conf; each label takes the FIRST such detection in NMS order with IoU > cnt_iou (a detection may serve several labels); TP per
 *   match, FN per label without, FP = p - distinct matched detections.  The IoU is the script's (max(0, .) on both sides, 0 unless union > 0),
 *   in fp32, on label corners truncated toward zero when cnt_trunc_labels != 0 (the script's int()).
 *   Slots: images, sum t, sum p, sum t^2, sum t*p, sum (t-p)^2, sum |t-p|, TP, FP, FN.
 * Classes are the float columns truncated toward zero; a row whose class is outside [0, nc) adds nothing.  Exact IoU ties resolve to the lower index.
 * Limits (MGDT_BAD_SHAPE before any launch): n <= 65535, max_det <= 1024, max_lab <= 256, nc <= 4096. */
#define MGDT_COUNT_SLOTS 10
int mgdt_val_confusion_fwd(const float* det, const int32_t* ndet, int n, int max_det, const float* labels, const int32_t* nlab, int max_lab,
                           int nc, float cm_conf, float cm_iou, float cnt_conf, float cnt_iou, int cnt_trunc_labels, int32_t* matrix,
                           int64_t* counts, mgdt_stream s);

/* ---- v8DetectionLoss: assigner + BCE/CIoU/DFL + gradient w.r.t. the head maps -----------------------------------------
 * yolo/utils/loss.py:108-208 (v8DetectionLoss.__call__, BboxLoss :56-89), yolo/utils/tal.py:56-353
 * (HeuristicPositiveSampleAssigner_v1 -> TaskAlignedAssigner, topk 10, alpha = 0.5*(100 - call_count/161)/100, beta 8),
 * yolo/utils/metrics.py:75-128 (CIoU).  feats[l]: raw head map of level l, NHWC view (B, 4R+nc, H, W); gt: fp32
 * [B][n_gt][5] = (cls, x1, y1, x2, y2) in pixels, zero rows = padding (what loss.py:132-148 `preprocess` builds).
 * out5 (device) = {loss*B, box, cls, dfl (gains applied), target_scores_sum}.  Optional device outputs (may be NULL):
 * fg_out uint8 [B][A], gt_idx_out int32 [B][A], tscore_out fp32 [B][A] (the normalised target score of the assigned class).
 * Top-k ties: lower anchor index first.  n_gt == 0: all-background targets (the reference raises here, tal.py:102-108).
 * bwd: grads[l] = gscale * d(loss*B)/d feats[l]; call after fwd with the same ws / out5 / arguments.                    */
size_t mgdt_detect_loss_workspace_bytes(int b, int a_total, int n_gt);
int mgdt_detect_loss_fwd(const mgdt_view* const* feats, const float* strides, int n_levels, int reg_max, int nc,
                         const float* gt, int n_gt, int call_count, float gain_box, float gain_cls, float gain_dfl,
                         float* out5, unsigned char* fg_out, int32_t* gt_idx_out, float* tscore_out, void* ws,
                         size_t ws_bytes, int dtype, mgdt_stream s);
/* The same with the per-call counter in device memory (a training step captured in a hipGraph; the host advances the counter between
 * replays).  Reference: the `epoch` argument of TaskAlignedAssigner.forward, yolo/utils/loss.py:195-206, tal.py:110,266-267. */
int mgdt_detect_loss_fwd_dev(const mgdt_view* const* feats, const float* strides, int n_levels, int reg_max, int nc,
                             const float* gt, int n_gt, const int32_t* call_count_dev, float gain_box, float gain_cls, float gain_dfl,
                             float* out5, unsigned char* fg_out, int32_t* gt_idx_out, float* tscore_out, void* ws,
                             size_t ws_bytes, int dtype, mgdt_stream s);
int mgdt_detect_loss_bwd(const mgdt_view* const* feats, const mgdt_view* const* grads, const float* strides, int n_levels,
                         int reg_max, int nc, const float* gt, int n_gt, float gain_box, float gain_cls, float gain_dfl,
                         float gscale, const float* out5, void* ws, size_t ws_bytes, int dtype, mgdt_stream s);

/* ---- training side: BatchNorm2d (batch statistics) + activation, its backward, conv dgrad / wgrad, adjoints ----------------
 * Conv.forward in training mode (nn/modules/conv.py:36-38: act(bn(conv(x))) with nn.BatchNorm2d eps 1e-3 / momentum 0.03,
 * yolo/utils/torch_utils.py:254-256) and what torch.autograd derives from it in trainer.py:343 (`scaler.scale(loss).backward()`).
 * ws: mgdt_reduce_workspace_bytes(c) / mgdt_conv_wgrad_workspace_bytes(cin, cout, k) bytes; all reductions have a fixed order.  */
size_t mgdt_reduce_workspace_bytes(int c);
int mgdt_bn_stats_fwd(const mgdt_view* y, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                      float* running_var, void* ws, int dtype, mgdt_stream s);
int mgdt_bn_act_fwd(const mgdt_view* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                    const mgdt_view* r1, const mgdt_view* r2, const mgdt_view* z, int dtype, mgdt_stream s);
int mgdt_bn_act_bwd(const mgdt_view* gz, const mgdt_view* y, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, int act, float* dgamma, float* dbeta, const mgdt_view* dy, void* ws, int dtype, mgdt_stream s);
int mgdt_conv_dgrad(const mgdt_view* dy, const float* w_oihw, int k, int stride, const mgdt_view* dx, int accumulate, int dtype,
                    mgdt_stream s);
/* Grouped / depth-wise convolution (the reference's DWConv, nn/modules/conv.py:82-86; Conv with g > 1): data and weight gradients.
   w / dw: [cout][cin/groups][k][k] fp32 (nn.Conv2d's layout); NHWC views; plain VALU kernels (no target YAML instantiates a grouped conv). */
int mgdt_gconv_dgrad(const mgdt_view* dy, const float* w, int k, int stride, int groups, const mgdt_view* dx, int accumulate, int dtype,
                     mgdt_stream s);
size_t mgdt_gconv_wgrad_workspace_bytes(int cin, int cout, int k, int groups);
int mgdt_gconv_wgrad(const mgdt_view* x, const mgdt_view* dy, int k, int stride, int groups, float* dw, int accumulate, void* ws, int dtype,
                     mgdt_stream s);
size_t mgdt_conv_wgrad_workspace_bytes(int cin, int cout, int k);
int mgdt_conv_wgrad(const mgdt_view* x, const mgdt_view* x2, const mgdt_view* dy, int k, int stride, float* dw_oihw, float* dbias,
                    int accumulate, void* ws, int dtype, mgdt_stream s);
/* Deferred final sums: mgdt_conv_wgrad with dw_oihw == NULL (and dbias == NULL) leaves its per-split partial sums in ws
 * ([mgdt_conv_wgrad_splits(cin, cout, k)][cout][cin][k*k] fp32); mgdt_wgrad_final_batch then finishes many convolutions in one launch, each in the
 * same fixed order as the immediate form (the results are bit-identical).  The caller keeps every ws alive until the batch has run. */
int mgdt_conv_wgrad_splits(int cin, int cout, int k);
typedef struct mgdt_wgrad_final_desc { const float* partial; float* dw; long n; int32_t nsplit; int32_t accumulate; } mgdt_wgrad_final_desc;
int mgdt_wgrad_final_batch(const mgdt_wgrad_final_desc* descs, int n, mgdt_stream s);
int mgdt_add_fwd(const mgdt_view* a, const mgdt_view* b, const mgdt_view* o, int dtype, mgdt_stream s);
int mgdt_maxpool5_bwd(const mgdt_view* x, const mgdt_view* gy, float* gx_f32, int dtype, mgdt_stream s);
int mgdt_nearest_bwd(const mgdt_view* gy, const mgdt_view* gx, int dtype, mgdt_stream s);
/* nn.MaxPool2d(2, stride) with stride 1 or 2, padding 0, dilation 1, ceil_mode False (models/v3/yolov3-tiny.yaml), pool.hip.  x, y, gy, gx: NHWC views with
 * any sn / sh / sw (a channel slice of a wider buffer, the interior of a padded map); y / gy = n x ((h - 2) / stride + 1) x ((w - 2) / stride + 1) x c, gx =
 * the shape of x.  16-byte accesses along c where c, the strides and the bases allow (c % 8 in bf16, c % 4 in fp32), one element per lane otherwise.
 * A NaN in a window is its maximum.  bwd recomputes the argmax from x (the first maximum in (ky, kx) order, a NaN replaces what came before; -0.0 == 0.0)
 * and GATHERS: every input pixel sums gy over the windows that hold it and whose argmax it is, in (oy, ox) order - no atomics, bit-reproducible; the
 * odd trailing row / column that stride 2 never reads gets 0.  gx is written in `dtype`, every element.  MGDT_BAD_ARG: null / empty view, another kernel
 * or stride; MGDT_BAD_SHAPE: views that are not NHWC or whose sizes do not match (an input smaller than 2 x 2 included); nothing is launched then.
 * mgdt_spp_pool_bwd: gx_f32 (dense fp32 [n][h][w][c], every element written) = sum over k in (5, 9, 13) of the adjoint of MaxPool2d(k, 1, k / 2) at x
 * applied to g_k - SPP's three DIRECT windows (nn/modules/block.py:121-135), whose first maximum is not the one a chain of 5 x 5 pools routes to.  One
 * launch; fixed summation order (5, 9, 13; per size ox ascending, within it oy ascending).  The plane sits in LDS up to 1638 pixels (40 x 40), a
 * global-memory route with the same bits serves larger maps.  x, g5, g9, g13: NHWC views of one shape, any sn / sh / sw. */
int mgdt_maxpool2d_fwd(const mgdt_view* x, const mgdt_view* y, int k, int stride, int dtype, mgdt_stream s);
int mgdt_maxpool2d_bwd(const mgdt_view* x, const mgdt_view* gy, const mgdt_view* gx, int k, int stride, int dtype, mgdt_stream s);
int mgdt_spp_pool_bwd(const mgdt_view* x, const mgdt_view* g5, const mgdt_view* g9, const mgdt_view* g13, float* gx_f32, int dtype, mgdt_stream s);

/* adjoints of the MSPA pooling attention and GD-neck ops (block.py:209-399, spr_module.py, convnextv2.py:48-77, utils.py:145-182) */
int mgdt_ew_binary(const mgdt_view* a, const mgdt_view* b, const mgdt_view* o, int mode, int dtype, mgdt_stream s);
int mgdt_channel_affine(const mgdt_view* x, const float* scale, const float* shift, const mgdt_view* y, int dtype, mgdt_stream s);
size_t mgdt_nc_reduce_workspace_bytes(int n, int c);
int mgdt_nc_reduce(const mgdt_view* a, const mgdt_view* b, float* out, void* ws, int dtype, mgdt_stream s);
int mgdt_adaptive_avgpool_bwd(const mgdt_view* gy, const mgdt_view* gx, int accumulate, int dtype, mgdt_stream s);
int mgdt_bilinear_bwd(const mgdt_view* gy, const mgdt_view* gx, int accumulate, int dtype, mgdt_stream s);
size_t mgdt_spr_bwd_workspace_bytes(int n, int c, int groups);
int mgdt_spr_bwd(const mgdt_view* gy, const float* pooled_partial, int splits, const float* attn, const float* dattn,
                 const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, int groups,
                 const mgdt_view* gx, float* param_grads, void* ws, int dtype, mgdt_stream s);
int mgdt_dwconv7_ln_train_fwd(const mgdt_view* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                              float eps, const mgdt_view* y, const mgdt_view* u_out, int dtype, mgdt_stream s);
size_t mgdt_dwconv7_ln_bwd_workspace_bytes(int c);
int mgdt_dwconv7_ln_bwd(const mgdt_view* x, const mgdt_view* u, const mgdt_view* gy, const float* dw_w49c, const float* ln_w, float eps,
                        const mgdt_view* du_tmp, const mgdt_view* dx, int accumulate_dx, float* d_dw_w, float* d_dw_b,
                        float* d_ln_w, float* d_ln_b, void* ws, int dtype, mgdt_stream s);
int mgdt_grn_bwd(const mgdt_view* g, const mgdt_view* t, const float* S, const float* A, const float* B, const float* gamma,
                 const mgdt_view* dt, float* dgamma, float* dbeta, void* ws, int dtype, mgdt_stream s);

/* ---- optimizer step on the flat parameter buffer (yolo/engine/trainer.py:462-470,633-664; torch_utils.py:335-367) ----------
 * clip: out2 = {total grad norm, min(1, max_norm/(norm+1e-6))} on device (no host sync); sgd: torch.optim.SGD(nesterov) with a
 * per-element weight-decay vector (0 for norm weights; a negative entry marks the bias group of trainer.py:644: no decay, stepped
 * with `lr_bias`, the warm-up bias learning rate of trainer.py:323) and the clip coefficient read from device memory.        */
size_t mgdt_grad_norm_workspace_bytes(void);
int mgdt_grad_clip_coef(const float* g, long n, float max_norm, float* out2, void* ws, mgdt_stream s);
int mgdt_sgd_step(float* p, const float* g, float* buf, const float* wd, long n, float lr, float lr_bias, float momentum, int nesterov,
                  int first, const float* clip2, mgdt_stream s);
int mgdt_ema_update(float* ema, const float* p, long n, float decay, mgdt_stream s);
/* SGD + EMA in one launch, scalars from device memory: hyper4 = {lr, lr_bias, momentum, ema_decay}; [0, n_param) parameters, [n_param, n_total)
 * buffers (EMA only; ema may be NULL); only hyper4[0..3] are read.  Bit-equal to mgdt_sgd_step followed by mgdt_ema_update: all three, like the
 * families below, are the one streaming kernel described there (SGD: 8 words per parameter; with `first` the old content of buf is not used).
 * Reference: yolo/engine/trainer.py:317-326 (warm-up values), :462-470, yolo/utils/torch_utils.py:342. */
int mgdt_sgd_ema_step_dev(float* p, const float* g, float* buf, const float* wd, long n_param, float* ema, long n_total, const float* hyper4,
                          int nesterov, int first, const float* clip2, mgdt_stream s);
/* Adam / AdamW / RMSProp on the same flat buffers (build_optimizer yolo/engine/trainer.py:651-654; `optimizer: auto` -> AdamW, :635-639), in
 * the operation order of torch's single-tensor path, one fp32 rounding per operation.  wd and clip2 as for mgdt_sgd_step (wd > 0 decayed group,
 * wd == 0 norm group, wd < 0 bias group stepping with lr_bias; either may be NULL).  Host scalars are doubles (Python floats); the entry points
 * derive 1 - beta, lr / bc1 and sqrt(bc2) in double, as torch does, and hand them to the kernel rounded to fp32 once.
 * adam: m = exp_avg, v = exp_avg_sq, step 1-based (bc1 = 1 - beta1^step, bc2 = 1 - beta2^step).  decoupled = 0 is torch.optim.Adam
 *   (g' = clip*g + wd*p), 1 is AdamW (p *= 1 - lr*wd, g' = clip*g); then m += (g' - m)*(1 - beta1); v = beta2*v + (1 - beta2)*g'*g';
 *   p -= (lr_group / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).  No amsgrad, no maximize.
 * rmsprop: torch.optim.RMSprop(centered=False): g' = clip*g + wd*p; sq = alpha*sq + (1 - alpha)*g'*g'; avg = sqrt(sq) + eps; with momentum > 0
 *   buf = momentum*buf + g'/avg, p -= lr_group*buf; else p -= lr_group*g'/avg (buf is then not touched and may be NULL).
 * *_ema_step_dev: the captured-step forms, bit-equal to the eager form followed by mgdt_ema_update: per-step scalars from device memory,
 *   [0, n_param) parameters (step, then EMA of the new value), [n_param, n_total) buffers (EMA only); ema may be NULL.  hyper8 (fp32[8], all eight
 *   readable; a family ignores what it has no use for):
 *     [0] lr  [1] lr_bias  [2] beta1 (Adam) / momentum (RMSProp)  [3] ema_decay  [4] lr / bc1  [5] lr_bias / bc1  [6] sqrt(bc2)  [7] 1 - beta1
 *   beta2 / alpha and eps are constants of a run and stay arguments.  Streaming kernels: 16-byte accesses when every array is 16-byte aligned
 *   (scalar otherwise), 10 words per parameter with all four state arrays.                                                                     */
#define MGDT_OPT_HYPER_LEN 8
int mgdt_adam_step(float* p, const float* g, float* m, float* v, const float* wd, long n, double lr, double lr_bias, double beta1,
                   double beta2, double eps, int step, int decoupled, const float* clip2, mgdt_stream s);
int mgdt_adam_ema_step_dev(float* p, const float* g, float* m, float* v, const float* wd, long n_param, float* ema, long n_total,
                           const float* hyper8, double beta2, double eps, int decoupled, const float* clip2, mgdt_stream s);
int mgdt_rmsprop_step(float* p, const float* g, float* sq, float* buf, const float* wd, long n, double lr, double lr_bias, double alpha,
                      double eps, double momentum, const float* clip2, mgdt_stream s);
int mgdt_rmsprop_ema_step_dev(float* p, const float* g, float* sq, float* buf, const float* wd, long n_param, float* ema, long n_total,
                              const float* hyper8, double alpha, double eps, int with_momentum, const float* clip2, mgdt_stream s);

/* ---- box helpers, validator reductions, predictor preprocess; fp32 boxes, rows of `row` >= 4 floats ------------
 * box_convert: mode 0 = xywh2xyxy (yolo/utils/ops.py:362-377), 1 = xyxy2xywh (:345-359); columns >= 4 are copied.
 * box_iou: pairwise IoU (n,4) x (m,4) -> (n,m), eps in the union (yolo/utils/metrics.py:52-72).
 * bbox_iou: row i of box1 (stride1 floats; 0 broadcasts one box) vs row i of box2; mode 0 IoU, 1 GIoU, 2 DIoU, 3 CIoU (metrics.py:75-128).
 * scale_boxes: in place (b - pad) / gain, then clip to [0, w0] x [0, h0] (ops.py:90-117 + clip_boxes :269-285).
 * letterbox: one uint8 HWC BGR image -> uint8 CHW RGB planes of the letter-boxed batch tensor (augment.py:538-593 geometry computed by the
 *   caller; resize = cv2 INTER_LINEAR 8-bit rule, border 114; predictor.py:123-125 BGR->RGB, HWC->CHW).
 * ap_per_class: the per-class part of metrics.py:410-497 (cumulative TP/FP, recall / precision, compute_ap's envelope + 101-point
 *   interpolation in numpy's own arithmetic order, the 1000-point P/R-vs-confidence curves); inputs grouped by class, descending confidence. */
int mgdt_box_convert(const float* in, float* out, long n, int row, int mode, mgdt_stream s);
int mgdt_box_iou(const float* b1, int n, const float* b2, int m, float eps, float* out, mgdt_stream s);
int mgdt_bbox_iou(const float* b1, int stride1, const float* b2, int stride2, long n, int xywh, int mode, float eps, float* out, mgdt_stream s);
int mgdt_scale_boxes(float* boxes, long n, int row, float gain, float padx, float pady, float h0, float w0, mgdt_stream s);
int mgdt_letterbox_fwd(const void* src_hwc_bgr, int sh, int sw, long src_pitch, void* dst_chw_rgb, int dh, int dw, int new_h, int new_w, int top,
                       int left, mgdt_stream s);
size_t mgdt_ap_workspace_bytes(int n_det, int n_cls);
int mgdt_ap_per_class(const void* tp, const float* conf, const int32_t* seg, const int32_t* nlab, int n_det, int n_cls, int T, const double* x101,
                      const double* px, double eps, void* ws, double* ap, double* pcur, double* rcur, mgdt_stream s);

/* ---- TOODHead training (reference nn/modules/head.py:466-572 under autograd; mmcv ModulatedDeformConv2d backward) -----------------------
 * GroupNorm(16)+act backward of Conv_GN / DyDCNv2.norm (head.py:67-81, block.py:401-432), composed with mgdt_nc_reduce:
 *   gn_affine:          sum_hw y, sum_hw y*y in double (the forward kernel's partial sums)  ->  mean / rstd per (image, group), A = gamma*rstd,
 *                       B = beta - mean*rstd*gamma  (u = y*A + B); y: 4-aligned NHWC view, c <= 4096; ws: mgdt_gn_affine_workspace_bytes, 8-byte aligned, whose
 *                       last n*groups*2 doubles (offset mgdt_gn_affine_workspace_bytes - n*groups*16) keep (mean, rstd) in double for gn_bwd_coef
 *   nc_affine_act_bwd:  gu = g * act'(y*A + B)        (A = B = NULL: u = y, i.e. with act = ReLU and y the layer output the ReLU mask)
 *   gn_act_grad:        GroupNorm's gu = g * act'((y - mean)*rstd*gamma + beta), u formed in double from stats_ng = gn_affine's double (mean, rstd) and
 *                       rounded once to fp32 (u = y*A + B with fp32 A, B is off by (|mean|/std) of 2^-24); matching 4-aligned NHWC views
 *   gn_bwd_coef:        S1 = sum_hw gu, S2 = sum_hw gu*y summed in double from the views, centred in double with stats_ng = gn_affine's double (mean, rstd)
 *                       ->  P, Q, R with dy = gu*P + y*Q + R, and dgamma / dbeta (written or accumulated: the head is shared by all levels);
 *                       ws: mgdt_gn_bwd_workspace_bytes, 8-byte aligned
 *   nc_axpby:           out = a*sa[n][c] (+ b*sb[n][c]) (+ shift[n][c])     (sa NULL: 1)
 * pixel_gate_bwd: adjoint of mgdt_pixel_gate_fwd (cls_feat * sigmoid(prob logit), head.py:530-537): gx = g*s, glogit = s(1-s) * sum_c g*x.
 * tood_layer_attn_bwd: adjoint of mgdt_tood_layer_attn_fwd (TaskDecomposition.forward head.py:107-116): dscale [n][c] -> dsums [n][c] (gradient
 *   w.r.t. sum_hw feat) and dW1 (hid*c), db1 (hid), dW2 (stacked*hid), db2 (stacked), written or accumulated.
 * dcn_im2col: col[n,y,x,c*9 + tap] = sigmoid(mask logit) * bilinear(x at p + offset) (mmcv modulated_deformable_im2col): the DCN output is the
 *   1x1 convolution of col with weight.view(cout, cin*9), so its weight / column gradients are mgdt_conv_wgrad / dgrad.
 * dcn_col2im_bwd: column gradient -> gx_f32 (dense fp32 NHWC, ZERO on entry; float atomics, the order-dependent scatter of mmcv's col2im) and
 *   gom (offset gradients 0..17, mask-LOGIT gradients 18..26, further channels zeroed) (mmcv modulated_deformable_col2im / col2im_coord). */
size_t mgdt_gn_affine_workspace_bytes(int n, int c, int groups);
int mgdt_gn_affine(const mgdt_view* y, const float* gamma, const float* beta, int groups, float eps, float* mean_ng, float* rstd_ng, float* A, float* B,
                   void* ws, int dtype, mgdt_stream s);
int mgdt_nc_affine_act_bwd(const mgdt_view* g, const mgdt_view* y, const float* A, const float* B, int act, const mgdt_view* gu, int dtype, mgdt_stream s);
int mgdt_gn_act_grad(const mgdt_view* g, const mgdt_view* y, const double* stats_ng, const float* gamma, const float* beta, int groups, int act,
                     const mgdt_view* gu, int dtype, mgdt_stream s);
size_t mgdt_gn_bwd_workspace_bytes(int n, int c);
int mgdt_gn_bwd_coef(const mgdt_view* gu, const mgdt_view* y, const double* stats_ng, const float* gamma, int groups, float* P, float* Q, float* R,
                     float* dgamma, float* dbeta, int accumulate, void* ws, int dtype, mgdt_stream s);
int mgdt_nc_axpby(const mgdt_view* a, const float* sa, const mgdt_view* b, const float* sb, const float* shift, const mgdt_view* out, int dtype,
                  mgdt_stream s);
int mgdt_pixel_gate_bwd(const mgdt_view* g, const mgdt_view* x, const mgdt_view* logit, const mgdt_view* gx, const mgdt_view* glogit, int dtype, mgdt_stream s);
size_t mgdt_tood_layer_attn_bwd_workspace_bytes(int n, int c, int hid, int stacked);
int mgdt_tood_layer_attn_bwd(const float* sums, const float* dscale, int n, int c, int hw, const float* w1, const float* b1, const float* w2,
                             const float* b2, int hid, int stacked, float* dsums, float* dw1, float* db1, float* dw2, float* db2, int accumulate,
                             void* ws, mgdt_stream s);
int mgdt_dcn_im2col(const mgdt_view* x, const mgdt_view* om, const mgdt_view* col, int dtype, mgdt_stream s);
int mgdt_dcn_col2im_bwd(const mgdt_view* gcol, const mgdt_view* x, const mgdt_view* om, float* gx_f32, const mgdt_view* gom, int dtype, mgdt_stream s);

/* ---- image classification (nn/modules/head.py:256-272 Classify, yolo/utils/loss.py:395-401, yolo/utils/metrics.py:197-207, :934-977) ----
 * mgdt_classify_pool_fwd: pooled[n][cout] (fp32) = mean over the pixels of SiLU(conv1x1(x, w) + bias): Classify.conv (BatchNorm folded by the caller
 *   into w [cout][c1] in `dtype`, row-major, and bias fp32[cout]) + AdaptiveAvgPool2d(1) in one launch on the matrix cores; the (n, cout, h, w) map is
 *   never stored.  Bit-reproducible (no floating-point atomics).  Refused before any launch: k != 1, groups != 1, act != MGDT_ACT_SILU (MGDT_BAD_ARG:
 *   those go through the unfused chain), x not NHWC, c1 % 8, cout % 16, pixel rows or w not 16-byte aligned, n > 65535.
 * mgdt_classify_linear_fwd: logits[n][nc] = pooled[n][k] @ w[nc][k]^T + bias (w in `dtype`, pooled / bias / logits fp32, fp32 accumulation; bias may
 *   be NULL); probs != NULL: the row softmax as well (a second launch).  k % 4 == 0, any nc >= 1.
 * mgdt_cls_softmax_fwd: probs = softmax(logits, dim 1), the row maximum subtracted; in place allowed.
 * mgdt_cls_loss_fwd: loss[0] = cross_entropy(logits, labels, reduction='sum') / 64 (the reference's constant, not the batch size); row_loss[n] is a
 *   caller-owned buffer that receives the per-row terms.  mgdt_cls_loss_bwd: dlogits = (softmax - onehot) / 64 * gscale.  labels: int64 on the
 *   device; a label outside [0, nc) gives a NaN loss and a zero gradient row, and nothing is read out of bounds.
 * mgdt_cls_topk_fwd: topk[n][min(nc, 5)] (int64) = indices of the largest values of each row of probs[n][nc], descending, equal values by lower
 *   index first.  matrix != NULL (int32 [nc][nc], accumulated: zero it first): matrix[topk[i][0]][targets[i]] += 1 (integer atomics). */
int mgdt_classify_pool_fwd(const mgdt_view* x, const void* w, const float* bias, int cout, int k, int groups, int act, float* pooled, int dtype,
                           mgdt_stream s);
int mgdt_classify_linear_fwd(const float* pooled, const void* w, const float* bias, int n, int k, int nc, float* logits, float* probs, int dtype,
                             mgdt_stream s);
int mgdt_cls_softmax_fwd(const float* logits, int n, int nc, float* probs, mgdt_stream s);
int mgdt_cls_loss_fwd(const float* logits, const int64_t* labels, int n, int nc, float* row_loss, float* loss, mgdt_stream s);
int mgdt_cls_loss_bwd(const float* logits, const int64_t* labels, int n, int nc, float gscale, float* dlogits, mgdt_stream s);
int mgdt_cls_topk_fwd(const float* probs, int n, int nc, int64_t* topk, const int64_t* targets, int32_t* matrix, mgdt_stream s);

/* ---- ByteTrack (reference tracker/trackers/byte_tracker.py:181-295, tracker/utils/kalman_filter.py KalmanFilterXYAH, tracker/utils/matching.py) ----
 * One frame of `streams` independent video streams in one launch, one workgroup per stream, no host read (capturable in a hipGraph).
 * rows [streams][max_det][6] fp32 (x1,y1,x2,y2,conf,cls) + counts[streams] as mgdt_nms_fwd writes them; active: NULL or uint8[streams], 0 = this
 * stream skips the frame (its state bytes, frame_id included, do not move; 0 rows).  state: mgdt_bytetrack_state_bytes(streams, cap) bytes, zeroed
 * by mgdt_bytetrack_reset (stream = -1: all).  cap <= 128 slots per stream for tracked + lost + unconfirmed tracks; at most 128 detections per
 * stream and frame above track_low_thresh.  track_buffer enters as max_time_lost = int(frame_rate / 30 * track_buffer).
 * tracks [streams][cap][8] fp32 (x1,y1,x2,y2,track_id,score,cls,idx), the activated Tracked tracks in ascending track_id, the box from the filter
 * mean after this frame's update, rows past ntracks[i] zero; flags[i] = 0, or 1 (too many detections) / 2 (no free slot for a new track): the
 * stream's state is then unchanged and ntracks[i] = 0.  Ids count from 1 per stream (the reference's counter is one class attribute shared by every
 * tracker of the process and reset by every constructor; per stream the ids equal those of a reference tracker run alone).
 * The filter state is fp64 in the decoupled form (four 2x2 blocks; every other covariance entry of the reference is exactly 0); costs are fp32 in
 * the reference's operation order; the three assignments of a frame are solved exactly (mgdt_track_assign's solver).
 * mgdt_track_assign: the solver alone. cost [batch][n_max][m_max] fp32, n[batch], m[batch] (n_max, m_max <= 128): the partial matching that
 *   minimises sum(c_ij - thresh) (lap.lapjv(cost, extend_cost=True, cost_limit=thresh)); pairs with c_ij >= thresh are never matched.
 *   x [batch][n_max] int32: the column of row i, -1 = unmatched (and for i >= n).
 * mgdt_bytetrack_export: the live tracks of one stream in ascending id: hdr[3] = {live tracks, frame_id, id counter}; ints [6][cap] = id, state
 *   (1 Tracked, 2 Lost, 3 Removed: see track.hip), is_activated, frame_id, start_frame, tracklet_len; score_cls [2][cap] fp32; mean [cap][8] fp64;
 *   cov [cap][8][8] fp64 (the blocks expanded, zeros elsewhere).  Only the first hdr[0] entries of each array are written. */
size_t mgdt_bytetrack_state_bytes(int streams, int cap);
int mgdt_bytetrack_reset(void* state, int streams, int cap, int stream, mgdt_stream s);
int mgdt_bytetrack_update(const float* rows, const int32_t* counts, const uint8_t* active, int streams, int max_det, void* state, int cap,
                          float track_high_thresh, float track_low_thresh, float new_track_thresh, float match_thresh, int max_time_lost,
                          float* tracks, int32_t* ntracks, int32_t* flags, mgdt_stream s);
int mgdt_track_assign(const float* cost, const int32_t* n, const int32_t* m, int batch, int n_max, int m_max, float thresh, int32_t* x,
                      mgdt_stream s);
int mgdt_bytetrack_export(const void* state, int streams, int cap, int stream, int32_t* hdr, int32_t* ints, float* score_cls, double* mean,
                          double* cov, mgdt_stream s);

/* ---- RT-DETR decoder head (reference nn/modules/head.py:275-464 RTDETRDecoder, nn/modules/transformer.py:187-378, vit/rtdetr/predict.py) ----
 * hd = 256 channels = 8 heads x 32, 4 sampling points, nl <= 4 levels; `shapes` = host int[2 * nl] (h, w) per level, tokens level after level,
 * row-major.  Every tensor is fp32 except the value tensor of mgdt_msdeform_attn_fwd and x of mgdt_add_layernorm_fwd (dtype: fp32 or bf16).  None of the calls reads back to the host.
 * mgdt_msdeform_attn_fwd: value[batch][L][ld_value >= 256] (image stride batch_stride_value elements), ref [batch][nq][4] (cx, cy, w, h in [0, 1]),
 *   offsets [batch][nq][ld_offsets >= 8*nl*4*2] and weights [batch][nq][ld_weights >= 8*nl*4] raw logits in the reference's (head, level, point[, xy])
 *   order.  loc = ref_xy + off / 4 * ref_wh * 0.5; bilinear at pixel loc * (W, H) - 0.5 with zero padding (grid_sample, align_corners=False);
 *   softmax over a head's nl*4 weights; out [batch][nq][256] fp32 = the weighted sum, accumulated in fp32.
 * mgdt_mha_fwd: softmax((q / sqrt(32)) k^T) v per head, no mask; q, k, v [batch][nq][ld >= 256], out [batch][nq][256]; any nq >= 1.
 * mgdt_add_layernorm_fwd: out[rows][256] = LayerNorm(x [+ res]) * gamma + beta; x in `dtype` (fp32 or bf16), everything else fp32.  fill != NULL (the masked form, rows = batch * L): rows whose
 *   anchor is invalid (head.py:382) read fill[256], rounded to `dtype`, in place of x.
 * mgdt_rtdetr_rowmax_fwd: out[rows] = max over x[rows][0..nc).
 * mgdt_rtdetr_topk_fwd: index[batch][k] int64 = the k best of scores[batch][L], descending, equal scores by ascending index (NaN = -inf); k <= L.
 * mgdt_rtdetr_gather_fwd: embed[b][q] = feat[b][index[b][q]] (256 channels), enc_scores[b][q] = scores[b][index[b][q]] (nc); an index outside
 *   [0, L) is clamped.
 * mgdt_rtdetr_ref_init_fwd: ref[b][q] = sigmoid(delta[b][q] + anchor(index[b][q])); an invalid anchor is +inf (ref = 1).
 * mgdt_rtdetr_refine_fwd: out = sigmoid(delta + inverse_sigmoid(ref)), eps 1e-5; out may be ref.
 * mgdt_rtdetr_sigmoid_fwd: out[rows][nc] dense = sigmoid(x[rows][ld]).
 * mgdt_rtdetr_post_fwd: boxes [batch][nq][4] xywh, scores [batch][nq][nc]; a query is kept when its best score > conf and (keep_class == NULL or
 *   keep_class[argmax]); rows [batch][nq][6] = (x1, y1, x2, y2) * (w, h, w, h) of wh[batch][2] (NULL: 1), conf, cls in query order, the rest zero;
 *   counts[batch] int32 - the layout mgdt_nms_fwd leaves. */
int mgdt_msdeform_attn_fwd(const void* value, long ld_value, long batch_stride_value, const int* shapes, int nl, int batch, int nq, const float* ref,
                           const float* offsets, long ld_offsets, const float* weights, long ld_weights, float* out, int dtype, mgdt_stream s);
int mgdt_mha_fwd(const float* q, long ld_q, const float* k, long ld_k, const float* v, long ld_v, int batch, int nq, float* out, mgdt_stream s);
int mgdt_add_layernorm_fwd(const void* x, int dtype, long ld_x, const float* res, long ld_res, const float* gamma, const float* beta, float eps, long rows,
                           const float* fill, const int* shapes, int nl, float* out, mgdt_stream s);
int mgdt_rtdetr_rowmax_fwd(const float* x, long rows, int nc, long ld, float* out, mgdt_stream s);
int mgdt_rtdetr_topk_fwd(const float* scores, int batch, int L, int k, int64_t* index, mgdt_stream s);
int mgdt_rtdetr_gather_fwd(const float* feat, const float* scores, long ld_scores, const int64_t* index, int batch, int L, int nq, int nc, float* embed,
                           float* enc_scores, mgdt_stream s);
int mgdt_rtdetr_ref_init_fwd(const float* delta, long ld_delta, const int64_t* index, int batch, int nq, const int* shapes, int nl, float* ref, mgdt_stream s);
int mgdt_rtdetr_refine_fwd(const float* delta, long ld_delta, const float* ref, long rows, float* out, mgdt_stream s);
int mgdt_rtdetr_sigmoid_fwd(const float* x, long rows, int nc, long ld, float* out, mgdt_stream s);
int mgdt_rtdetr_post_fwd(const float* boxes, const float* scores, int batch, int nq, int nc, float conf, const uint8_t* keep_class, const float* wh, float* rows,
                         int32_t* counts, mgdt_stream s);

/* ---- RT-DETR criterion and validator rows (reference vit/utils/ops.py:12-111 HungarianMatcher, vit/utils/loss.py DETRLoss / RTDETRDetectionLoss,
 * yolo/utils/loss.py:16-53, vit/rtdetr/val.py:90-106) ----
 * boxes [layers][batch][nq][4] xywh in [0, 1], logits [layers][batch][nq][ld_logits >= nc] raw, gt_boxes [G][4] xywh normalised, gt_cls [G] int32 (a
 * class outside [0, nc) is clamped), gt_off [batch + 1] int32 = the exclusive offsets of the images' ground truths, passed on the device (read by the
 * kernel) and on the host (checked; G = gt_off_host[batch]).  All fp32 unless said otherwise; no allocation, no host read, capturable.
 * mgdt_detr_match_fwd: one launch for every (layer, image).  C[q][g] = g_class * cost_class + g_bbox * L1 + g_giou * (1 - GIoU), cost_class the focal
 *   form of ops.py:86-88 on p = sigmoid(logit[q][gt_cls[g]]), GIoU = bbox_iou(xywh, eps 1e-7), in the reference's fp32 operation order; a cost that
 *   is not finite becomes 1e18.  Per (layer, image) the assignment that minimises the sum of C over the matchings that give every ground truth of
 *   the image a distinct query (scipy.optimize.linear_sum_assignment on the nq x ng block): shortest augmenting paths with fp64 potentials, exact for
 *   the fp32 costs up to fp64 rounding of path sums; with several optima the one found is unspecified.
 *   assign [layers][batch][nq] int32 = the global ground-truth index (into [G]) of the query, or -1.  cost: NULL or [layers][batch][nq][MGDT_DETR_GCAP],
 *   only the entries [q][0 .. ng) of an image are written.  layer_of_match = -1: every layer on its own costs; k >= 0: only layer k is solved and its
 *   assignment (and cost) is written for every layer (use_uni_match).  MGDT_BAD_SHAPE before any launch when an image has more than nq or more than
 *   MGDT_DETR_GCAP ground truths or nq > MGDT_DETR_MAX_NQ; any nq >= 1, nc >= 1; an image without ground truths gets -1 everywhere.
 *   workspace: mgdt_detr_match_workspace_bytes(layers, G, nq) bytes (the cost blocks, ground-truth major; contents undefined afterwards).
 * mgdt_detr_loss_fwd: one launch for every layer.  assign as above (any value outside [0, G) = unmatched; several queries may share a ground truth:
 *   a denoising pass); num_pairs = matched pairs per layer, known to the host.  gt_score [layers][batch][nq] = IoU (bbox_iou xywh, eps 1e-7) of a
 *   matched query with its ground truth, 0 otherwise.  out [layers + 1][3] = (class, bbox, giou) per layer, then in row `layers` the sum of the rows 0 .. layers - 2 (the `_aux` entries): class = g_class * sum over (b, q, c) / max(num_pairs, 1)
 *   of VarifocalLoss (use_vfl and num_pairs > 0: weight 0.75 sigmoid(x)^2 (1 - label) + gt_score label, target gt_score * onehot) or FocalLoss
 *   (gamma 1.5, alpha 0.25); bbox = g_bbox * sum L1 / num_pairs; giou = g_giou * sum (1 - GIoU) / num_pairs; both 0 when num_pairs == 0.
 *   d_boxes [layers][batch][nq][4] and d_logits [layers][batch][nq][nc] (dense), both or neither NULL: the gradients of gscale * sum over layers of
 *   (class + bbox + giou), gt_score held constant, the varifocal weight differentiated; every element is written (0 for an unmatched query's box).
 *   Box terms in fp64, class terms in fp32, sums in fp64: per-workgroup partials, then one fixed-order reduction by the workgroup that arrives last -
 *   no floating-point atomics, bit-equal from run to run.  workspace: mgdt_detr_loss_workspace_bytes(layers, batch, nq) bytes, 16-byte aligned; its
 *   first 16 bytes are zero before the first call and the kernel leaves them zero.
 * mgdt_rtdetr_val_post_fwd: boxes [batch][nq][4] xywh, scores [batch][nq][nc] -> rows [batch][nq][6] = (x1, y1, x2, y2) * (w, h, w, h) of
 *   wh[batch][2] (NULL: 1), conf = class maximum, cls (lowest index on ties); ALL nq rows, no threshold, in descending confidence, equal confidences
 *   by ascending query index, NaN last (the reference's argsort(descending=True) leaves ties unspecified); counts[batch] int32 = nq.
 *   1 <= nq <= MGDT_RTDETR_VAL_MAX_NQ, one workgroup per image. */
#define MGDT_DETR_GCAP 256
#define MGDT_DETR_MAX_NQ 2048
#define MGDT_RTDETR_VAL_MAX_NQ 4096
size_t mgdt_detr_match_workspace_bytes(int layers, int G, int nq);
int mgdt_detr_match_fwd(const float* boxes, const float* logits, long ld_logits, int layers, int batch, int nq, int nc, const float* gt_boxes,
                        const int32_t* gt_cls, const int32_t* gt_off_dev, const int32_t* gt_off_host, float g_class, float g_bbox, float g_giou,
                        float alpha, float gamma, int layer_of_match, void* workspace, size_t workspace_bytes, int32_t* assign, float* cost,
                        mgdt_stream s);
size_t mgdt_detr_loss_workspace_bytes(int layers, int batch, int nq);
int mgdt_detr_loss_fwd(const float* boxes, const float* logits, long ld_logits, int layers, int batch, int nq, int nc, const float* gt_boxes,
                       const int32_t* gt_cls, int G, const int32_t* assign, long num_pairs, float g_class, float g_bbox, float g_giou, int use_vfl,
                       float gscale, void* workspace, size_t workspace_bytes, float* out, float* gt_score, float* d_boxes, float* d_logits,
                       mgdt_stream s);
int mgdt_rtdetr_val_post_fwd(const float* boxes, const float* scores, int batch, int nq, int nc, const float* wh, float* rows, int32_t* counts,
                             mgdt_stream s);

/* ---- training augmentation (reference yolo/data/augment.py:762-790 v8_transforms, detection, stretch=False: Mosaic :117-188 or LetterBox
 * :538-601, RandomPerspective :289-476 with perspective = 0, RandomHSV :479-501, RandomFlip :504-535, Format :692-746) -----------------------
 * A batch of B output images in two launches; every random draw is made by the caller.  Nothing reads back to the host.
 * pool: flat uint8, the images one after another, each h x w x 3 BGR (HWC, packed rows); the image table says where: one mgdt_aug_image per pool
 *   image = byte offset, h, w (each <= imgsz) and the image's rows label_start .. +label_count of pool_labels [n_labels][5] fp32
 *   (cls, x, y, w, h normalised to the image).  The table is passed twice: on the device for the kernels, on the host for the checks.
 * records: one mgdt_aug_record per output image, 56 32-bit words, also passed on the device (read by the kernels) and on the host (checked):
 *   word 0       nrect   rectangles placed on the canvas, 0..4 (4: a mosaic, 1: a letter-boxed image)
 *   word 1       canvas  side of the square canvas in pixels (2 * imgsz for a mosaic, imgsz otherwise); it is never stored: 114 wherever no rectangle lies
 *   word 2       flags   bit 0 flip up-down, bit 1 flip left-right, bit 2 the labels are clipped to the canvas and zero-area boxes dropped (Mosaic._cat_labels)
 *   word 3       lut     byte offset into `luts` of this image's three 256-entry tables (hue, saturation, value: 768 bytes), a multiple of 4; -1: no HSV step
 *   words 4..31  rect    [4][7] int32: source id, destination x1 y1 x2 y2 on the canvas (exclusive ends), source x1 y1: canvas[y1:y2, x1:x2] =
 *                        image[sy1:.., sx1:..]; a later rectangle lies over an earlier one
 *   words 32..37 inv     fp32: output pixel (x, y) of the unflipped imgsz x imgsz image reads the canvas at (inv0 x + inv1 y + inv2, inv3 x + inv4 y + inv5),
 *                        pixel centres at integers, bilinear over the four neighbours, each 114 outside the canvas or outside every rectangle;
 *                        evaluated in fp64 and rounded to the nearest integer
 *   words 38..43 m       fp32: the first two rows of the forward matrix M (canvas -> output), for the boxes
 *   word 44      scale   fp32: s of box_candidates (the source box is scaled by it; wh_thr 2, ar_thr 100, area_thr 0.1, eps 1e-16)
 *   words 45..52 pad     [4][2] fp32: what is added to the de-normalised boxes of rectangle k's source (x, y)
 *   words 53..55 reserved, 0
 * mgdt_aug_check: the host-side test both launches run first (callable alone, no GPU): MGDT_BAD_ARG for a null table, a source id outside the pool, a
 *   LUT offset outside `luts` or a non-finite coefficient; MGDT_BAD_SHAPE for a count, size, image or rectangle out of range.  imgsz % 4 == 0.
 *   The kernels cut every rectangle to its source image again, so device records that differ from the checked ones read 114, never out of bounds.
 * mgdt_aug_warp_fwd: out [batch][3][imgsz][imgsz] uint8, planes R, G, B, dense.  8-bit BGR <-> HSV by OpenCV's documented formulas (V = max,
 *   S = 255 (V - min) / V, H / 2 in 0..179) in exact integer arithmetic, rounded half to even, H rounded before the wrap by 180.
 * mgdt_aug_labels_fwd: cap = label rows per image, a multiple of 16.  labels [batch][cap][5] = (cls, x, y, w, h) normalised (Format's output), gt
 *   [batch][cap][5] = (cls, x1, y1, x2, y2) in pixels (what v8DetectionLoss.preprocess makes of them), both in the order source by source, then the source's own;
 *   rows past nlabels[b] zero.  flags[b] = 1 when more than cap boxes survive: the rows are then the first cap, nlabels[b] = cap. */
typedef struct { int64_t offset; int32_t h, w, label_start, label_count; } mgdt_aug_image;
typedef struct {
  int32_t nrect, canvas, flags, lut;
  int32_t rect[4][7];
  float inv[6], m[6], scale, pad[4][2];
  int32_t reserved[3];
} mgdt_aug_record;
int mgdt_aug_check(const mgdt_aug_record* records_host, int batch, const mgdt_aug_image* images_host, int n_pool, size_t pool_bytes, long n_labels,
                   size_t lut_bytes, int imgsz);
int mgdt_aug_warp_fwd(const void* pool, size_t pool_bytes, const mgdt_aug_image* images_dev, const mgdt_aug_image* images_host, int n_pool,
                      const mgdt_aug_record* records_dev, const mgdt_aug_record* records_host, const void* luts, size_t lut_bytes, int batch, int imgsz,
                      void* out, mgdt_stream s);
int mgdt_aug_labels_fwd(const float* pool_labels, long n_labels, const mgdt_aug_image* images_dev, const mgdt_aug_image* images_host, int n_pool,
                        const mgdt_aug_record* records_dev, const mgdt_aug_record* records_host, int batch, int imgsz, int cap, float* gt, float* labels,
                        int32_t* nlabels, int32_t* flags, mgdt_stream s);

#ifdef __cplusplus
}
#endif
#endif /* MGDT_H */
