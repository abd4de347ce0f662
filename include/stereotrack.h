/*
 * stereotrack.h — C ABI of libstereotrack_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-frame dense compute path of
 * Superjie13/StereoTracking.  The reference has NO FFI of its own (pure Python
 * on third-party wheels, reference setup.py:223 `ext_modules=[]`), so every
 * entry point below cites the reference *Python* interface it replaces; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ST_ERR_* otherwise;
 *     st_last_error() returns a thread-local message.  No exceptions cross
 *     the ABI.
 *   - all pointers named *_dev are device pointers owned by the CALLER
 *     (PyTorch); the library owns only packed weights (freed by *_destroy).
 *   - all work is enqueued on the caller's stream (a hipStream_t passed as
 *     void*); no call synchronises the device or allocates on the hot path.
 *   - pointer contract (DESIGN.md "Pointer contract"): a device pointer is aligned to its element at least.  Where a
 *     kernel moves 16 bytes at a time the entry either takes a scalar kernel for a pointer (stride, offset) that is
 *     not 16-byte aligned - same results, bit for bit - or refuses it with ST_ERR_INVALID before anything is
 *     launched; which of the two is said at the entry.  Packed weights, biases and workspaces are always 16-byte
 *     aligned (8 bytes where a workspace holds 64-bit fields only).
 *   - activations are fp32.  Internal activation layout is NHWC
 *     (pixel-major, channel-contiguous); the boundary tensors keep the
 *     reference's NCHW layout.
 */
#ifndef STEREOTRACK_H_
#define STEREOTRACK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_VERSION 430

enum {
  ST_OK = 0,
  ST_ERR_INVALID = -1,   /* bad argument / shape mismatch            */
  ST_ERR_HIP = -2,       /* a HIP runtime call failed                */
  ST_ERR_STATE = -3,     /* call order violated (e.g. not finalized) */
  ST_ERR_WORKSPACE = -4, /* caller workspace too small               */
  ST_ERR_NOTFOUND = -5   /* unknown parameter name                   */
};

typedef void* st_stream_t; /* hipStream_t */

int st_version(void);
const char* st_last_error(void);

/* ------------------------------------------------------------------------
 * 1. Convolution primitive (exact-fp32 MFMA implicit GEMM, NHWC).
 *    Replaces one mmcv ConvModule = Conv2d(bias=False) + BatchNorm2d(eps) +
 *    SiLU as built in reference
 *    mmtrack/models/backbones/csp_darknet_disparity_v1.py:104-153
 *    (BN already folded into wgt/bias by the caller or by st_detector_*).
 * ---------------------------------------------------------------------- */
typedef struct StConvDesc {
  /* input: NHWC view, pixel (n,y,x) at in_dev[((n*Hi+y)*Wi+x)*in_ld + in_off + c] */
  const float* in_dev;
  int N, Hi, Wi, Cin, in_ld, in_off;
  /* weights [CoutPad][Kpad] row-major, K index = (kh*KW+kw)*Cin + ci,
   * Kpad = roundup(KH*KW*Cin, 32), CoutPad = roundup(Cout, 32), zero padded;
   * bias [CoutPad] */
  const float* wgt_dev;
  const float* bias_dev;
  int Cout, KH, KW, stride, pad;
  /* outputs: channels [0,split) -> out1, [split,Cout) -> out2 (NULL if unused) */
  float* out1_dev;
  int out1_ld, out1_off, split;
  float* out2_dev;
  int out2_ld, out2_off;
  /* optional: every channel is ALSO stored nearest-x2 upsampled (2Ho x 2Wo) */
  float* up_dev;
  int up_ld, up_off;
  /* optional residual: out = (act(conv+bias) + res) * post_scale */
  const float* res_dev;
  int res_ld, res_off;
  float post_scale;
  int act; /* 0 = identity, 1 = SiLU */
  /* optional: the same weights in Winograd F(2x2,3x3) form (st_wino_pack_weights of wgt, fragment order); enables
   * kernel instances 43 / 44 for 3x3 / stride-1 / pad-1 layers with Cin % 4 == 0 (>= 16; a Cin that is not a multiple
   * of 32 runs a short last K-chunk) and Cout a multiple of 32 or 33..64 (one zero-padded block of 64).  NULL = not
   * available. */
  const float* wgt_wino_dev;
} StConvDesc;

/* in_dev and wgt_dev must be 16-byte aligned, Cin / in_ld / in_off multiples of 4 (ST_ERR_INVALID otherwise); the
 * output, upsample and residual tensors of the tile instances take any float alignment, stride and offset. */
int st_conv2d_nhwc(const StConvDesc* d, st_stream_t stream);
/* The same convolution with the kernel instance chosen by the caller instead of the library's heuristic:
 * variant 0..21 = tile instances of the implicit-GEMM kernel (st_conv_variant_name), 41 = streaming 1x1 kernel,
 * 42 = direct 3x3 kernel, 43 / 44 = Winograd F(2x2,3x3) kernel with 64- / 32-cout workgroups (need wgt_wino_dev),
 * 46 = 1x1 kernel with the weight matrix resident in LDS and register-fed pixels (Cin -> Cout one of 64->64, 128->64,
 * 128->128, 256->128), -1 = heuristic.  Returns ST_ERR_INVALID when the instance cannot run this layer (tile
 * does not divide the padded Cout, ...), so callers can autotune per layer by timing the valid ones — which is
 * what st_detector_autotune does internally and StereoCostVolume.autotune does for the aggregation convs.
 * Results are the same convolution for every valid variant (fp32 rounding differs with the summation order).
 * Instances 41 .. 46 also return ST_ERR_INVALID for a tensor, weight or bias pointer that is not 16-byte aligned (41:
 * in_dev and wgt_dev; its outputs and residual take a scalar epilogue) and for strides / offsets that are not
 * multiples of 4. */
int st_conv2d_nhwc_variant(const StConvDesc* d, st_stream_t stream, int variant);
/* Winograd form of a 3x3 weight tensor.  packed_wgt_host: the [CoutPad][Kpad] matrix st_conv_pack_weights produced
 * (host memory); out_host: st_wino_packed_floats(Cout, Cin) floats, to be uploaded and passed as wgt_wino_dev.
 * U = G g G^T is evaluated in fp64 on the folded fp32 weights and rounded once. */
size_t st_wino_packed_floats(int Cout, int Cin);
int st_wino_pack_weights(const float* packed_wgt_host, int Cout, int Cin, float* out_host);
/* GROUPED Winograd launch: n = 2..6 INDEPENDENT layers (their own shapes, tensors and weights) as ONE grid - what the
 * detector plan does with one tower depth of the head over the three levels (instances 48 / 49).  Every layer must be
 * a wide Winograd layer without a K tail: 3x3 / stride 1 / pad 1, wgt_wino_dev set, Cout % 64 == 0, Cin % 32 == 0, no
 * residual / split / upsample store.  Each output is bit-identical to st_conv2d_nhwc_variant(&descs[k], stream, 43).
 * ST_ERR_INVALID (nothing launched) when a layer or n does not qualify. */
int st_conv3x3_wino_group(const StConvDesc* descs, int n, st_stream_t stream);

/* Fused pair of 1x1 convolutions for the narrow high-resolution CSP layers: `b` (Cin = 32, Cout <= 32) consumes
 * output channels [0, 32) of `a` (Cin 32 or 64, 32 < Cout <= 64, no residual) - the CSPLayer main_conv ->
 * DarknetBottleneck conv1 pair (mmdet CSPLayer, built at csp_darknet_disparity_v1.py:113-153).  a's outputs are
 * written as usual; b's in_dev / in_ld / in_off are ignored (its input never leaves the registers).  The same pair
 * one stage deeper (a: 128 or 256 -> 64 | 64 split store, b: 64 -> 64) runs on the LDS-resident kernel (variant 46). */
int st_conv1x1_chain(const StConvDesc* a, const StConvDesc* b, st_stream_t stream);
/* Fused head of a stage-1 CSP branch: `a` = 3x3 / stride-2 / pad-1 ConvModule 32 -> 64 (its own output tensor is never
 * written: a->out1_dev is ignored), `ms` = CSPLayer main_conv | short_conv on a's output (1x1, 64 -> 32 | 32, split
 * store to ms->out1 / ms->out2), `c1` = DarknetBottleneck conv1 on the main half (1x1, 32 -> 32, to c1->out1).  One
 * launch instead of three; the 64-channel stride-2 tensor stays in MFMA accumulators.  Replaces the module sequence
 * csp_darknet_disparity_v1.py:113-153 builds for `stage1` / `disp_stage1` (ConvModule(c, 2c, 3, stride=2) followed by
 * mmdet CSPLayer) as run at :176-183.  All three: SiLU, no residual / upsample store / post_scale.  frag_*_dev =
 * st_front_pack_frags of the ms / c1 packed weight matrices (device copies).  ST_ERR_INVALID when the shapes differ. */
size_t st_front_frag_floats(int Cout, int Cin);
int st_front_pack_frags(const float* packed_wgt_host, int Cout, int Cin, float* out_host);
int st_conv3x3s2_csp_front(const StConvDesc* a, const StConvDesc* ms, const StConvDesc* c1, const float* frag_ms_dev,
                           const float* frag_c1_dev, st_stream_t stream);
/* Fused TAIL of a stage-1 CSP branch (round 6, tile variant 56): `conv2` = DarknetBottleneck conv2 (3x3 / stride 1 /
 * pad 1, 32 -> 32, SiLU, with the identity in conv2->res) whose output tensor conv2->out1 (the first 32 channels of the
 * CSP concat) is NEVER written, `fin` = CSPLayer final_conv (1x1, 64 -> 64, SiLU) reading that concat (fin->in_dev ==
 * conv2->out1_dev, same ld / offset; its channels [32, 64) = the `short` half must already be in memory), with an
 * optional residual on `fin` = the two-branch average (v + other) * post_scale of
 * csp_darknet_disparity_v1.py:155-184.  One PERSISTENT launch instead of two: Winograd F(2x2,3x3) with the transformed
 * 32 x 32 weights resident in registers, conv2's output handed to the 1x1 GEMM through LDS.  Replaces the module
 * sequence mmdet CSPLayer builds behind its first bottleneck (reference csp_darknet_disparity_v1.py:145-153, run at
 * :176-184).  conv2 needs wgt_wino_dev; frag_fin_dev = st_csp_tail_pack_frags of fin's packed weight matrix (device
 * copy, st_csp_tail_frag_floats() floats).  ST_ERR_INVALID when the shapes differ. */
size_t st_csp_tail_frag_floats(void);
int st_csp_tail_pack_frags(const float* packed_wgt_host, float* out_host);
int st_conv3x3_csp_tail(const StConvDesc* conv2, const StConvDesc* fin, const float* frag_fin_dev, st_stream_t stream);
/* Pack one Conv2d weight [Cout][Cin][KH][KW] (+ optional BN, folded in fp64)
 * into the kernel layout above.  Host function; out buffers are host memory
 * of st_conv_packed_floats(...) / roundup(Cout,32) floats. */
size_t st_conv_packed_floats(int Cout, int Cin, int KH, int KW);
int st_conv_pack_weights(const float* w, const float* conv_bias, /* may be NULL */
                         const float* bn_gamma, const float* bn_beta,
                         const float* bn_mean, const float* bn_var, /* NULL = no BN */
                         double bn_eps, int Cout, int Cin, int KH, int KW,
                         float* wgt_out, float* bias_out);

/* ------------------------------------------------------------------------
 * 2. Input packing: NCHW fp32 image -> Focus (space-to-depth) NHWC 12-ch.
 *    Replaces mmdet Focus slicing, reference
 *    csp_darknet_disparity_v1.py:104-111 (order TL,BL,TR,BR).
 *    H, W even; the image 8-byte and the output 16-byte aligned (ST_ERR_INVALID otherwise).
 * ---------------------------------------------------------------------- */
int st_focus_pack(const float* img_nchw_dev, int N, int C, int H, int W,
                  float* out_nhwc_dev, st_stream_t stream);

/* Fused Focus + stem ConvModule: Focus(x) followed by the 3x3/s1/p1 ConvModule over its 12 channels is a
 * 6x6/s2/p2 convolution of the planar 3-channel image, computed here in one kernel (no NHWC 12-channel
 * intermediate).  Replaces csp_darknet_disparity_v1.py:104-111 (`Focus(3, c, kernel_size=3)`, both the RGB
 * `stem` and the `disp_stem`) as run at :176-179.  Cout <= 64; H even, W a multiple of 4, image and bias 16-byte aligned
 * (ST_ERR_INVALID otherwise); an output that is not 16-byte aligned, or whose out_ld / out_off / Cout is not a multiple
 * of 4, is written by scalar stores - same values.
 *   w            stem conv weight [Cout][12][3][3], channels in Focus order (TL,BL,TR,BR groups of 3)
 *   wgt_out      st_stem_packed_floats(Cout) floats, bias_out round_up(Cout,32) floats (host buffers)
 *   out_nhwc_dev [N][H/2][W/2][out_ld], channels written at [out_off, out_off + Cout)          */
size_t st_stem_packed_floats(int Cout);
/* used_planes: 3 = generic image; 1 = the caller guarantees that the three planes are identical (disp_postp is
 * a 3-channel repeat of one map, loading_disparity.py:85-86): the per-tap weights of the three planes are summed
 * (fp64, rounded once) and only plane 0 is read: K = 36 instead of 108. */
int st_stem_pack_weights(const float* w, const float* conv_bias, /* may be NULL */
                         const float* bn_gamma, const float* bn_beta,
                         const float* bn_mean, const float* bn_var, /* NULL = no BN */
                         double bn_eps, int Cout, int used_planes, float* wgt_out, float* bias_out);
int st_stem_focus_conv(const float* img_nchw_dev, int N, int H, int W, int used_planes, const float* wgt_dev,
                       const float* bias_dev, int Cout, float* out_nhwc_dev, int out_ld, int out_off,
                       int act /* 1 = SiLU */, st_stream_t stream);
/* The same stem reading RAW frames: N separate uint8 [3][h][w] device frames (HOST array of N <= 32 device pointers,
 * 4-byte aligned, w % 4 == 0), converted to fp32 and padded to H x W with pad_value (integral, 0..255) while the input
 * windows are staged - TrackDataPreprocessor_Disparity_V1's cast + stack_batch pad (reference
 * data_preprocessor_disparity_v1.py:38-51, utils/misc.py:13-64) fused into the stem; same values as st_pack_raw_frames
 * followed by st_stem_focus_conv. */
int st_stem_focus_conv_u8(const unsigned char* const* frames_u8_dev_ptrs_host, int N, int h, int w, int H, int W,
                          float pad_value, const float* wgt_dev, const float* bias_dev, int Cout, float* out_dev,
                          int out_ld, int out_off, int act, st_stream_t stream);

/* Raw input packing: uint8 image (N,3,h,w) -> fp32 (N,3,H,W) padded with img_pad;
 * uint16 disparity PNG codes (N,h,w) -> disp_postp fp32 px = code/16 (65535 -> 0) x3 channels padded with
 * 0, and disp_mask (N,1,H,W) = code < 65535.  Replaces LoadDisparityFromFile._post_processing_v2
 * (reference datasets/transforms/loading_disparity.py:82-86,129-134), Pad_Disparity
 * (transforms_disparity.py:234-249) and the preprocessor's cast + pad
 * (data_preprocessor_disparity_v1.py:38-51) for frames uploaded raw.  Any of the two halves may be NULL. */
int st_pack_raw_inputs(const unsigned char* img_u8_dev, const unsigned short* disp_u16_dev, int N, int h, int w,
                       int H, int W, float img_pad, float* img_out_dev, float* disp_postp_out_dev,
                       float* disp_mask_out_dev, st_stream_t stream);
/* The image half of st_pack_raw_inputs for frames in SEPARATE allocations (one contiguous (3, h, w) uint8 tensor per
 * frame, as a dataloader hands them over - reference formatting_disparity.py:139-338 packs one frame per sample):
 * frames_u8_dev_ptrs_host = HOST array of N device pointers (N <= 32; they travel in the kernel arguments), w and W
 * multiples of 4.  No concatenated staging copy. */
int st_pack_raw_frames(const unsigned char* const* frames_u8_dev_ptrs_host, int N, int h, int w, int H, int W,
                       float img_pad, float* img_out_dev, st_stream_t stream);
/* Resize_Disparity with a non-identity scale (reference datasets/transforms/transforms_disparity.py:23-137: the image
 * through mmcv.imrescale / imresize = cv2.resize INTER_LINEAR, disp_postp / disp_mask / depth_postp through
 * INTER_NEAREST, :52-112).  P planes of h x w elements -> h2 x w2; interleaved = 0: planar [P][h][w], 1: [h][w][P].
 * bilinear = 1 (elem_bytes 1 only): OpenCV's 8-bit INTER_LINEAR restated (11-bit fixed-point taps, the exact 2 x 2
 * decimation as a box mean; cv2 is un-vendored: published algorithm, parity unpinned); bilinear = 0: INTER_NEAREST for
 * 1- / 2- / 4-byte elements (uint8 masks, uint16 PNG codes, fp32 maps: the sampling commutes with code / 16). */
int st_resize_planes(const void* in_dev, int P, int h, int w, int interleaved, void* out_dev, int h2, int w2,
                     int elem_bytes, int bilinear, st_stream_t stream);
/* StereoRectify (new; the reference's AirSim pairs arrive rectified): undistort + rectify F <= 32 raw frames through
 * fixed-point maps in ONE launch (csrc/rectify.hip).  src_dev_ptrs_host = HOST array of F device pointers (they travel
 * in the kernel arguments), each a contiguous planar (P, h, w) frame, P in {1, 3}; maps_dev = M maps [M][h2][w2][2]
 * int32 (qx, qy) in 1/32 px (stereotracking_amd/rectify.py builds them: initUndistortRectifyMap restated, 8-byte
 * aligned); map_index_host[f] in [0, M) selects frame f's map (left / right of a pair in one launch).  The results go
 * to dst_dev_ptrs_host (HOST array of F device pointers) or to dst_block_dev (one contiguous (F, P, h2, w2) block);
 * exactly one of the two is non-NULL.  Rule (exact integers, identical on host and device): x0 = qx >> 5, a = qx & 31,
 * y0 = qy >> 5, b = qy & 31;  bilinear = 1 (elem_bytes 1 only):
 *   out = ((32-a)(32-b) p00 + a(32-b) p01 + (32-a)b p10 + ab p11 + 512) >> 10
 * with a tap outside the raw image = border and a tap of weight 0 NEVER READ - cv2.remap's 8-bit INTER_LINEAR on
 * CV_16SC2 maps (cv2 un-vendored: published algorithm, parity unpinned);  bilinear = 0 (elem_bytes 1, 2 or 4): the
 * element at ((qx + 16) >> 5, (qy + 16) >> 5), outside the image `border` (1-byte elements) or 0.  Any h, w, h2, w2;
 * no workspace; nothing outside the outputs is written, nothing outside the frames and maps is read. */
int st_rectify_remap(const void* const* src_dev_ptrs_host, int F, int P, int h, int w, const int* maps_dev, int M,
                     const int* map_index_host, void* const* dst_dev_ptrs_host, void* dst_block_dev, int h2, int w2,
                     int elem_bytes, int bilinear, int border, st_stream_t stream);

/* SPP: out[..., 0:C]=x, [C:2C]=maxpool5, [2C:3C]=maxpool9, [3C:4C]=maxpool13
 * (stride 1, same pad, -inf padding).  x may alias out channels [0,C).
 * Replaces mmyolo SPPFBottleneck pooling, csp_darknet_disparity_v1.py:137-144.  C, strides and offsets multiples
 * of 4, x_dev and out_dev 16-byte aligned (ST_ERR_INVALID otherwise). */
int st_spp_pool(const float* x_dev, int x_ld, int x_off, int N, int H, int W, int C,
                float* out_dev, int out_ld, int out_off, st_stream_t stream);

/* ------------------------------------------------------------------------
 * 3. Two-branch YOLOX detector (backbone + PAFPN + decoupled head).
 *    Replaces YOLODetector_Disparity_V1._forward, reference
 *    mmtrack/models/detectors/yolo_detector_disparity_v1.py:127-142
 *    (extract_feat :77-90 -> backbone forward
 *    csp_darknet_disparity_v1.py:155-206 -> mmyolo YOLOXPAFPN ->
 *    YOLOXHeadModule.forward).
 * ---------------------------------------------------------------------- */
typedef struct StDetector StDetector;

typedef struct StDetectorConfig {
  int struct_size;      /* = sizeof(StDetectorConfig) */
  float widen_factor;   /* 0.5 for YOLOX-s */
  float deepen_factor;  /* 0.33 */
  int num_classes;      /* 1 */
  int batch;            /* N frames per forward */
  int height, width;    /* padded input size, multiples of 32 */
  double bn_eps;        /* 1e-3 */
  int with_right_branch; /* also build stem+stage1 features for the right image (stereo module) */
  int disp_planes_identical; /* 1 = the caller guarantees disp_postp is a 3-channel repeat of ONE map (what the
                              * reference loader yields, loading_disparity.py:85-86, and what
                              * st_disp_upsample_pack writes): the disparity stem then reads plane 0 only with
                              * plane-summed weights (K = 36 instead of 108).  0 = generic 3-plane input. */
  int rgb_only;         /* 1 = the single-branch detector of the reference's second stereo config
                         * (configs/stereo_tracking/ocsort/yolox_s_mmyolo_mot_airdrone.py:40-42: backbone
                         * `mmtrack.CSPDarknet`, mmtrack/models/backbones/csp_darknet.py:8-13 - forward reads x['img']
                         * only): no disp_stem / disp_stage1 parameters or launches, no branch average; stage2 consumes
                         * the RGB stage-1 features.  The disparity input of the forward calls may then be NULL (the
                         * MOT shell still consumes the disparity for the per-box depth, ocsort_disparity.py:82-83). */
  int out_fd;           /* 1 = the backbone's `out_fd=True` (csp_darknet_disparity_v1.py:72,203-204): the disparity
                         * branch's stage-1 features BEFORE the average are an output too (tap "stage1_disp", the `df`
                         * input of the disparity-completion head, section 23).  disp_stage1 then stores its own tensor
                         * and the average (o_disp + o_rgb) * 0.5 is one more op of the plan; "stage1_fused" and the
                         * head output are bit-identical to the out_fd = 0 plan.  0 = the plan as before, launch for
                         * launch.  Not with rgb_only (ST_ERR_INVALID).  The field sits in what used to be the struct's
                         * tail padding, so sizeof(StDetectorConfig) did not change: a caller that zero-initialises
                         * the struct (or passes struct_size = offsetof(StDetectorConfig, out_fd)) gets the old plan;
                         * other values than 0 / 1 are refused. */
} StDetectorConfig;

int st_detector_create(const StDetectorConfig* cfg, StDetector** out);
int st_detector_destroy(StDetector* det);

/* Parameter table, named exactly like the reference state_dict
 * ("backbone.stem.conv.conv.weight", "backbone.disp_stage1.0.bn.running_var",
 *  "neck.reduce_layers.2.conv.weight", "bbox_head.head_module.multi_level_conv_cls.0.bias" ...;
 *  SURVEY.md §5 checkpoint row). */
int st_detector_num_params(const StDetector* det);
int st_detector_param_info(const StDetector* det, int idx, char* name, int name_cap,
                           int64_t shape[4], int* ndim);
int st_detector_set_param(StDetector* det, const char* name, const float* host, int64_t numel);
/* fold BN (fp64), repack, upload.  Needs a current HIP device. */
int st_detector_finalize(StDetector* det);

size_t st_detector_workspace_bytes(const StDetector* det);
/* head output layout: for level l (stride 8,16,32): float[N][H_l*W_l][row] rows of
 * [cls logits (num_classes) | reg x,y,w,h | obj logit | unused up to st_head_row_floats(num_classes): 8 for 1..3 classes];
 * levels concatenated.  st_detector_head_floats = total float count. */
size_t st_detector_head_floats(const StDetector* det);
int st_detector_num_levels(const StDetector* det);
int st_detector_level_info(const StDetector* det, int level, int* h, int* w, int* stride,
                           size_t* float_offset);
/* img/disp: NCHW fp32 [N][3][H][W] device pointers (the tensors
 * TrackDataPreprocessor_Disparity_V1 produces, reference
 * data_preprocessor_disparity_v1.py:21-84).  Every device pointer of the forward entries (images, workspace, head
 * output) must be 16-byte aligned: ST_ERR_INVALID before the first launch otherwise. */
int st_detector_forward(StDetector* det, const float* img_dev, const float* disp_dev,
                        void* workspace_dev, size_t workspace_bytes, st_stream_t stream,
                        float* head_out_dev);
/* Number of conv MACs one forward performs (for roofline reporting). */
double st_detector_macs(const StDetector* det);
/* Stereo configuration (with_right_branch=1), two phases around the cost-volume module:
 * phase 0 = stem+stage1 features of left AND right (shared RGB-branch weights, one stacked
 * batch of 2N; tap "stage1_rgb" = [2N][H/4][W/4][C]); phase 1 = disparity branch + fused trunk +
 * neck + head.  With with_right_branch=0 the two phases together equal st_detector_forward. */
int st_detector_forward_phase(StDetector* det, int phase, const float* img_dev,
                              const float* disp_dev, const float* right_dev, void* workspace_dev,
                              size_t workspace_bytes, st_stream_t stream, float* head_out_dev);
/* Phase 0 from RAW frames (see st_stem_focus_conv_u8): left / right = HOST arrays of `batch` device pointers to uint8
 * [3][h][w] frames; the detector's height x width is the padded size.  Requires the fused stem (always the case for the
 * shipped widths).  Results are bit-identical to st_pack_raw_frames + st_detector_forward_phase(det, 0, ...). */
int st_detector_forward_phase0_raw(StDetector* det, const unsigned char* const* left_frames_host,
                                   const unsigned char* const* right_frames_host, int h, int w, float pad_value,
                                   void* workspace_dev, size_t workspace_bytes, st_stream_t stream);
/* st_detector_forward (the disparity-INPUT configuration, the reference's shipped one) with the image as RAW frames:
 * img_frames_host = HOST array of `batch` device pointers to uint8 [3][h][w] frames, converted + padded inside the RGB
 * stem (see st_stem_focus_conv_u8); disp_dev = the fp32 (N,3,H,W) disparity input as before.  Bit-identical to
 * st_pack_raw_frames + st_detector_forward. */
int st_detector_forward_raw(StDetector* det, const unsigned char* const* img_frames_host, int h, int w,
                            float pad_value, const float* disp_dev, void* workspace_dev, size_t workspace_bytes,
                            st_stream_t stream, float* head_out_dev);
/* Per-op timing for bench.py / profiling.  When enabled every op (focus pack, conv, spp) of the
 * following forwards is bracketed by hipEvents on the caller's stream; st_detector_op_times
 * synchronises on them and returns, per op: elapsed ms, kind (0 focus, 1 conv, 2 spp, 3 the out_fd average), the kernel
 * instance that ran it (0..21 implicit-GEMM tiles, 40 fused stem, 41 streaming 1x1, 42 direct 3x3,
 * 43 / 44 Winograd, 45 fused front, 46 resident 1x1, 47 head prediction, 48 / 49 grouped Winograd launch
 * and its riders, 50..55 split-operand instances; names: st_conv_variant_name; -1 otherwise), conv MACs, phase. */
int st_detector_set_timing(StDetector* det, int enable);
int st_detector_num_ops(const StDetector* det);
int st_detector_op_times(StDetector* det, int cap, float* ms, int* kind, int* variant, double* macs,
                         int* phase);
int st_detector_op_desc(const StDetector* det, int i, char* buf, int cap);
/* Which launch computed each op at the most recent forward (no timing events needed): owner[i] = i for an op with a
 * launch of its own, the index of the FIRST op for the riders of a fused (45, 56), chained (41, 46) or grouped
 * (48 / 49) launch, -1 for an op that has not run yet.  variant (may be NULL) = the instance per op as
 * st_detector_op_times reports it.  A chained rider reports the same instance as its owner; only `owner` tells a chain
 * from two launches. */
int st_detector_op_owner(const StDetector* det, int cap, int* owner, int* variant);
/* Measure every valid conv tile variant on every conv op's real shape and keep the fastest
 * (host-synchronous; call once after st_detector_finalize, never inside a timed region). */
/* Split-operand instances (tile variants 50-55 of st_conv2d_nhwc_variant): the same implicit GEMM with every fp32 operand
 * split into three bf16 terms (error-free: 3 x 8 = 24 mantissa bits), six exact term products on
 * v_mfma_f32_32x32x16_bf16, fp32 accumulate.  PARKED (round 5): the plan built from them did not pass the frozen parity
 * gate (profiles/r05_gpu_tests_split_plan.log) and bought +0.7 % in flight, so they exist in the TOOLS build only
 * (make ABLATION=1).  st_split_instances_available() = 1 there, 0 in the product library, where
 * st_detector_set_split(det, allow != 0) and variants 50-55 return an error; st_detector_set_split(det, 0) is a no-op. */
int st_split_instances_available(void);
int st_detector_set_split(StDetector* det, int allow);
int st_detector_autotune(StDetector* det, void* workspace_dev, size_t workspace_bytes,
                         float* head_out_dev, st_stream_t stream, int reps);
const char* st_conv_variant_name(int id);
const char* st_conv_variant_signature(int id); /* template args of the variant's kernel (profiler row matching) */
/* Per-op tile choice (one int per op of st_detector_num_ops, -1 = heuristic): read it after an
 * autotune, restore it in another process to skip the measurement. */
int st_detector_get_tuning(const StDetector* det, int* variants, int cap);
int st_detector_set_tuning(StDetector* det, const int* variants, int n);
/* Internal NHWC activations inside the workspace (valid after forward); name in
 * {"stage1_rgb","stage1_fused","stage2","stage3","stage4","p3_inner","p3","p4","p5"}, and "stage1_disp" in an
 * out_fd plan (valid until the end of the forward, like "p3").  Pixel p, channel c is ptr[p*ld + c]. */
int st_detector_tap(const StDetector* det, const char* name, const void* workspace_dev,
                    const float** ptr_dev, int* N, int* C, int* H, int* W, int* ld);
/* The prediction convolutions of the decoupled head on their own (instance 47 of the plan): per level conv_cls
 * (feat -> 1) on the cls tower and conv_reg | conv_obj (feat -> 4 | 1) on the reg tower, all three levels in ONE
 * launch.  Pixel m of a level reads cls_dev[m * cls_ld + cls_off + c] / reg_dev[...], c < feat, and writes its 32-byte
 * head row out_dev[m * 8 + 0..5] = [cls | x y w h | obj]; floats 6, 7 of a row and rows >= M are not written.
 * wgt_* / bias_* = st_conv_pack_weights of the 1 x feat and the stacked 5 x feat (reg rows, then obj) 1x1 weights.
 * feat in {96, 128, 256} and num_classes == 1 only (ST_ERR_INVALID otherwise, nothing launched); tensors 16-byte
 * aligned, strides / offsets multiples of 4, M > 0. */
typedef struct StHeadPredLevel {
  const float* cls_dev;
  int cls_ld, cls_off;
  const float* reg_dev;
  int reg_ld, reg_off;
  const float* wgt_cls_dev;
  const float* bias_cls_dev;
  const float* wgt_reg_dev;
  const float* bias_reg_dev;
  float* out_dev;
  int M;
} StHeadPredLevel;
int st_head_pred(const StHeadPredLevel levels[3], int feat, int num_classes, st_stream_t stream);

/* ------------------------------------------------------------------------
 * 4. Decode + score filter + sort + NMS.
 *    Replaces mmyolo YOLOXHead.predict_by_feat -> YOLOXBBoxCoder.decode ->
 *    mmdet filter_scores_and_topk -> mmcv.ops.batched_nms
 *    (un-vendored; call site reference yolo_detector_disparity_v1.py:121-122,
 *    thresholds configs/stereo_tracking/ocsort/yolox_s_mmyolo_mot_airdrone_disp.py:42).
 * ---------------------------------------------------------------------- */
typedef struct StDecodeDesc {
  int struct_size;
  int batch;
  int num_levels;
  int level_h[4], level_w[4], level_stride[4];
  size_t level_offset[4]; /* float offset of level l inside head_out */
  float score_thr;        /* keep score > thr  */
  float iou_thr;          /* suppress IoU > thr */
  int max_det;            /* capacity of the out_* arrays per image */
  float scale_x, scale_y; /* scale_factor (w,h); boxes /= scale before NMS */
  float pad_left, pad_top;/* pad_param subtracted before scaling (0 if none) */
  float ori_w, ori_h;     /* clamp range after NMS */
  int nms_mask_rows;      /* candidates (in score order) whose pairwise IoU bits are precomputed chip-wide;
                           * 0 = default 4096.  Sizes the workspace (rows^2 / 8 bytes per image); later
                           * candidates are resolved on the fly by one wave - results do not depend on it */
  int num_classes;        /* 0 / 1: one class (the shipped config).  2..1024: head rows carry num_classes class logits
                           * (then x, y, w, h, obj; st_head_row_floats(num_classes) floats per row); multi_label
                           * decode - every (prior, class) pair with score > thr is a candidate, in
                           * filter_scores_and_topk's order - and class-aware NMS by mmcv batched_nms's offset trick
                           * (boxes + label * (max coordinate + 1)); out_labels = class, out_prior_idx = prior */
  int single_label;       /* with several classes: test_cfg.multi_label = False - ONE candidate per prior, the class of
                           * its largest score sigmoid(cls_c) * sigmoid(obj) (first maximum on ties; mmyolo
                           * predict_by_feat: scores.max(1)), thresholded afterwards; NMS stays class-aware */
} StDecodeDesc;

/* Floats per prior in head_out: 8 for 1..3 classes (cls.., x, y, w, h, obj, padding), num_classes + 5 rounded up to a
 * multiple of 4 beyond. */
int st_head_row_floats(int num_classes);

size_t st_decode_nms_workspace_bytes(const StDecodeDesc* d);
/* outputs per image n: out_boxes[n][max_det][4] (xyxy), out_scores[n][max_det],
 * out_labels[n][max_det] (int64), out_prior_idx[n][max_det] (flat prior index,
 * the bit-exact identity of a kept box), out_count[n] = number kept (may exceed
 * max_det: then only the first max_det are stored - the reference applies NO cap under
 * yolox_style=True, so callers must treat out_count[n] > max_det as an overflow and re-run with a
 * larger buffer or raise; rows past min(count, max_det) are written as zero, prior index -1).
 * workspace_dev and out_boxes_dev must be 16-byte aligned; with 1..3 classes (8-float rows) head_out_dev too, and every
 * level_offset a multiple of 4 (ST_ERR_INVALID, nothing launched, otherwise). */
int st_decode_nms(const StDecodeDesc* d, const float* head_out_dev, void* workspace_dev,
                  size_t workspace_bytes, st_stream_t stream, float* out_boxes_dev,
                  float* out_scores_dev, int64_t* out_labels_dev, int32_t* out_prior_idx_dev,
                  int32_t* out_count_dev);

/* ------------------------------------------------------------------------
 * 5. Stereo cost volume -> soft-argmin disparity (NEW module named by
 *    north_star; no reference function exists — consumer contract is
 *    reference loading_disparity.py:129-134 and ocsort_disparity.py:115,132-134).
 *    featL/featR: NHWC [N][Hf][Wf][C].  cost[d] = (1/C) sum_c L[x,c]*R[x-d,c]
 *    (0 where x-d<0); disp_lowres = sum_d d*softmax_d(temperature*cost[d]).
 *    out_cost_dev (optional) receives the materialised volume [N][Hf][Wf][D].
 *    featL_dev / featR_dev must be 16-byte aligned, C and feat_ld multiples of 4
 *    (ST_ERR_INVALID otherwise).  The volume pointers (out_cost_dev here, cost_dev
 *    of st_softargmin, disp_postp_dev of st_disp_upsample_pack) take any float
 *    alignment: one that is not 16-byte aligned runs a scalar kernel, same bits.
 * ---------------------------------------------------------------------- */
int st_costvolume_softargmin(const float* featL_dev, const float* featR_dev, int N, int Hf,
                             int Wf, int C, int feat_ld, int D, float temperature,
                             float* out_cost_dev, float* out_disp_dev, st_stream_t stream);
/* One 3-D aggregation layer on the materialised volume [N][Hf][Wf][D] (north_star: "its 3D/2D aggregation"; no
 * reference function - the specification is oracle/st_oracle.c::oracle_agg3d, bit-exact): a single-channel 3x3x3
 * convolution over (d, y, x), zero padded, out = act(bias + sum w[kD][kH][kW] * vol[d+kD-1, y+kH-1, x+kW-1]),
 * act = SiLU (1) or none (0).  weight27_host: the 27 taps in (kD, kH, kW) order, HOST memory (they travel in the
 * kernel arguments).  vol_in != vol_out, 16-byte aligned, D a multiple of 4 (<= 192). */
int st_volume_agg3d(const float* vol_in_dev, float* vol_out_dev, int N, int Hf, int Wf, int D,
                    const float* weight27_host, float bias, int act, st_stream_t stream);
/* Cost volume and the FIRST 3-D aggregation layer in one pass (the volume between them never reaches memory):
 * vol_out = agg3d(costvolume(featL, featR)), cell for cell the arithmetic of st_costvolume_softargmin's volume followed by
 * st_volume_agg3d (specification: oracle_costvolume then oracle_agg3d, bit-exact).  featL/featR: NHWC [N][H][W][ld],
 * channels [0, C) used.  Built for the full-resolution mode of the stereo module (north_star's D = 192 sizing; no
 * reference function, consumer contract as for st_costvolume_softargmin).  C in {4, 8, 16}, D a multiple of 4 (<= 192):
 * st_costvolume_agg3d_supported(C, D) tells (1/0); other shapes take the two calls above. */
int st_costvolume_agg3d_supported(int C, int D);
int st_costvolume_agg3d(const float* featL_dev, const float* featR_dev, int N, int H, int W, int C, int feat_ld, int D,
                        const float* weight27_host, float bias, int act, float* vol_out_dev, st_stream_t stream);
/* Round 6: the same pass with the SOFT-ARGMIN of the aggregated volume taken inside the kernel - for a stereo module whose
 * only 3-D layer this is (StereoCostVolume(full_res=True, agg3d_layers=1)): the D-level volume (4 D bytes per pixel, 5.8 GB
 * per 8 pairs at D = 192 x 736 x 1280) is neither written nor read back.  disp_out_dev [N][H][W] px (float), as
 * st_softargmin writes it; bit-equal to st_costvolume_agg3d followed by st_softargmin (specification
 * oracle_costvolume -> oracle_agg3d -> oracle_softargmin).  Needs st_costvolume_agg3d_supported(C, D) and D in {48, 96, 192}
 * (ST_ERR_INVALID otherwise: the caller takes st_costvolume_agg3d + st_softargmin, same results). */
int st_costvolume_agg3d_softargmin(const float* featL_dev, const float* featR_dev, int N, int H, int W, int C, int feat_ld,
                                   int D, const float* weight27_host, float bias, int act, float temperature,
                                   float* disp_out_dev, st_stream_t stream);
/* soft-argmin only, on an (aggregated) volume [N][Hf][Wf][D] */
int st_softargmin(const float* cost_dev, int N, int Hf, int Wf, int D, float temperature,
                  float* out_disp_dev, st_stream_t stream);
/* bilinear (align_corners=False) x`scale` upsample of the low-res disparity,
 * multiplied by `scale`, cropped to (valid_h, valid_w), zero elsewhere, written
 * replicated into the 3 channels of disp_postp NCHW [N][3][H][W]. */
int st_disp_upsample_pack(const float* disp_lr_dev, int N, int Hf, int Wf, int scale, int H,
                          int W, int valid_h, int valid_w, float* disp_postp_dev,
                          st_stream_t stream);

/* LEFT-RIGHT CHECK of the stereo module (StereoCostVolume(lr_check=True); csrc/lr_check.hip).  NEW, no reference function
 * (as for the module itself); the consumer contract is the one above: 0 = invalid in disp_postp
 * (loading_disparity.py:85-86,129-134; extract_depth keeps 0 < depth < 150, ocsort_disparity.py:136-175).  Levels are the
 * unit; s = `scale` is the level spacing in image pixels.  With V [N][H][W][D] the volume st_softargmin reads:
 *   1  dL = st_softargmin(V)
 *   2  VR[n][y][x'][d] = V[n][y][x'+d][d] if x'+d < W, else 0
 *   3  dR = softargmin(VR) in the operation order of oracle_softargmin (maximum first, then d ascending)
 *   4  r = (int)floorf(dL + 0.5f), xr = x - r; (y, x) is invalid if dL is not finite, xr < 0 (or xr >= W), or
 *      !(fabsf(dL - dR[y][xr]) * (float)s <= lr_max_diff)   (NaN fails; a difference equal to lr_max_diff is valid)
 *   5  disp_postp[n][c][Y][X] = valid(Y / s, X / s) ? the value st_disp_upsample_pack writes : +0;
 *      disp_mask[n][0][Y][X] = valid ? 1 : 0 inside (valid_h, valid_w), 0 outside.
 * st_softargmin_right: rules 2 + 3 -> out_disp_right_dev [N][H][W] (levels).  Any D >= 1 (16-byte loads when D % 4 == 0
 * and vol_dev is 16-byte aligned), any W >= 1 (W < D included), bit-equal to oracle_softargmin on the sheared volume. */
int st_softargmin_right(const float* vol_dev, int N, int H, int W, int D, float temperature,
                        float* out_disp_right_dev, st_stream_t stream);
/* st_lr_check_pack: rules 4 + 5 in one pass.  disp_left_dev / disp_right_dev [N][Hl][Wl] (levels), H == Hl * scale,
 * W == Wl * scale, lr_max_diff >= 0 in image pixels; disp_postp_dev [N][3][H][W], disp_mask_dev [N][1][H][W] or NULL.
 * A valid pixel's disparity is bit-identical to st_disp_upsample_pack's on the same disp_left. */
int st_lr_check_pack(const float* disp_left_dev, const float* disp_right_dev, int N, int Hl, int Wl, int scale, int H,
                     int W, int valid_h, int valid_w, float lr_max_diff, float* disp_postp_dev, float* disp_mask_dev,
                     st_stream_t stream);

/* Bilinear x`scale` upsampling (align_corners=False) of an NHWC feature map [N][Hf][Wf][C] (pixel stride feat_ld floats)
 * to [N][Hf*scale][Wf*scale][C] dense: the feature side of the stereo module's FULL-RESOLUTION mode
 * (StereoCostVolume(full_res=True): the D = max_disp level volume of north_star's sizing, D x H x W, built at image
 * resolution from reduced + upsampled stage-1 features).  NEW, no reference function; specification
 * oracle/st_oracle.c::oracle_feat_upsample (bit-exact).  Consumer contract of the module's output as for
 * st_disp_upsample_pack: mmtrack/datasets/transforms/loading_disparity.py:85-86,129-134. */
int st_feat_upsample(const float* feat_dev, int N, int Hf, int Wf, int C, int feat_ld, int scale,
                     float* out_dev, st_stream_t stream);

/* ------------------------------------------------------------------------
 * 6. Per-box depth (disp2depth + extract_depth + scale), reference
 *    mmtrack/models/mot/ocsort_disparity.py:113-175 and
 *    mmtrack/models/trackers/utils.py:58-73.
 *    disp: channel 0 of disp_postp, [N][H][W] with row pitch W and image pitch
 *    img_pitch floats.  boxes [N][max_det][4], counts[N].
 *    outputs: depth[N][max_det] (-1 = no valid depth), scale[N][max_det],
 *    scaled_boxes[N][max_det][4].
 *    boxes_dev and out_scaled_boxes_dev (box rows move as 16 bytes) must be
 *    16-byte aligned, as boxes_dev / scaled_boxes_dev of st_pack_records
 *    (ST_ERR_INVALID otherwise).
 * ---------------------------------------------------------------------- */
size_t st_box_depth_workspace_bytes(int N, int max_det, int H, int W);
int st_box_depth(const float* disp_dev, size_t img_pitch, int N, int H, int W,
                 const float* boxes_dev, const int32_t* counts_dev, int max_det, float baseline,
                 float focal, void* workspace_dev, size_t workspace_bytes, st_stream_t stream,
                 float* out_depth_dev, float* out_scale_dev, float* out_scaled_boxes_dev);

/* Per-box depth estimators: the reference's default extract_depth and the four alternatives of its depth-extraction
 * comparison (mmtrack/models/mot/depth_extraction_comparison.py).  All share the default's window, validity rule
 * (0 < depth < 150) and discard rule (no valid depth or w > 800 => depth -1, scale 1); the alternatives scale by
 * max(min(d * d / 400, 3), 1) (tests/depth_methods_ref.py):
 *   TRUNCATED_MEAN  mean of sorted[int(0.1 n) : int(0.9 n)] (empty => sorted[:-1]; n == 1 => NaN)
 *   MEAN            mean of the valid depths
 *   MEDIAN          np.median of the valid depths
 *   CENTER          raw depth[(y1 + y2) // 2, (x1 + x2) // 2] (numpy wrap; out of range => -1, scale 1) */
enum {
  ST_DEPTH_REFERENCE = 0,
  ST_DEPTH_TRUNCATED_MEAN = 1,
  ST_DEPTH_MEAN = 2,
  ST_DEPTH_MEDIAN = 3,
  ST_DEPTH_CENTER = 4
};

/* st_box_depth with the estimator `method` (ST_DEPTH_*; another value => ST_ERR_INVALID).  ST_DEPTH_REFERENCE launches
 * exactly what st_box_depth launches.  Same grid (one workgroup per box), same outputs. */
int st_box_depth_method(const float* disp_dev, size_t img_pitch, int N, int H, int W,
                        const float* boxes_dev, const int32_t* counts_dev, int max_det, float baseline,
                        float focal, void* workspace_dev, size_t workspace_bytes, st_stream_t stream,
                        float* out_depth_dev, float* out_scale_dev, float* out_scaled_boxes_dev, int method);

/* Frame records: the fixed-size, self-describing unit of the detection all-gather and of the ONE
 * device->host copy per chunk of the MOT shell: out (N, max_det + 1, cols) fp32, row 0 = [true count (may exceed
 * max_det = overflow), max_det, valid-frame flag, 0...], rows 1.. = x1,y1,x2,y2,score,label,depth,scale.
 * mode 0: unscaled boxes (what reference mmtrack/models/mot/ocsort_disparity.py:107-108 returns as pred_det_instances),
 * mode 1: the depth-scaled boxes the tracker consumes (:82-86), cols = 8; mode 2: unscaled box first, scaled box and
 * kept prior index appended, cols = 13.  Frames >= n_real are batch padding (header all zero).  One launch. */
int st_pack_records(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const float* depth_dev,
                    const float* scales_dev, const float* scaled_boxes_dev, const int32_t* prior_idx_dev,
                    const int32_t* counts_dev, int N, int max_det, int mode, int n_real, float* out_records_dev,
                    st_stream_t stream);
/* rows k >= min(counts[n], max_det) of the three outputs are written as 0 (never stale). */

/* ------------------------------------------------------------------------
 * 7. Linear assignment of the CPU association step (HOST function, no GPU):
 *    replaces `lap.lapjv(dists, extend_cost=True, cost_limit=1 - match_iou_thr)`,
 *    reference mmtrack/models/trackers/ocsort_tracker_disparity.py:260-261, :312-313.
 *    cost: row-major float64 [n_rows][n_cols] (tracks x detections).
 *    x_out[n_rows] = column matched to row i or -1; y_out[n_cols] = row matched to
 *    column j or -1.  Dense Jonker-Volgenant on lap's (n_rows+n_cols)^2 extension, so
 *    that non-unique optima resolve as they do there.  NaN costs are unmatchable.
 * ---------------------------------------------------------------------- */
int st_lapjv_extended(const double* cost, int n_rows, int n_cols, double cost_limit,
                      int32_t* x_out, int32_t* y_out);

/* ------------------------------------------------------------------------
 * 8. The whole association step of one frame as a HOST routine (no GPU): the
 *    consumer of the detection records.  Reference
 *    OCSORTTracker_Disparity.track, mmtrack/models/trackers/ocsort_tracker_disparity.py:345-618
 *    (+ kalman_tracker_base.py:49-88, base_tracker.py:54-141, motion/kalman_filter.py:60-189);
 *    constructor kwargs = configs/stereo_tracking/ocsort/yolox_s_mmyolo_mot_airdrone_disp.py:49-58.
 *    dets[n][8] = x1,y1,x2,y2 (depth-SCALED box), score, label, depth, scale - one row of a frame
 *    record; out_rows / out_ids = pred_track_instances in the reference's output order
 *    (matched detections stage by stage, then the newly started tracks).
 * ---------------------------------------------------------------------- */
typedef struct StTracker StTracker;
typedef struct StTrackerConfig {
  int struct_size;
  float obj_score_thr, init_track_thr;
  int weight_iou_with_det_scores;
  float match_iou_thr;
  int num_tentatives;
  float vel_consist_weight;
  int vel_delta_t;
  int num_frames_retain;
} StTrackerConfig;
int st_tracker_create(const StTrackerConfig* cfg, StTracker** out);
int st_tracker_destroy(StTracker* t);
int st_tracker_reset(StTracker* t);
int st_tracker_track(StTracker* t, int frame_id, const float* dets, int n, float* out_rows,
                     int64_t* out_ids, int cap, int* out_n);
/* The same over a CHUNK of frame records (st_pack_records mode 2: (F, rows_per_frame, cols >= 12) fp32 in host memory,
 * e.g. the page-locked buffer the chunk's ONE device->host copy landed in): for every valid frame f the detections
 * (depth-scaled box, score, label, depth, scale) feed st_tracker_track with frame_ids[f]; out_rows (F, cap, 8) /
 * out_ids (F, cap) receive pred_track_instances with the box UNSCALED again (scale_bbox(b, 1 / scale), reference
 * mmtrack/models/mot/ocsort_disparity.py:88-97); out_counts[f] = rows written, -1 for batch-padding frames.  A frame
 * whose record says count > capacity returns ST_ERR_WORKSPACE (the DetectionOverflow of the Python side). */
int st_tracker_track_records(StTracker* t, const int* frame_ids, const float* records, int F, int rows_per_frame,
                             int cols, float* out_rows, int64_t* out_ids, int cap, int* out_counts);
/* state inspection (tests, checkpointing): live tracks in creation order */
int st_tracker_num_tracks(const StTracker* t);
long long st_tracker_next_id(const StTracker* t);
int st_tracker_get_track(const StTracker* t, int index, int64_t* id, double* mean8, double* cov64,
                         int* tentative, int* tracked, int* last_frame);
/* EVERYTHING a track knows (tests/test_cpu_tracker_state.py, tests/test_tracker_state_gpu.py): the fields the host
 * tracker's tracks and the device tracker's (section 9) share, in one layout, so that the two can be compared field for
 * field.  mean / cov: the float64 Kalman state; saved_*: the filter observation-centric recovery restores (all zero
 * until the track's first predict as a confirmed, tracked track); win / win_valid: the last win_len <= vel_delta_t + 1
 * entries of the observation history, OLDEST FIRST (win_valid 0 = the frame had no detection for the track: that row is
 * zero), slots >= win_len zero; n_obs: entries ever pushed; last_valid: the last detection; trailing_none: frames
 * since; vel: the velocity direction (dy, dx), vel_placeholder: it is the (-1, -1) "no velocity yet" value. */
#define ST_TRACK_WINDOW 8
typedef struct StTrackState {
  int struct_size;
  int tentative, tracked, last_frame, n_fed, win_len, trailing_none, vel_placeholder;
  int64_t id;
  int64_t n_obs;
  double mean[8], cov[64], saved_mean[8], saved_cov[64];
  float win[ST_TRACK_WINDOW][4];
  int win_valid[ST_TRACK_WINDOW];
  float last_valid[4];
  float vel[2];
} StTrackState;
/* All live tracks in creation order -> out[0 .. *out_n), *next_id = the id the next new track gets.  Read-only.
 * struct_size = sizeof(StTrackState) of the caller.  cap < live tracks, or a tracker whose window (vel_delta_t + 1) is
 * longer than ST_TRACK_WINDOW: ST_ERR_INVALID. */
int st_tracker_get_states(const StTracker* t, StTrackState* out, int cap, int struct_size, int* out_n,
                          long long* next_id);


/* ------------------------------------------------------------------------
 * 9. Batched GPU association: the SAME association step (section 8) for `batch` independent
 *    sequences advanced in lockstep on the device, one wave per sequence and frame; state stays in device memory
 *    between steps.  Results (ids, rows, order) equal st_tracker_track's on the same detections.  For many short
 *    sequences per step (multi-camera serving); for one video the host routine is the faster one.
 *    dets (batch, max_dets, 8) = rows of frame records (depth-scaled box, score, label, depth, scale), counts[b] = rows
 *    of sequence b in this step (-1: sequence b has no frame in this step), frame_ids[b] (0 resets sequence b).
 *    state / scratch: caller-owned device buffers of st_batched_tracker_{state,scratch}_bytes (state zero-filled
 *    before the first step).  out_rows (batch, max_dets, 8), out_ids (batch, max_dets), out_counts (batch),
 *    status (batch): 0 ok, 1 = more than max_tracks live tracks, 2 = counts[b] > max_dets (that sequence's
 *    output count is 0; the caller checks status).  A non-zero status is STICKY: the overflow is detected after the
 *    association has mutated the sequence's tracks, so the sequence is invalid from then on and every later step
 *    reports the same status with an output count of 0 until a step with frame_id 0 resets it.
 *    Enqueued on `stream`, no host sync.
 * ---------------------------------------------------------------------- */
typedef struct StBatchedTracker StBatchedTracker;
int st_batched_tracker_create(const StTrackerConfig* cfg, int batch, int max_tracks, int max_dets,
                              StBatchedTracker** out);
int st_batched_tracker_destroy(StBatchedTracker* t);
size_t st_batched_tracker_state_bytes(const StBatchedTracker* t);
size_t st_batched_tracker_scratch_bytes(const StBatchedTracker* t);
int st_batched_tracker_step(StBatchedTracker* t, const int32_t* frame_ids_dev, const float* dets_dev,
                            const int32_t* counts_dev, void* state_dev, void* scratch_dev, float* out_rows_dev,
                            int64_t* out_ids_dev, int32_t* out_counts_dev, int32_t* status_dev, st_stream_t stream);
/* State read-back of sequence b from the caller's state_dev (tests): the live tracks in slot (= creation) order ->
 * out_host[0 .. *n_tracks) (HOST memory, the StTrackState of section 8), *next_id, *status = the sequence's sticky
 * status.  The copies are enqueued on `stream`, i.e. after the steps already enqueued there, and the call waits for
 * them; state_dev is only read.  A sequence with a non-zero status reports it with *n_tracks = 0 (its slots are not a
 * tracker state any more).  cap < live tracks: ST_ERR_INVALID. */
int st_batched_tracker_get_states(const StBatchedTracker* t, const void* state_dev, int b, StTrackState* out_host,
                                  int cap, int struct_size, int* n_tracks, long long* next_id, int* status,
                                  st_stream_t stream);

/* ------------------------------------------------------------------------
 * 10. Mesh-Affine camera-motion compensation (CMC) of the tracker (reference OCSORTTracker_Disparity(cmc=dict(
 *     method='glme_affine', glme=dict(step, winsize, ransac_thr, min_inlier_ratio)))): the estimate on the device
 *     (csrc/cmc_flow.hip; every OpenCV rule restated [upstream-memory], see DESIGN.md "Camera-motion compensation"),
 *     the application to the Kalman states in the tracker routines of section 8.
 *   front    frames -> equalised 255 x 255 uint8 grey planes (crop to (h, w), BGR -> RGB, 8-bit INTER_LINEAR resize,
 *            RGB2GRAY, equalizeHist), one workgroup per frame.  From N separate uint8 (3, fh, fw) device frames (host
 *            array of device pointers, as st_pack_raw_frames) or from a padded fp32 (N, 3, H, W) batch (values cast
 *            to uint8); both give the same planes.
 *   flow     plane pairs (prev[n], curr[n]) -> dense Farneback flow (N, 255, 255, 2) fp32 (pyr_scale 0.5, levels 5,
 *            iterations 3, poly_n 5, poly_sigma 1.2, flags 0); levels_out (optional): every pyramid level's final flow,
 *            levels finest first, (N, sum of side^2, 2) (st_cmc_num_levels gives the sides).
 *   estimate plane pairs -> warps (N, ST_CMC_WARP_FLOATS) = {valid, inlier ratio, a00, a01, a02, a10, a11, a12}
 *            (the 2 x 3 warp in the coordinates of the (img_h, img_w) crop), via flow, per-cell medians and a
 *            deterministic exhaustive consensus similarity fit (stated deviation from cv2's RANSAC); mesh_out
 *            (optional, N x points x 4: src x, y, dst x, y) and inliers_out (optional, N x points uint8).
 *   ws: caller-owned device workspace of st_cmc_workspace_bytes(N), 8-byte aligned for the entries that fit (it holds
 *            64-bit keys; ST_ERR_INVALID otherwise).  Enqueued on `stream`, no host sync.
 * ---------------------------------------------------------------------- */
#define ST_CMC_SIDE 255
#define ST_CMC_WARP_FLOATS 8
typedef struct StCmcParams {
  int struct_size;        /* sizeof(StCmcParams) */
  int step;               /* mesh cell side (8..16; reference default 16) */
  int winsize;            /* Farneback box window (odd; default 31) */
  float ransac_thr;       /* inlier: squared residual <= ransac_thr^2 (default 5.0) */
  float min_inlier_ratio; /* valid = inliers / points >= this (default 0.3) */
} StCmcParams;
int st_cmc_num_levels(int* sides);
size_t st_cmc_workspace_bytes(int N);
int st_cmc_front_u8(const void* const* frames_u8_dev_ptrs_host, int N, int fh, int fw, int h, int w, void* planes_dev,
                    st_stream_t stream);
int st_cmc_front_f32(const float* batch_dev, int N, int H, int W, int h, int w, void* planes_dev, st_stream_t stream);
int st_cmc_flow(const void* prev_planes_dev, const void* curr_planes_dev, int N, int winsize, void* ws, size_t ws_bytes,
                float* flow_out_dev, float* levels_out_dev, st_stream_t stream);
int st_cmc_estimate(const void* prev_planes_dev, const void* curr_planes_dev, int N, int img_h, int img_w,
                    const StCmcParams* params, void* ws, size_t ws_bytes, float* warps_out_dev, float* mesh_out_dev,
                    unsigned char* inliers_out_dev, st_stream_t stream);
/* The two later stages of st_cmc_estimate entered directly (the same launches; test-facing, no product caller).
 * st_cmc_mesh_fit: a device flow field (N, 255, 255, 2) fp32 in place of the two planes, copied into the workspace where
 * st_cmc_flow leaves its own, then mesh -> fit with `params` (winsize unused); outputs as st_cmc_estimate.  The flow must
 * be free of NaN: a NaN has no rank, the cell's median is left unset and its mesh row is undefined (as it is for a NaN
 * out of the Farneback solve, which the regularised determinant rules out for finite planes).
 * st_cmc_fit: device points (N, P, 4) fp32 {src x, src y, dst x, dst y}, 2 <= P <= 1024, straight into the consensus fit
 * with its two options; warps and inliers (optional, N x P uint8) as st_cmc_estimate.  Both refuse, before any launch, a
 * null pointer, N <= 0, a workspace under st_cmc_workspace_bytes(N), and a step / P outside their range. */
int st_cmc_mesh_fit(const float* flow_dev, int N, int img_h, int img_w, const StCmcParams* params, void* ws,
                    size_t ws_bytes, float* warps_out_dev, float* mesh_out_dev, unsigned char* inliers_out_dev,
                    st_stream_t stream);
int st_cmc_fit(const float* points_dev, int N, int P, float ransac_thr, float min_inlier_ratio, void* ws,
               size_t ws_bytes, float* warps_out_dev, unsigned char* inliers_out_dev, st_stream_t stream);
/* The tracker step of section 8 with camera-motion compensation: `warp` (2 x 3, row-major, float64) is applied to every
 * confirmed track's Kalman state right after the predict (reference gmc.py:20-45: mean[0:2] = R mean[0:2] + t,
 * mean[4:6] = R mean[4:6], mean[3], mean[7] *= s = sqrt(max(det R, 1e-12)), cov = M cov M^T); NULL = no warp.  The
 * caller decides, as the reference does, that a warp exists only for a frame of the non-empty branch
 * (st_tracker_cmc_needed). */
int st_tracker_cmc_needed(const StTracker* t, int frame_id, int n);
int st_tracker_track_cmc(StTracker* t, int frame_id, const float* dets, int n, const double* warp, float* out_rows,
                         int64_t* out_ids, int cap, int* out_n);
/* st_tracker_track_records with per-frame warps.  warps (F, ST_CMC_WARP_FLOATS) as st_cmc_estimate writes them,
 * warp_src[f] = frame id of the image the warp of frame f was estimated FROM (-1: none).  *cmc_prev (in / out) = frame
 * id of the tracker's previous CMC image (-1: none; frame id 0 resets it).  A frame of the non-empty branch uses
 * warps[f] when warp_src[f] == *cmc_prev, no warp when *cmc_prev == -1, and otherwise STOPS: the call returns ST_OK
 * with *stop_at = f (else F) and out_counts written for frames < f; the caller estimates the pair (*cmc_prev, frame f),
 * puts it in warps[f] / warp_src[f] and calls again from frame f. */
int st_tracker_track_records_cmc(StTracker* t, const int* frame_ids, const float* records, int F, int rows_per_frame,
                                 int cols, const float* warps, const int* warp_src, int* cmc_prev, float* out_rows,
                                 int64_t* out_ids, int cap, int* out_counts, int* stop_at);

/* ------------------------------------------------------------------------
 * 11. Stereo matching: OpenCV StereoSGBM in mode SGBM_3WAY (the matcher behind the reference's AirDrone disparity PNGs,
 *     reproducibility.md section 3), restated from OpenCV 4.x [upstream-memory] in csrc/sgbm.hip; the rules are listed in
 *     tests/sgbm_ref.py and DESIGN.md "Stereo SGBM".  Every stage is integer arithmetic.
 *   input    N uint8 (3, fh, fw) left / right device frames (host arrays of device pointers, as st_pack_raw_frames),
 *            or padded fp32 (N, 3, H, W) batches with integral values; the top-left h x w is matched.  BGR; color = 0
 *            matches the fixed-point BGR2GRAY of the frames.  Both forms give the same bits.
 *   output   disp_postp (N, 3, H, W) fp32 = max(d16, 0) / 16 in all three channels, 0 outside h x w (the PNG
 *            loader's convention: invalid -> 0).
 *   limits   min_disparity 0; num_disparities in {16, 32, 48, 64} (one level per lane of a wave) or {128, 192, 256}
 *            (2, 3, 4 levels per lane) and < w; every other value is refused (ST_ERR_INVALID); w <= 4096; N h w < 2^31;
 *            block_size odd, 1..9;
 *            pre_filter_cap 1..127; parameter sets whose worst-case aggregated cost
 *            3 (block_size^2 cn (2 ftzero + 63) + max(P2, P1 + 1)) leaves int16 are refused (ST_ERR_INVALID).
 *   status   int on the device, written by every call that runs the speckle filter: 0 = every union-find loop
 *            converged; bit 0 / 1 = a find / link loop reached its bound (the result is then not the spec's).
 *   ws: caller-owned device workspace of st_sgbm_workspace_bytes(N, h, w, D), 8-byte aligned; the two int16 cost
 *   volumes in it take 2 N h (w - D) D bytes each, so the size passes 2^32 for large batches at D = 256 (size_t
 *   throughout).  Enqueued on `stream`, no host sync.
 *   Stage entry points (tests): st_sgbm_match_f32 -> the block-summed cost C (N, h, w - D, D) int16 and / or the int16
 *   disparity x 16 (N, h, w) after the left-right check, before the median (-16 invalid); st_sgbm_median (3 x 3,
 *   replicated borders); st_sgbm_speckle (filterSpeckles with newVal -16; out int16 and / or disp_postp, workspace
 *   2 N h w ints, each 256-byte aligned).
 * ---------------------------------------------------------------------- */
typedef struct StSgbmParams {
  int struct_size;         /* sizeof(StSgbmParams) */
  int num_disparities;     /* D: 16, 32, 48, 64, 128, 192 or 256 */
  int block_size;          /* odd */
  int P1, P2;              /* smoothness penalties; P2 is used as max(P2, P1 + 1) */
  int disp12_max_diff;     /* <= 0 is taken as 1 */
  int uniqueness_ratio;    /* percent, 0..99 (0 = no uniqueness test) */
  int speckle_window_size; /* 0 = no speckle filter */
  int speckle_range;       /* maxDiff = 16 * speckle_range */
  int pre_filter_cap;      /* ftzero = max(pre_filter_cap, 15) | 1 */
  int color;               /* 1: match the 3 BGR channels; 0: grey */
} StSgbmParams;
size_t st_sgbm_workspace_bytes(int N, int h, int w, int D);
int st_sgbm_u8(const void* const* left_ptrs_host, const void* const* right_ptrs_host, int N, int fh, int fw, int h,
               int w, const StSgbmParams* params, void* ws, size_t ws_bytes, float* disp_postp_dev, int H, int W,
               int* status_dev, st_stream_t stream);
int st_sgbm_f32(const float* left_dev, const float* right_dev, int N, int H, int W, int h, int w,
                const StSgbmParams* params, void* ws, size_t ws_bytes, float* disp_postp_dev, int* status_dev,
                st_stream_t stream);
int st_sgbm_match_f32(const float* left_dev, const float* right_dev, int N, int H, int W, int h, int w,
                      const StSgbmParams* params, void* ws, size_t ws_bytes, int16_t* cost_out_dev,
                      int16_t* disp_out_dev, st_stream_t stream);
int st_sgbm_median(const int16_t* in_dev, int N, int h, int w, int16_t* out_dev, st_stream_t stream);
int st_sgbm_speckle(const int16_t* in_dev, int N, int h, int w, int max_size, int max_diff, void* ws, size_t ws_bytes,
                    int16_t* out_dev, float* disp_postp_dev, int H, int W, int* status_dev, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 12. COCO bbox evaluation (the configs' evaluator, mmdet.CocoMetric -> pycocotools COCOeval), restated from
 *     pycocotools / mmdet 3.0.0rc4 [upstream-memory] in csrc/coco_eval.hip; the rules are listed in
 *     tests/coco_eval_ref.py and DESIGN.md "COCO bbox evaluation".  fp64 and integer counts throughout: the outputs
 *     are reproducible to the bit.
 *   rows     detections: float32 xyxy boxes (D, 4), float32 scores, int labels in [0, num_cats), int image index,
 *            NON-DECREASING (the concatenation of the per-image results in image order; equal scores keep row order);
 *            ground truth: float64 xywh (G, 4), float64 area, int crowd flag, int category, int image index
 *            (non-decreasing), on the device, plus host copies of the image index and category (checked before launch).
 *   tables   iou_thrs (T), area_rng (A, 2) [lo, hi], rec_thrs (R) fp64 on the device; max_dets (M) ints on the HOST,
 *            non-decreasing: the match is made at max_dets[M - 1], entry m keeps the first max_dets[m] of a group.
 *            T * A <= 64 (one lane of a wave per pair), A <= 16, M <= 16, R <= 128.
 *   limits   at most st_coco_max_gt() = ST_COCO_MAX_GT ground-truth boxes per (image, category): ST_ERR_INVALID above.
 *   outputs  det_rank (D) rank inside the (image, category) group, -1 beyond max_dets[M - 1]; det_matched /
 *            det_ignored (D) 64-bit tables, bit t * A + a (0 for rank -1); npig (K, A); precision (T, R, K, A, M),
 *            recall (T, K, A, M), scores (T, R, K, A, M) fp64, -1 where npig == 0.  Every cell is written.
 *   status   4 ints on the device, 0 = fine.  [0] bits: 1 det_img / 2 gt_img decreasing or out of range, 4 non-finite
 *            detection ([1] = D - its first row), 8 label out of range ([2] = D - row), 16 ground-truth overflow,
 *            32 gt category out of range.  Non-zero: the other outputs are not valid.
 *   Three stages, each enqueued on `stream` with a launch count independent of num_images and no host wait:
 *   st_coco_prepare (offsets, ranks, npig), st_coco_match (the two tables), st_coco_accumulate (sort + curves).
 *   ws: caller-owned device workspace of st_coco_workspace_bytes(args), shared by the three calls.
 * ---------------------------------------------------------------------- */
#define ST_COCO_MAX_GT 256
typedef struct StCocoArgs {
  int struct_size;              /* sizeof(StCocoArgs) */
  int num_images, num_cats, num_dets, num_gts;
  int T, A, M, R;
  const float* det_boxes;
  const float* det_scores;
  const int* det_labels;
  const int* det_img;
  const double* gt_boxes;
  const double* gt_area;
  const int* gt_crowd;
  const int* gt_cat;
  const int* gt_img;
  const int* gt_img_host;
  const int* gt_cat_host;
  const double* iou_thrs;
  const double* area_rng;
  const double* rec_thrs;
  const int* max_dets;          /* host */
  void* ws;
  size_t ws_bytes;
  int* det_rank;
  unsigned long long* det_matched;
  unsigned long long* det_ignored;
  int* npig;
  double* precision;
  double* recall;
  double* scores;
  int* status;
} StCocoArgs;
int st_coco_max_gt(void);
size_t st_coco_workspace_bytes(const StCocoArgs* args);
int st_coco_prepare(const StCocoArgs* args, st_stream_t stream);
int st_coco_match(const StCocoArgs* args, st_stream_t stream);
int st_coco_accumulate(const StCocoArgs* args, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 13. Multi-stream tracking (MultiStreamTracker): the device path of one TICK - at most one frame from each of
 *     `streams` videos - between the dense launch plan, the batched association of section 9 and the tick's ONE
 *     device->host copy (csrc/stream_track.hip).  The tick's frames occupy SLOTS: slot i is frame i % chunk of dense
 *     chunk i / chunk; the routing (stream_of_slot, frame_ids) and the chunks' buffer pointers are HOST arrays that
 *     travel in the kernel arguments - a tick needs no host->device copy.  Three launches, each enqueued on `stream`
 *     without a host wait:
 *   st_stream_gather   chunk_records[c] = the chunk's frame records (st_pack_records mode 2, (chunk, det_rows + 1, 13))
 *                      -> the tracker's input BY STREAM: dets (streams, max_dets, 8), counts (streams) = the TRUE
 *                      number kept, unclipped (above max_dets st_batched_tracker_step reports status 2), -1 for a stream
 *                      without a frame; frame_ids (streams); and the detection rows of the tick record.
 *   st_stream_unscale  the tracker's out_rows / out_counts -> scale_bbox(box, 1 / scale) (reference
 *                      mmtrack/models/mot/ocsort_disparity.py:95-97; the same single fp32 operations as
 *                      st_tracker_track_records) BY SLOT: boxes (chunk * num_chunks, max_dets, 4), box_counts
 *                      (chunk * num_chunks; 0 for padding slots) - st_box_depth's input, chunk c at slot c * chunk.
 *   st_stream_record   chunk_depth[c] / chunk_gt_depth[c] (NULL array: gt_depth = depth) = st_box_depth's depth output
 *                      of chunk c, (chunk, max_dets) -> the tick record.
 *   Tick record (st_stream_record_bytes, one buffer):
 *     int64   ids    [streams][max_dets]                     instances_id
 *     int32   header [streams][ST_STREAM_HDR_INTS]           track rows (-1: no frame in this tick), detections kept
 *                                                            (true count), tracker status (section 9), frame id
 *     float32 tracks [streams][max_dets][ST_STREAM_ROW_FLOATS]   unscaled box (4), score, label, scale, depth,
 *                                                            gt depth, 0
 *     float32 dets   [streams][det_rows][ST_STREAM_DET_FLOATS]   unscaled box (4), score, label, kept prior index, 0
 *   Rows past a stream's counts are not written.
 * ---------------------------------------------------------------------- */
#define ST_STREAM_MAX_STREAMS 128
#define ST_STREAM_HDR_INTS 4
#define ST_STREAM_ROW_FLOATS 10
#define ST_STREAM_DET_FLOATS 8
typedef struct StStreamTick {
  int struct_size;                 /* sizeof(StStreamTick) */
  int streams;                     /* <= ST_STREAM_MAX_STREAMS */
  int chunk, num_chunks;           /* chunk * num_chunks slots, <= ST_STREAM_MAX_STREAMS */
  int max_dets;                    /* rows per stream of the tracker's input and output */
  int det_rows;                    /* detection rows of a frame record (the dense plan's max_det) */
  const int32_t* stream_of_slot;   /* host, [chunk * num_chunks]: stream in [0, streams), each at most once; -1 = padding */
  const int32_t* frame_ids;        /* host, [streams]: read for the streams that have a slot */
} StStreamTick;
size_t st_stream_record_bytes(int streams, int max_dets, int det_rows);
int st_stream_gather(const StStreamTick* tick, const float* const* chunk_records, float* dets_dev, int32_t* counts_dev,
                     int32_t* frame_ids_dev, void* record_dev, st_stream_t stream);
int st_stream_unscale(const StStreamTick* tick, const float* rows_dev, const int32_t* out_counts_dev, float* boxes_dev,
                      int32_t* box_counts_dev, st_stream_t stream);
int st_stream_record(const StStreamTick* tick, const float* rows_dev, const int64_t* ids_dev,
                     const int32_t* out_counts_dev, const int32_t* status_dev, const int32_t* counts_dev,
                     const float* boxes_dev, const float* const* chunk_depth, const float* const* chunk_gt_depth,
                     void* record_dev, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 15. MOT evaluation (MOTDroneMetrics: CLEAR, Identity, HOTA) on the device, csrc/mot_eval.hip.  The rules are the
 *     statements of stereotracking_amd/metrics.py (clear_identity, hota); DESIGN.md section 15 lists what runs where.
 *     fp64 and integer counts throughout, no floating-point atomics: two runs give the same bits.
 *   rows     B sequences packed.  gt_rows (num_gt, 6) / pred_rows (num_pred, 6) fp64 = (frame number, DENSE id index
 *            in [0, ng) / [0, nt) of the row's sequence, x, y, w, h), grouped by sequence, sorted by frame.
 *   tables   built by the host (stereotracking_amd/mot_eval.py pack_sequences) and TRUSTED to be consistent:
 *            seq_frame_off (B + 1) first global frame of every sequence; the frames of a sequence are the union of
 *            its gt and prediction frames, ascending; frame_seq (F) sequence of a frame; frame_no (F) frame numbers;
 *            frame_gt_off / frame_pred_off (F + 1) first row of every frame; frame_pair_off (F + 1) first cell of the
 *            frame's G x P similarity matrix; seq_ng / seq_nt (B) id counts; seq_gid_off / seq_tid_off / seq_mat_off
 *            (B + 1) first element of a sequence's per-gt-id, per-tracker-id and ng x nt arrays (ragged).
 *            alphas (num_alphas <= ST_MOT_MAX_ALPHAS) fp64, passed from the host, never recomputed.
 *   limits   at most st_mot_max_objects() = ST_MOT_MAX_OBJECTS rows of either kind in one frame.  A frame above it
 *            sets status bit 8 and, with max_frame_objects filled in, st_mot_similarity returns ST_ERR_INVALID after
 *            launching the checks.  The number of ids per sequence is bounded by the workspace only.
 *   status   8 ints on the device, 0 = fine.  [0] bits: 1 non-finite box, 2 an id twice in one frame, 4 rows that are
 *            not sorted (a row's frame number is not its frame's, or frame numbers do not ascend), 8 a frame above the
 *            per-frame limit, 16 a dense id outside its sequence's range.  [1 + k] for bit 1 << k: num_frames - the
 *            global frame index of the first offender.  Non-zero: the later stages return at once, outputs are not valid.
 *   outputs  gt_count (sum ng) / tr_count (sum nt) ints; id_potential (sum ng nt) ints, frames with IoU >= iou_thr - eps;
 *            hota_potential (sum ng nt) fp64, bit-equal to the host's per-frame +=; gt_frames / gt_matched / gt_frag
 *            (sum ng) ints (MT / PT / ML / Frag bookkeeping); clear_counts (B, 4) TP FN FP IDSW; motp_sum (B);
 *            hota_counts (B, num_alphas, 3) TP FN FP; hota_sums (B, num_alphas, 4) = sum of IoU over the TPs and the
 *            AssA / AssRe / AssPr sums BEFORE the division by max(1, TP).  Identity's one global assignment, the
 *            divisions and the combination over videos stay on the host.
 *   Four stages, each enqueued on `stream`, launch count independent of the number of frames, no host wait:
 *   st_mot_similarity (checks, IoU, row / column sums), st_mot_walk (flags ST_MOT_CLEAR | ST_MOT_HOTA: counts, both
 *   potentials, CLEAR's matching in frame order, one wave per sequence), st_mot_hota_match (one assignment per frame),
 *   st_mot_hota_accumulate (per sequence and alpha).  ws: caller-owned, st_mot_workspace_bytes(args), shared.
 *   Order: st_mot_similarity first; st_mot_walk needs it and reads nothing a later stage writes, so it may be repeated
 *   (for another flags value) at any point after it; st_mot_hota_match needs st_mot_walk with ST_MOT_HOTA (the
 *   potential and the id counts), st_mot_hota_accumulate needs st_mot_hota_match.
 * ---------------------------------------------------------------------- */
#define ST_MOT_MAX_OBJECTS 256
#define ST_MOT_MAX_ALPHAS 32
#define ST_MOT_CLEAR 1
#define ST_MOT_HOTA 2
typedef struct StMotArgs {
  int struct_size;              /* sizeof(StMotArgs) */
  int num_seqs, num_frames, num_gt, num_pred, num_alphas;
  int max_frame_objects;        /* host's knowledge of the largest frame (0: unknown) */
  int flags;                    /* ST_MOT_CLEAR | ST_MOT_HOTA: what st_mot_walk accumulates */
  long long num_pairs;          /* frame_pair_off[F] */
  long long num_cells;          /* seq_mat_off[B] */
  long long num_gids, num_tids; /* seq_gid_off[B], seq_tid_off[B] */
  double iou_thr;
  const double* gt_rows;
  const double* pred_rows;
  const int* seq_frame_off;
  const int* frame_seq;
  const long long* frame_no;
  const int* frame_gt_off;
  const int* frame_pred_off;
  const long long* frame_pair_off;
  const int* seq_ng;
  const int* seq_nt;
  const long long* seq_gid_off;
  const long long* seq_tid_off;
  const long long* seq_mat_off;
  const double* alphas;
  void* ws;
  size_t ws_bytes;
  int* gt_count;
  int* tr_count;
  int* id_potential;
  double* hota_potential;
  int* gt_frames;
  int* gt_matched;
  int* gt_frag;
  int* clear_counts;
  double* motp_sum;
  int* hota_counts;
  double* hota_sums;
  int* status;
} StMotArgs;
int st_mot_max_objects(void);
int st_mot_max_alphas(void);
size_t st_mot_workspace_bytes(const StMotArgs* args);
/* byte offset of the similarity matrices (num_pairs fp64, frame f at frame_pair_off[f], row-major G x P) inside ws */
size_t st_mot_workspace_sim_offset(const StMotArgs* args);
int st_mot_similarity(const StMotArgs* args, st_stream_t stream);
int st_mot_walk(const StMotArgs* args, st_stream_t stream);
int st_mot_hota_match(const StMotArgs* args, st_stream_t stream);
int st_mot_hota_accumulate(const StMotArgs* args, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 16. KITTI 2-D box preprocessing (MOTKittiMetrics) on the device, csrc/mot_eval.hip.  The rules are the statements of
 *     stereotracking_amd/metrics.py kitti_preprocess: per frame and evaluated class one
 *     assignment between the ground truth of the class or its distractors and the predictions of the class; matched
 *     predictions on a distractor / occluded / truncated object and unmatched ones that are too small or inside an
 *     ignore region are removed; the ground truth kept is that of the class within the occlusion / truncation limits.
 *     fp64 and integers throughout, no atomics on the outputs, one launch: two runs give the same bytes.
 *   rows     all sequences packed, sorted by sequence and frame.  gt_rows (num_gt, 9) fp64 = (frame, id, class,
 *            truncation, occlusion, x1, y1, x2, y2); pred_rows (num_pred, 8) = (frame, id, class, x1, y1, x2, y2,
 *            score); ignore_rows (num_ignore, 5) = (frame, x1, y1, x2, y2).  Only class, truncation, occlusion and the
 *            boxes are read.
 *   tables   built by the host (stereotracking_amd/mot_eval.py kitti_keep_masks) and TRUSTED: frame_gt_off /
 *            frame_pred_off / frame_ignore_off (num_frames + 1) first row of every frame; frame_ws_off (num_frames + 1,
 *            64-bit) first cell of the frame's slot in ws: a frame whose rows of all classes make more than 64 x 64
 *            cells needs a slot of (gt rows) x (prediction rows) cells, any other frame may have an empty one (smaller
 *            matrices are solved out of LDS); num_ws_cells = frame_ws_off[num_frames].  class_table (num_classes, 5)
 *            int32: the class id, then up to 4 distractor ids, unused entries -1.
 *   consts   max_occlusion, max_truncation, min_height, match_thr (IoU of a match), ignore_thr (intersection over the
 *            prediction's area with an ignore region); eps = 2^-52 is added / subtracted as kitti_preprocess does.
 *   limits   at most ST_MOT_MAX_OBJECTS ground-truth rows of a class and its distractors, and as many prediction rows
 *            of the class, in one frame; more rows of other classes may share the frame.
 *   status   8 ints, 0 = fine, zeroed by the call.  [0] bits: 1 non-finite box (any row of the frame), 8 a frame above
 *            the limit, 32 a frame whose ws slot is too small.  [1 + k] for bit 1 << k: num_frames - the frame index
 *            of the first offender.  The frames that set a bit write nothing.
 *   outputs  gt_keep (num_classes, num_gt) / pred_keep (num_classes, num_pred) bytes, 1 = the row is scored for that
 *            class.  Both are zeroed by the call, so a row of another class holds 0.
 *   One stage, enqueued on `stream`, one kernel launch (one wave per frame and class), no host wait.
 *   ws: caller-owned, st_mot_kitti_workspace_bytes(args) (0: invalid sizes).
 * ---------------------------------------------------------------------- */
#define ST_MOT_KITTI_MAX_DISTRACTORS 4
typedef struct StMotKittiArgs {
  int struct_size;              /* sizeof(StMotKittiArgs) */
  int num_frames, num_classes, num_gt, num_pred, num_ignore;
  int max_frame_objects;        /* largest number of gt or prediction rows (all classes) in one frame; 0: unknown */
  long long num_ws_cells;       /* frame_ws_off[num_frames] */
  double max_occlusion, max_truncation, min_height, match_thr, ignore_thr;
  const double* gt_rows;
  const double* pred_rows;
  const double* ignore_rows;
  const int* frame_gt_off;
  const int* frame_pred_off;
  const int* frame_ignore_off;
  const long long* frame_ws_off;
  const int* class_table;
  void* ws;
  size_t ws_bytes;
  unsigned char* gt_keep;
  unsigned char* pred_keep;
  int* status;
} StMotKittiArgs;
size_t st_mot_kitti_workspace_bytes(const StMotKittiArgs* args);
int st_mot_kitti_preprocess(const StMotKittiArgs* args, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 17. Tracklet post-processing (InterpolateTracklets) on the device, csrc/tracklet_post.hip.  The rules are the
 *     statements of stereotracking_amd/tracklets.py (backend='host'): linear filling of frame
 *     gaps (ByteTrack) and Gaussian-smoothed interpolation (StrongSORT): per track the mean of a Gaussian-process
 *     regression with a fixed RBF kernel at the track's own frames, K (K + 1e-10 I)^-1 y for the four coordinates.
 *     fp64 throughout, no atomics, every sum in an order that depends on the track alone: a track's output bytes are
 *     the same from run to run, alone or among other tracks, in one launch or several.
 *   rows     (num_rows, 7) fp64 = (frame, id, c0, c1, c2, c3, score): the kept tracks of all prediction sets, a
 *            track's rows contiguous and ascending in frame.  out_rows (num_out_rows, 7): the same tracks with the
 *            filled rows in place, in the same order.
 *   tables   built by the host (tracklets.py) from the frame numbers alone: row_out_off (num_rows) the output row of
 *            every input row; row_gap (num_rows) g = the frame gap to the next row of the track when it is filled
 *            (the g - 1 rows after row_out_off), else 0; trk_out_off (num_tracks + 1) first output row of every track;
 *            trk_order (num_tracks) the tracks by descending row count; trk_len_scale (num_tracks) the RBF length
 *            scale.  A table entry that points outside the buffers writes nothing and sets status bit 2.
 *   status   (num_tracks) ints, zeroed by st_tracklet_interpolate.  Bits: 1 a Cholesky pivot <= 0 (or not a number):
 *            the track's coordinates are left unsmoothed; 2 a table entry out of range (st_tracklet_gsi: in the
 *            track's word; st_tracklet_interpolate knows rows, not tracks, and sets it in word 0).
 *   st_tracklet_interpolate   one thread per input row: copies it and writes the filled rows j = 1 .. g - 1 as
 *            j / g * (right - left) + left, unfused fp64 operations in this order, score 1.
 *   st_tracklet_gsi           after st_tracklet_interpolate, in place on out_rows, for the tracks
 *            trk_order[first .. first + count): num_groups persistent workgroups, workgroup b takes the entries
 *            b, b + num_groups, ...  One track per workgroup at a time: K, a blocked right-looking Cholesky
 *            factorisation of K + 1e-10 I (blocks of 16 columns), the two triangular solves with the four right-hand
 *            sides and K alpha.  Tracks of at most 128 rows keep the matrix in LDS; longer ones, up to
 *            st_tracklet_max_rows(), use a slot of ws per WORKGROUP with the panel in LDS.  max_rows: the rows of the
 *            longest track of the range (sizes the slots).  ws: caller-owned, st_tracklet_gsi_workspace_bytes(args)
 *            (0: invalid sizes).  Enqueued on `stream`, no host wait, no allocation.
 * ---------------------------------------------------------------------- */
typedef struct StTrackletArgs {
  int struct_size;              /* sizeof(StTrackletArgs) */
  int num_rows, num_out_rows, num_tracks;
  int first, count;             /* st_tracklet_gsi: the range of trk_order of this launch */
  int num_groups;               /* st_tracklet_gsi: workgroups of this launch */
  int max_rows;                 /* st_tracklet_gsi: rows of the longest track of the range */
  const double* rows;
  const int* row_out_off;
  const int* row_gap;
  const int* trk_out_off;
  const int* trk_order;
  const double* trk_len_scale;
  void* ws;
  size_t ws_bytes;
  double* out_rows;
  int* status;
  long long* phase_ticks;       /* st_tracklet_gsi, optional (NULL: off): (num_groups, 4) counters the caller zeroed; every
                                   workgroup adds the ticks of the 100 MHz wall clock it spent building K, factorising,
                                   in the two solves and in the product (tools/tracklet_post_bench.py) */
} StTrackletArgs;
int st_tracklet_max_rows(void);
size_t st_tracklet_gsi_workspace_bytes(const StTrackletArgs* args);
int st_tracklet_interpolate(const StTrackletArgs* args, st_stream_t stream);
int st_tracklet_gsi(const StTrackletArgs* args, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 18. AppearanceFreeLink (AFLink, StrongSORT) on the device, csrc/aflink.hip.  Replaces the double loop of the
 *     reference's mmtrack/models/task_modules/track/aflink.py:230-259 (gate, data_transform and one batch-1 forward
 *     of the link network per pair); the rules are the statements of stereotracking_amd/aflink.py (backend='host',
 *     DESIGN.md section 18).  The linear assignment and the relabelling stay on the host.
 *   tables   built by the host: feat (num_rows, 3) fp64 = (frame, c0, c1) of every row, the tracks of all prediction
 *            sets one after the other, a set's tracks by (first frame, id), a track's rows ascending in frame;
 *            trk_off (num_tracks + 1) first row of every track; trk_set (num_tracks) the set of every track; set_off
 *            (num_sets + 1) first track of every set.  An entry that points outside the buffers sets header bit 2.
 *   header   2 ints, zeroed by st_aflink_gate: [0] the number of candidates, [1] status bits: 1 more candidates than
 *            `capacity` (the list holds the first `capacity`), 2 a table entry out of range.
 *   st_aflink_gate       every ordered pair i != j of a set with t_lo <= first_frame(j) - last_frame(i) <= t_hi and
 *            sqrt(dx * dx + dy * dy) <= spatial_thr (unfused fp64, the corners of i's last and j's first row) is a
 *            candidate.  A counting pass, an exclusive prefix sum (ws_off, num_tracks + 1 ints) and a filling pass:
 *            cand (capacity, 3) ints = (set, i, j) with i, j counted inside the set, row-major, no atomics.
 *   st_aflink_transform  candidates [first, first + count) (those at or past header[0] are skipped) -> ws_x
 *            (count, 2, 30, 3) fp32: i's last 30 rows (zero rows in front), j's first 30 (zero rows behind), every
 *            column (v - (max + min) / 2) / ((max - min) / 2 + 1e-5) over all 60 rows in fp64, rounded once.
 *   st_aflink_score      ws_x -> conf[first ...]: the softmax probability of class 1; logits (optional, NULL: off)
 *            (capacity, 2) the two fp32 logits.  One workgroup per st_aflink_group_pairs() candidates, activations in
 *            LDS, layers 2-4 and the fusion conv on v_mfma_f32_32x32x2_f32 (exact fp32).  A candidate's bytes do not
 *            depend on its neighbours, the range or the launch.
 *   st_aflink_run        gate, then transform + score over [0, capacity) in rounds of `chunk` candidates (ws_x holds
 *            chunk x 180 floats).  capacity: any upper bound of the candidate count the host knows (aflink.py takes
 *            the pairs that pass the temporal rule), at most st_aflink_max_candidates().
 *   weights  st_aflink_weights_create copies st_aflink_packed_floats() floats (BatchNorm folded to scale and shift by
 *            the host; the layout is written out at the top of csrc/aflink.hip and in aflink.pack_weights) to the
 *            device; the library owns that copy until st_aflink_weights_destroy.  These two calls allocate and wait;
 *            the stage calls are enqueued on `stream`, no host wait, no allocation.  All other buffers are the
 *            caller's.  A call that returns non-zero has written nothing.
 * ---------------------------------------------------------------------- */
typedef struct StAflinkArgs {
  int struct_size;              /* sizeof(StAflinkArgs) */
  int num_sets, num_tracks, num_rows;
  int capacity;                 /* slots of cand / conf / logits */
  int first, count;             /* st_aflink_transform, st_aflink_score: the candidate range of this call */
  int chunk;                    /* st_aflink_run: candidates per round */
  double t_lo, t_hi, spatial_thr;
  const double* feat;
  const int* trk_off;
  const int* trk_set;
  const int* set_off;
  int* ws_off;
  float* ws_x;
  int* header;
  int* cand;
  float* conf;
  float* logits;
} StAflinkArgs;
int st_aflink_group_pairs(void);
size_t st_aflink_packed_floats(void);
int st_aflink_max_candidates(void);
int st_aflink_weights_create(const float* packed_host, size_t num_floats, void** handle);
int st_aflink_weights_destroy(void* handle);
int st_aflink_gate(const StAflinkArgs* args, st_stream_t stream);
int st_aflink_transform(const StAflinkArgs* args, st_stream_t stream);
int st_aflink_score(const StAflinkArgs* args, const void* weights, st_stream_t stream);
int st_aflink_run(const StAflinkArgs* args, const void* weights, st_stream_t stream);

/* ------------------------------------------------------------------------
 * 19. ECC camera-motion compensation (tracker option cmc=dict(method='ecc'); the reference's CameraMotionCompensation =
 *     cv2.findTransformECC), csrc/cmc_ecc.hip.  The rules E0..E10 are restated from OpenCV 4.x ecc.cpp
 *     [upstream-memory], listed in tests/ecc_ref.py and DESIGN.md "ECC camera-motion compensation"; parity with cv2 is
 *     unpinned.  The warps feed the tracker routines of section 10 (st_tracker_track_cmc, ..._records_cmc) unchanged.
 *   plane    fp32 (plane_h, plane_w) = (img_h / downscale, img_w / downscale), st_cmc_ecc_plane_size.
 *   front    frames -> planes (crop to (h, w), fixed-point grey of the BGR frame, downscale x downscale box mean),
 *            from N separate uint8 (3, fh, fw) device frames (host array of device pointers) or a padded fp32
 *            (N, 3, H, W) batch; both give the same bits.
 *   prepare  planes -> blurred template, blurred input and its two gradients, each (N, plane_h, plane_w) fp32 (any
 *            output may be null).  Test-facing.
 *   step     ONE iteration from the given plane warps (N, 6) float64 {m00, m01, m02, m10, m11, m12} (null: identity)
 *            -> (N, ST_ECC_STEP_DOUBLES) float64 at the ST_ECC_STEP_* offsets (H as 6 x 6 row-major, its top-left
 *            K x K used; the warp in PLANE coordinates; fields behind a failure stay 0).  Test-facing, the same
 *            launches as the estimate.
 *   estimate plane pairs (prev[n] = template, curr[n] = input) -> warps (N, ST_CMC_WARP_FLOATS) = {valid, rho, 2 x 3
 *            warp in IMAGE coordinates} (a failed estimate: {0, 0, identity}) and, optionally, the iterations run
 *            (N,) int32.  All num_iters rounds are enqueued on `stream`; no host sync.  Bit-identical from run to run,
 *            and a pair's row does not depend on N.
 *   ws: caller-owned device workspace of st_cmc_ecc_workspace_bytes(N, plane_h, plane_w), 16-byte aligned
 *            (ST_ERR_INVALID otherwise).
 *   Every call refuses, before any launch (ST_ERR_INVALID, nothing written): a struct_size mismatch, a null pointer,
 *   a short workspace, a warp_mode / downscale / gauss_filt_size outside its set, num_iters < 1, a plane side under 8
 *   (and N outside 1..65535, a NaN stop_eps, num_iters > 1000 in the estimate: 2 launches are enqueued per round).
 * ---------------------------------------------------------------------- */
#define ST_ECC_TRANSLATION 0
#define ST_ECC_EUCLIDEAN 1
#define ST_ECC_AFFINE 2
#define ST_ECC_STEP_DOUBLES 72
#define ST_ECC_STEP_VALID 0
#define ST_ECC_STEP_N 1
#define ST_ECC_STEP_MEAN_I 2
#define ST_ECC_STEP_MEAN_T 3
#define ST_ECC_STEP_STD_I 4
#define ST_ECC_STEP_STD_T 5
#define ST_ECC_STEP_IMG_NORM 6
#define ST_ECC_STEP_TMP_NORM 7
#define ST_ECC_STEP_CORR 8
#define ST_ECC_STEP_RHO 9
#define ST_ECC_STEP_LAMBDA 10
#define ST_ECC_STEP_H 12      /* 36 */
#define ST_ECC_STEP_IP 48     /* 6 */
#define ST_ECC_STEP_TP 54     /* 6 */
#define ST_ECC_STEP_DP 60     /* 6 */
#define ST_ECC_STEP_WARP 66   /* 6: the updated warp (the input warp after a failure) */
typedef struct StEccParams {
  int struct_size;        /* sizeof(StEccParams) */
  int warp_mode;          /* ST_ECC_TRANSLATION / EUCLIDEAN / AFFINE (reference default EUCLIDEAN) */
  int num_iters;          /* >= 1 (default 50) */
  float stop_eps;         /* stop when |rho - last rho| < stop_eps (default 1e-3) */
  int gauss_filt_size;    /* 1, 3 or 5 (default 1) */
  int downscale;          /* 1, 2 or 4: plane = box mean of downscale x downscale grey pixels */
} StEccParams;
int st_cmc_ecc_plane_size(int img_h, int img_w, int downscale, int* plane_h, int* plane_w);
size_t st_cmc_ecc_workspace_bytes(int N, int plane_h, int plane_w);
int st_cmc_ecc_front_u8(const void* const* frames_u8_dev_ptrs_host, int N, int fh, int fw, int h, int w, int downscale,
                        float* planes_dev, st_stream_t stream);
int st_cmc_ecc_front_f32(const float* batch_dev, int N, int H, int W, int h, int w, int downscale, float* planes_dev,
                         st_stream_t stream);
int st_cmc_ecc_prepare(const float* prev_planes_dev, const float* curr_planes_dev, int N, int img_h, int img_w,
                       const StEccParams* params, void* ws, size_t ws_bytes, float* tmpl_out_dev, float* input_out_dev,
                       float* gx_out_dev, float* gy_out_dev, st_stream_t stream);
int st_cmc_ecc_step(const float* prev_planes_dev, const float* curr_planes_dev, int N, int img_h, int img_w,
                    const StEccParams* params, const double* warps_in_dev, void* ws, size_t ws_bytes,
                    double* step_out_dev, st_stream_t stream);
int st_cmc_ecc_estimate(const float* prev_planes_dev, const float* curr_planes_dev, int N, int img_h, int img_w,
                        const StEccParams* params, void* ws, size_t ws_bytes, float* warps_out_dev, int* iters_out_dev,
                        st_stream_t stream);

/* ----------------------------------------------------------------------
 * 20. Tracker-option sweeps on the batched GPU association (section 9): per-sequence tracker options, and a whole
 *    recorded detection stream in ONE launch (stereotracking_amd.sweep.TrackerSweep; csrc/batched_assoc.hip).
 *
 *  st_batched_tracker_create_multi: as st_batched_tracker_create, with cfgs[b] = the option set of sequence b
 *    (`batch` of them).  Whatever st_batched_tracker_create refuses is refused here for ANY member, before any device
 *    call, and st_last_error() names the member index.  State layout, scratch layout, state_bytes, scratch_bytes and
 *    get_states are those of section 9.  The option sets are copied; their device copy is owned by the tracker object
 *    (made by its first launch, freed by st_batched_tracker_destroy).  st_batched_tracker_step on such a tracker
 *    applies member b's options to sequence b.
 *
 *  st_batched_tracker_run: frames [f_begin, f_end) of V recorded videos for every sequence of the tracker (from either
 *    create function), ONE launch, one wave per sequence: sequence b walks the frames of video video_of[b] and writes
 *    every frame's rows, ids and count.
 *      frame_ids (V, F), dets (V, F, max_dets, 8), counts (V, F): the inputs of st_batched_tracker_step per video and
 *      frame; counts == -1 is a frame the video does not have (ragged lengths, gaps): out_counts = -1, the state does
 *      not move.  video_of (batch) in [0, V): sequences that share a video read the same rows, nothing is copied.
 *      out_rows (batch, F, max_dets, 8), out_ids (batch, F, max_dets), out_counts (batch, F): frames outside the range
 *      are not written.  status (batch): written as st_batched_tracker_step writes it (a code only, never 0).
 *    DEFINED as equal, on the bits, to f_end - f_begin calls of st_batched_tracker_step whose inputs were gathered
 *    through video_of - outputs, device state and status.  A capacity overflow is sticky exactly as there: the frame
 *    and all later ones get count 0 and report the code, until a frame with frame_id 0.  The state persists in
 *    state_dev between calls, so [0, F) in one call equals [0, k) then [k, F); that also bounds a launch.
 *    One code of its own: status 3 = video_of[b] outside [0, V) (that sequence reads nothing, counts 0).
 *    Refused before any launch: null pointers (video_of included), V or F <= 0, a range that is not
 *    0 <= f_begin < f_end <= F.  Enqueued on `stream`, no host sync.
 * ---------------------------------------------------------------------- */
int st_batched_tracker_create_multi(const StTrackerConfig* cfgs, int batch, int max_tracks, int max_dets,
                                    StBatchedTracker** out);
int st_batched_tracker_run(StBatchedTracker* t, const int32_t* frame_ids_dev, const float* dets_dev,
                           const int32_t* counts_dev, const int32_t* video_of_dev, int V, int F, int f_begin, int f_end,
                           void* state_dev, void* scratch_dev, float* out_rows_dev, int64_t* out_ids_dev,
                           int32_t* out_counts_dev, int32_t* status_dev, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 21. The MOTChallenge protocol of MOTDroneMetrics(protocol='trackeval') on the device, csrc/mot_eval.hip.  The rules
 *     are the statements of stereotracking_amd/metrics.py motchallenge_file_rows and motchallenge_preprocess (DESIGN.md
 *     section 21): the values a reader of the written text files gets, then TrackEval's MotChallenge2DBox preprocessing.
 *     fp64 and integers throughout, no atomics on the outputs: two runs give the same bytes.
 *
 *  st_mot_file_round: elementwise over rows (num_rows, num_cols) fp64, out-of-place or in place (out_dev == rows_dev).
 *    col_modes (num_cols <= ST_MOT_FILE_MAX_COLS ints, HOST memory): ST_MOT_FILE_COPY the value as it is;
 *    ST_MOT_FILE_TRUNCATE int(v), toward zero (the '%d' columns); ST_MOT_FILE_ROUND3 float('%.3f' % v): the exact
 *    binary value to 3 decimals, ties to even, then the nearest double to that decimal - from the exact residual of
 *    v * 1000 (one fused multiply-add), never from rint(v * 1000) alone.
 *    status: 8 ints on the device, zeroed by the call.  [0] bits: 1 a non-finite value in a TRUNCATE / ROUND3 column,
 *    2 |v| >= 2^43 in a ROUND3 column (v * 1000 must stay below 2^53).  [1 + k] for bit 1 << k: num_rows - the row
 *    index of the first offender.  An offending cell is copied unchanged.  Enqueued on `stream`, no host wait.
 *
 *  st_mot_challenge_preprocess: per frame with ground truth and predictions, one assignment on the IoU of the xywh
 *    boxes with entries < 0.5 - eps zeroed; a prediction matched (weight > eps) to ground truth of a distractor class
 *    is removed; ground truth is kept iff conf != 0 and class == 1.  do_preproc == 0 (MOT15): no matching, every
 *    prediction kept, ground truth kept iff conf != 0.
 *   rows     all sequences packed, sorted by sequence and frame.  gt_rows (num_gt, 8) fp64 = (frame, id, x, y, w, h,
 *            conf, class); pred_rows (num_pred, 7) = (frame, id, x, y, w, h, score).  Only the boxes, conf and class are read.
 *   tables   built by the host (stereotracking_amd/mot_eval.py) and TRUSTED: frame_gt_off / frame_pred_off
 *            (num_frames + 1) first row of every frame; frame_ws_off (num_frames + 1, 64-bit) first cell of the frame's
 *            slot in ws: a frame of more than 64 x 64 cells needs a slot of G x P cells, any other may have an empty
 *            one (solved out of LDS); num_ws_cells = frame_ws_off[num_frames].  distractors: num_distractors <=
 *            ST_MOT_CHALLENGE_MAX_DISTRACTORS class ids.
 *   limits   at most ST_MOT_MAX_OBJECTS rows of either kind in one frame.
 *   status   8 ints, 0 = fine, zeroed by the call, the bits of section 16: 1 non-finite box, 8 a frame above the limit,
 *            32 a frame whose ws slot is too small.  [1 + k] for bit 1 << k: num_frames - the frame index of the first
 *            offender.  The frames that set a bit write nothing.
 *   outputs  gt_keep (num_gt) / pred_keep (num_pred) bytes, 1 = the row is scored.  Both are zeroed by the call.
 *   One stage, enqueued on `stream`, one kernel launch (one wave per frame), no host wait.
 *   ws: caller-owned, st_mot_challenge_workspace_bytes(args) (0: invalid sizes).
 * ---------------------------------------------------------------------- */
#define ST_MOT_FILE_COPY 0
#define ST_MOT_FILE_TRUNCATE 1
#define ST_MOT_FILE_ROUND3 2
#define ST_MOT_FILE_MAX_COLS 16
#define ST_MOT_CHALLENGE_MAX_DISTRACTORS 8
typedef struct StMotChallengeArgs {
  int struct_size;              /* sizeof(StMotChallengeArgs) */
  int num_frames, num_gt, num_pred;
  int max_frame_objects;        /* largest number of gt or prediction rows in one frame; 0: unknown */
  int do_preproc;               /* 0: MOT15 */
  int num_distractors;
  int distractors[ST_MOT_CHALLENGE_MAX_DISTRACTORS];
  long long num_ws_cells;       /* frame_ws_off[num_frames] */
  const double* gt_rows;
  const double* pred_rows;
  const int* frame_gt_off;
  const int* frame_pred_off;
  const long long* frame_ws_off;
  void* ws;
  size_t ws_bytes;
  unsigned char* gt_keep;
  unsigned char* pred_keep;
  int* status;
} StMotChallengeArgs;
int st_mot_file_round(const double* rows_dev, double* out_dev, long long num_rows, int num_cols, const int* col_modes,
                      int* status_dev, st_stream_t stream);
size_t st_mot_challenge_workspace_bytes(const StMotChallengeArgs* args);
int st_mot_challenge_preprocess(const StMotChallengeArgs* args, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 22. Dense stereo evaluation (stereo_eval.stereo_error_stats, StereoMetric, OCSORT_Disparity(stereo_eval=...)),
 *     csrc/stereo_eval.hip.  NEW, no reference function: the definitions below are the specification, their executable
 *     form is tests/stereo_eval_ref.py (numpy float32 / float64, operation by operation).
 *   inputs   pred: plane 0 of an (N, C, H, W) fp32 disparity map (pixels), image n at pred_dev + n * pred_img_pitch
 *            floats, rows of W floats; gt: plane 0 of an (N, Cg, H, W) fp32 map, gt_img_pitch likewise, metres
 *            (ST_STEREO_GT_DEPTH) or pixels (ST_STEREO_GT_DISP).  extent (N, 2) int32 = (h_n, w_n), clamped to (H, W):
 *            rows >= h_n and columns >= w_n are padding and are NOT read, nor is any other plane.  boxes
 *            (N, max_boxes, 4) fp32 xyxy and box_counts (N,) int32 (clamped to 0..max_boxes; rows at or beyond the count
 *            are not read); max_boxes == 0: no boxes, both pointers may be NULL.  bf = baseline * focal length.
 *   pixel    all fp32, unfused, IEEE division.  depth: gz = g, gd = bf / gz; disp: gd = g, gz = bf / gd.
 *            gt-valid: g finite, g > 0, depth_edges[0] < gz <= depth_edges[K]; depth bin b: depth_edges[b] < gz <=
 *            depth_edges[b + 1].  pred-valid: p finite, p > 0; pz = bf / p.  region 1 iff a counted box row has
 *            x1 <= (float)x < x2 and y1 <= (float)y < y2, else 0.  On pixels valid both ways: e = |p - gd|;
 *            bad_t: e > bad_thresholds[t]; d1: e > 3 && e > 0.05f * gd; r = max(pz / gz, gz / pz), delta_k: r < 1.25^k
 *            (k = 1, 2, 3); histogram bin e * 16 >= 511 ? 511 : (int)(e * 16); fp64 dz = (double)pz - (double)gz.
 *   outputs  per cell (n, region, bin), region-major: counts (N, 2, K, T + 6) int64 = n_gt, n_both, n_bad[T], n_d1,
 *            n_delta[3]; sums (N, 2, K, 5) fp64 = sum e, e^2, |dz| / gz, dz^2 / gz, dz^2 (every term formed in double
 *            from the fp32 values); hist (N, 2, K, 512) int64.  Every cell is defined by the call, whatever the buffers
 *            and the workspace held.  Integers are exact; the fp64 sums use NO floating-point atomics (fixed pixel range
 *            per workgroup, fixed reduction tree, one partial per cell in the workspace, a second launch adds the
 *            partials in index order): two calls on the same inputs return the same bytes.
 *   workspace  caller-owned device memory, 8-byte aligned, st_stereo_eval_workspace_bytes(args) bytes (0: invalid
 *            arguments), its size in args->workspace_bytes.  Enqueued on `stream` (one memset of hist, two launches), no
 *            host wait, no allocation.  A call that returns non-zero has launched nothing.
 * ---------------------------------------------------------------------- */
#define ST_STEREO_EVAL_MAX_BINS 8
#define ST_STEREO_EVAL_MAX_THRESHOLDS 6
#define ST_STEREO_EVAL_HIST_BINS 512
#define ST_STEREO_EVAL_NUM_SUMS 5
#define ST_STEREO_EVAL_MAX_BOXES 256
#define ST_STEREO_GT_DEPTH 0
#define ST_STEREO_GT_DISP 1
typedef struct StStereoEvalArgs {
  int struct_size;              /* sizeof(StStereoEvalArgs) */
  int N, H, W;
  int gt_kind;                  /* ST_STEREO_GT_DEPTH / ST_STEREO_GT_DISP */
  int num_bins;                 /* K, 1 .. ST_STEREO_EVAL_MAX_BINS */
  int num_thresholds;           /* T, 1 .. ST_STEREO_EVAL_MAX_THRESHOLDS */
  int max_boxes;                /* M, 0 .. ST_STEREO_EVAL_MAX_BOXES */
  size_t pred_img_pitch;        /* floats between images of pred (>= H * W) */
  size_t gt_img_pitch;          /* floats between images of gt */
  size_t workspace_bytes;
  float bf;
  float depth_edges[ST_STEREO_EVAL_MAX_BINS + 1];     /* K + 1 used, strictly ascending */
  float bad_thresholds[ST_STEREO_EVAL_MAX_THRESHOLDS]; /* T used */
} StStereoEvalArgs;
size_t st_stereo_eval_workspace_bytes(const StStereoEvalArgs* args);
int st_stereo_eval(const StStereoEvalArgs* args, const float* pred_dev, const float* gt_dev, const int32_t* extent_dev,
                   const float* boxes_dev, const int32_t* box_counts_dev, int64_t* counts_dev, double* sums_dev,
                   int64_t* hist_dev, void* workspace_dev, st_stream_t stream);

/* ----------------------------------------------------------------------
 * 23. Disparity-completion head (DispHeadV2) on the device, csrc/disp_head.hip.  Replaces the forward of the
 *     reference's mmtrack/models/dense_head/disp_head_v2.py:129-176 (input_transform=None, out_channels=1; CBAM(64, 4,
 *     no_spatial=True) :126, :264-300) and the rescale of base_disp_head.py:131-139:
 *
 *       x = ELU(BN(conv3x3 in_channels -> C))   dconv1_1        x: the stride-8 neck level (detector tap "p3")
 *       x = ELU(BN(conv3x3 C -> C))             dconv1_2
 *       x = nearest x2(x)
 *       g = df * (1 - sigmoid(mlp(avg(df)) + mlp(max(df))))     df: detector tap "stage1_disp" (64 channels, stride 4);
 *                                                               avg / max per image and channel over H x W,
 *                                                               mlp = Linear(64, 16), ReLU, Linear(16, 64)
 *       x = ELU(BN(conv3x3 C + 64 -> 256))      dconv2_1        on cat(x, g)
 *       x = ELU(BN(conv3x3 256 -> 256))         dconv2_2
 *       x = nearest x2(x)
 *       x = ELU(BN(conv3x3 256 -> 128))         dconv3_1
 *       y = ReLU(conv1x1 128 -> 1 + bias)       reg             -> pred [N][1][4 p3_height][4 p3_width]
 *
 *     ELU alpha 1.  The 3x3 convolutions run on the conv primitive of section 1 (act = 0; the Winograd instance where
 *     the layer qualifies, else the implicit GEMM at the library's tile choice - a function of the shapes alone).  The
 *     rest are bandwidth kernels: ELU in place (dconv1_1, dconv2_1); ELU + nearest x2 stored into the concat slice /
 *     the input of dconv3_1 (no ELU-ed low-resolution copy); the channel gate (sum and max with a fixed reduction
 *     order and no float atomics, MLP + sigmoid, apply into channels [C, C + 64) of the concat); ELU + reg + bias +
 *     ReLU in one pass over the RAW dconv3_1 output (its ELU-ed form is never written).  Two runs are bit-equal and an
 *     image's result does not depend on the batch around it.
 *     Parameters are named like the reference state_dict below the head: dconv1_1.conv.weight, dconv1_1.bn.weight /
 *     .bias / .running_mean / .running_var, ... dconv3_1.*, reg.conv.weight [1][128][1][1], reg.conv.bias [1],
 *     cbam.ChannelGate.mlp.1.weight [16][64], .mlp.1.bias, .mlp.3.weight [64][16], .mlp.3.bias.
 *     st_disp_head_finalize folds BN in fp64, packs (Winograd form included) and uploads; needs a current device.
 * ---------------------------------------------------------------------- */
typedef struct StDispHead StDispHead;
typedef struct StDispHeadConfig {
  int struct_size;          /* = sizeof(StDispHeadConfig) */
  int batch;
  int p3_height, p3_width;  /* size of the stride-8 map: padded input / 8 */
  int in_channels;          /* channels of the stride-8 level, a multiple of 4 (128 for YOLOX-s) */
  int channels;             /* C, a multiple of 32 (at most 1024) */
  double bn_eps;            /* 1e-3 */
} StDispHeadConfig;
int st_disp_head_create(const StDispHeadConfig* cfg, StDispHead** out);
int st_disp_head_destroy(StDispHead* head);
int st_disp_head_num_params(const StDispHead* head);
int st_disp_head_param_info(const StDispHead* head, int idx, char* name, int name_cap, int64_t shape[4], int* ndim);
int st_disp_head_set_param(StDispHead* head, const char* name, const float* host, int64_t numel);
int st_disp_head_finalize(StDispHead* head);
size_t st_disp_head_workspace_bytes(const StDispHead* head);
/* p3 / df: NHWC views, pixel p, channel c at p3_dev[p * p3_ld + p3_off + c] (c < in_channels) and
 * df_dev[p * df_ld + df_off + c] (c < 64); strides and offsets multiples of 4, pointers 16-byte aligned.  Nothing
 * outside the two slices is read.  The prediction is written to the workspace (tap "pred") and, when pred_out_dev is
 * not NULL, to pred_out_dev [N][1][4 p3_height][4 p3_width] as well. */
int st_disp_head_forward(StDispHead* head, const float* p3_dev, int p3_ld, int p3_off, const float* df_dev, int df_ld,
                         int df_off, void* workspace_dev, size_t workspace_bytes, st_stream_t stream, float* pred_out_dev);
/* Internal activations inside the workspace (valid after forward), NHWC, pixel p channel c at ptr[p * ld + c]:
 * "dconv1_2" (RAW: conv + BN, before the ELU), "gate_scale" ([N][64], the sigmoid s), "cat" ([N][2h][2w][C + 64]),
 * "dconv2_2" (raw), "dconv3_1_raw", "pred" ([N][4h][4w][1]). */
int st_disp_head_tap(const StDispHead* head, const char* name, const void* workspace_dev, const float** ptr_dev, int* N,
                     int* C, int* H, int* W, int* ld);
/* The rescale of predict(rescale=True): N maps [h][w] -> [H][W], bilinear with torch's align_corners=False rule (source
 * index (dst + 0.5) * in / out - 0.5, clamped at 0).  As in the reference the source is the map of the PADDED input,
 * resized straight to img_shape (base_disp_head.py:131-139 does not crop the padding first). */
int st_disp_head_resize(const float* pred_dev, int N, int h, int w, float* out_dev, int H, int W, st_stream_t stream);
/* Per-launch timing (tools/disp_head_bench.py): when enabled, the st_disp_head_num_launches() launches of the following
 * forwards (the five convolutions and the kernels between them, st_disp_head_launch_name) are bracketed by hipEvents on
 * the caller's stream; st_disp_head_launch_times synchronises on them and returns the elapsed ms per launch. */
int st_disp_head_set_timing(StDispHead* head, int enable);
int st_disp_head_num_launches(void);
const char* st_disp_head_launch_name(int i);
int st_disp_head_launch_times(StDispHead* head, int cap, float* ms);
/* The map the per-box depth stage reads when it takes its depths from the head (pipeline depth_source): ONE launch, at
 * the PADDED input size, aligned with disp_postp pixel for pixel (image in the top-left corner) - not the squeezed
 * predict(rescale=True) map above.
 *   up2  = dense [N][1][H/2][W/2] (the head's prediction) resized to [H][W] by exactly the arithmetic of
 *          st_disp_head_resize (same operation order, contraction off): mode 1 is bit-equal to that call;
 *   mode 1 (completed): out = up2;
 *   mode 2 (fused):     out = disp > 0 ? disp : up2 per pixel, disp = plane 0 of frame n at disp_dev + n *
 *          disp_frame_stride.  `disp > 0` is false for 0, -0.0, negatives and NaN (the head's value is taken), +Inf is
 *          kept.  Planes 1.. of disp are never read; in mode 1 disp is not read at all.
 *   filled_dev [N] (may be NULL): pixels of frame n inside [0, ext_h) x [0, ext_w) whose value came from the head (all of
 *          them in mode 1).  Zeroed on the stream by this call, then integer atomics: independent of the order.
 * Refused (non-zero, nothing written or enqueued): null dense / disp / out, N <= 0, H or W odd or not positive, ext_h
 * outside [1, H], ext_w outside [1, W], mode not 1 or 2, disp_frame_stride < H * W, H * W >= 2^31. */
int st_disp_fuse(const float* dense_dev, const float* disp_dev, size_t disp_frame_stride, int N, int H, int W, int ext_h,
                 int ext_w, int mode, float* out_dev, int32_t* filled_dev, st_stream_t stream);

/* ----------------------------------------------------------------------
 * Dataset reader helper (host, no GPU): reverse the PNG scanline filters (RFC 2083 6: None/Sub/Up/Average/Paeth).
 * Replaces the OpenCV PNG decode behind mmcv.imfrombytes(..., flag='unchanged') that the reference's loaders call
 * (mmtrack/datasets/transforms/loading_disparity.py:74-75 uint16 disparity, :213-215 uint16 depth; mmcv's
 * LoadImageFromFile for the uint8 left / right images).  Container parsing and inflate stay in the host language
 * (Python zlib, stereotracking_amd/datasets.py).
 *   filtered: height rows of (1 filter-type byte + stride data bytes), as inflate yields them;
 *   bpp: bytes per complete pixel (1 gray8, 2 gray16, 3 rgb8, 4 rgba8, 6 rgb16, 8 rgba16); out: height x stride.
 * ---------------------------------------------------------------------- */
int st_png_unfilter(const uint8_t* filtered, int height, int stride, int bpp, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* STEREOTRACK_H_ */
