/*
 * rewriting_hip.h -- C ABI of librewriting_hip.so, the MI355X (gfx950) kernels behind the
 * rule-editing hot path of davidbau/rewriting.
 *
 * Boundary contract (level B3):
 *   - every pointer is a DEVICE pointer to contiguous float32 unless stated otherwise;
 *   - the CALLER owns and allocates every buffer (the Python host passes
 *     torch.Tensor.data_ptr()); the library allocates nothing and keeps no global state;
 *   - every entry point enqueues on the stream it is given (a hipStream_t passed as void*,
 *     NULL = the default stream) and returns immediately: stream-ordered and re-entrant;
 *   - return value 0 = success, otherwise a hipError_t (or RW_ERR_* below); the host
 *     wrapper raises RuntimeError(rw_error_string(code)) -- the reference's ops surface
 *     failures as RuntimeError through TORCH_CHECK
 *     (utils/stylegan2/op/fused_bias_act.cpp:6-8, upfirdn2d.cpp:8-10);
 *   - "nullable" pointers may be NULL, mirroring the reference's "empty tensor means
 *     absent" convention (utils/stylegan2/op/fused_bias_act_kernel.cu:62-63).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef REWRITING_HIP_H
#define REWRITING_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rw_stream_t; /* hipStream_t */

#define RW_ERR_BAD_ARGUMENT 10001
#define RW_ERR_UNSUPPORTED  10002

/* 10: the _f64 forward entries (rw_pixel_norm_f64 ... rw_conv_transpose3x3s2_f64, the last section of this header): a
 * library without them is refused by the loader as stale, not at the first missing symbol.  9: rw_dconv3x3_rgb_partial_f32 /
 * rw_rgb_combine_f32; 8: rw_tconv_blur_*.  7 since round 5: the split-operand ("H16") entry points take their bounds as
 * RW_BOUND_LANES-float vectors written
 * by plain stores (no memset, no atomic, no device scalar that one launch raises and the next reads) and their weight
 * scale BY VALUE (rw_split_weight_scale); rw_publish_scalar_f32 is gone.  (3: rw_solve_run_*, the whole-image 8x8 / 4x4
 * shapes, the point order of the packed F(4x4,3x3) weights; 4: rw_*_wino4h_*; 5: rw_dconv*; 6: rw_publish_scalar_f32.)
 * Buffers packed by an older library do not fit this one: repack, as the Python side does per weight version.
 * rw_resize_bilinear_u8 joins at 11, as rw_render_bytes_f32 and rw_png_* did: an entry that is only ADDED changes no
 * existing call, and the loader names the missing symbol of a library built before it ("stale ... no symbol").  So do
 * rw_rgb_combine_up_f32 and rw_conv3x3_wino4[h]_to_rgb_up_f32 (the ToRGB skip upsampled inside its consumer), and
 * rw_png_inflate_u8 / rw_png_unfilter_u8 (PNG decoding). */
int rw_abi_version(void);
const char* rw_error_string(int code);

/* ---------------------------------------------------------------------------------------
 * L1 native ops -- replace the two pybind entry points of utils/stylegan2/op/
 *
 * Three dtypes here, fp32 everywhere else.  These three ops -- fused_bias_act, bias_grad, upfirdn2d -- take float
 * (_f32), double (_f64) and half (_f16) buffers, as the reference's modules dispatch float, double and half
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF, fused_bias_act_kernel.cu:79, upfirdn2d_kernel.cu:225).  Each dtype form takes
 * the same arguments as its _f32 twin, and every operand (bias, refer, filter taps) comes in the dtype
 * of the input (the reference reads them through data_ptr<scalar_t>()).  Half buffers are uint16_t* holding IEEE
 * binary16.
 *   - _f64: the fp32 kernel's arithmetic in double; alpha and scale are passed as double.
 *   - _f16: each value is widened to float on load, goes through exactly the fp32 kernel's arithmetic in the same
 *     order, and is rounded to half ONCE, at the store: an _f16 result equals the _f32 entry run on the widened inputs,
 *     then rounded (round to nearest even).  bias_grad sums in float, as torch.sum does for half.  This differs from
 *     the reference's half path, which rounds after every operation and rounds alpha and scale to half.
 * The generator's forward has a float64 form as well: the _f64 entries of the last section of this header (pixel norm,
 * equalised linear, latent adjustment, style multiply, demodulation factors, the two 3x3 convolutions, noise, ToRGB)
 * take `double` buffers and `double` scalars and compute and accumulate in double, so that a model cast with .double()
 * runs its whole forward on the device, module by module.  That form is forward only: no fused epilogues, no packed
 * weights, no gradients, no solver.
 * Every other entry of this library is fp32 ONLY: it takes `float` pointers -- the path it accelerates runs in fp32 end
 * to end (BASELINE.json: "images within 1e-3 L-inf fp32").  A .half() model does not reach those entries, and neither
 * does a double tensor handed to an fp32 wrapper: the Python wrappers (rewriting_amd/hip.py) refuse any other dtype with
 * an error that names this limit (the status of the refusal is RW_ERR_UNSUPPORTED: nothing was launched), they never
 * convert silently.  The ctypes stub of INTEGRATION.md dispatches on the input's dtype to the three forms above and
 * refuses any other dtype, or an operand of another dtype, before anything is launched.
 * ------------------------------------------------------------------------------------- */

/* fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 *   pybind: utils/stylegan2/op/fused_bias_act.cpp:11-20
 *   kernel: utils/stylegan2/op/fused_bias_act_kernel.cu:18-49 (host wrapper :52-98)
 * y[i] = act'(x[i] + b[(i / step_b) % size_b]) * scale, act*10+grad in {10,11,12,30,31,32}.
 * b nullable (no bias), ref nullable (required for grad=1 of act=3). */
int rw_fused_bias_act_f32(const float* x, const float* b, const float* ref, float* y,
                          int64_t n, int64_t step_b, int64_t size_b,
                          int act, int grad, float alpha, float scale, rw_stream_t stream);
int rw_fused_bias_act_f16(const uint16_t* x, const uint16_t* b, const uint16_t* ref, uint16_t* y,
                          int64_t n, int64_t step_b, int64_t size_b,
                          int act, int grad, float alpha, float scale, rw_stream_t stream);
int rw_fused_bias_act_f64(const double* x, const double* b, const double* ref, double* y,
                          int64_t n, int64_t step_b, int64_t size_b,
                          int act, int grad, double alpha, double scale, rw_stream_t stream);

/* grad_bias = grad_input.sum(all dims but 1)   (utils/stylegan2/op/fused_act.py:32-39)
 * g viewed as (outer, channels, inner); gb[c] = sum_{o,i} g[o][c][i]. */
int rw_bias_grad_f32(const float* g, float* gb, int64_t outer, int64_t channels, int64_t inner,
                     rw_stream_t stream);
int rw_bias_grad_f16(const uint16_t* g, uint16_t* gb, int64_t outer, int64_t channels, int64_t inner,
                     rw_stream_t stream);
int rw_bias_grad_f64(const double* g, double* gb, int64_t outer, int64_t channels, int64_t inner,
                     rw_stream_t stream);

/* upfirdn2d(input[major,H,W,minor], kernel[kh,kw], up_x, up_y, down_x, down_y,
 *           pad_x0, pad_x1, pad_y0, pad_y1) -> out[major,out_h,out_w,minor]
 *   pybind: utils/stylegan2/op/upfirdn2d.cpp:12-22
 *   kernel: utils/stylegan2/op/upfirdn2d_kernel.cu:52-137 (host wrapper :140-271)
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh + down_y) / down_y  (:167-168); the caller
 * allocates y with that shape.  Any up/down/pad/kernel size (the reference compiles only
 * six modes, :178-210). */
int rw_upfirdn2d_f32(const float* x, const float* k, float* y,
                     int major, int in_h, int in_w, int minor, int kh, int kw,
                     int up_x, int up_y, int down_x, int down_y,
                     int pad_x0, int pad_x1, int pad_y0, int pad_y1, rw_stream_t stream);
int rw_upfirdn2d_f16(const uint16_t* x, const uint16_t* k, uint16_t* y,
                     int major, int in_h, int in_w, int minor, int kh, int kw,
                     int up_x, int up_y, int down_x, int down_y,
                     int pad_x0, int pad_x1, int pad_y0, int pad_y1, rw_stream_t stream);
int rw_upfirdn2d_f64(const double* x, const double* k, double* y,
                     int major, int in_h, int in_w, int minor, int kh, int kw,
                     int up_x, int up_y, int down_x, int down_y,
                     int pad_x0, int pad_x1, int pad_y0, int pad_y1, rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Generator forward -- replaces the torch expressions of utils/stylegan2/models.py
 * ------------------------------------------------------------------------------------- */

/* PixelNormL: y = x * rsqrt(mean(x^2, dim=1) + eps)      (models.py:609-614) */
int rw_pixel_norm_f32(const float* x, float* y, int batch, int dim, float eps, rw_stream_t stream);

/* EqualLinear.forward (models.py:503-511): y[b][o] = sum_i x[b*x_stride + i] * (w[o][i]*w_scale)
 * + bias[o]*b_scale, then, if act != 0, fused lrelu(alpha) * act_scale
 * (op/fused_act.py:85-86).  x_stride lets the caller pass latent[:, index] un-copied
 * (PickLatent, models.py:585-595). */
int rw_equal_linear_f32(const float* x, const float* w, const float* bias, float* y,
                        int batch, int in_dim, int out_dim, int64_t x_stride,
                        float w_scale, float b_scale, int act, float alpha, float act_scale,
                        rw_stream_t stream);

/* AdjustLatent (models.py:570-583): out[b][l][:] = avg + psi*(w[b] - avg) for l < n_latent;
 * avg nullable (no truncation). */
int rw_adjust_latent_f32(const float* w, const float* avg, float* out, int batch, int n_latent,
                         int dim, float psi, rw_stream_t stream);

/* ApplyStyle (models.py:616-620): y[b][c][p] = style[b][c] * x[b][c][p].  This output is the
 * rewriter's KEY (rewrite/ganrewrite.py:662-665). */
int rw_style_mul_f32(const float* x, const float* style, float* y, int batch, int channels,
                     int64_t hw, rw_stream_t stream);

/* wsq[o][i] = sum_{ky,kx} (w_scale * W[o][i][ky][kx])^2   -- first half of the demodulation
 * factor of DemodulatedConv2dF.forward (models.py:320-328), cached per weight version. */
int rw_weight_sqsum_f32(const float* w, float* wsq, int out_ch, int in_ch, int taps, float w_scale,
                        rw_stream_t stream);

/* demod[b][o] = rsqrt(sum_i style[b][i]^2 * wsq[o][i] + eps)      (models.py:326-327) */
int rw_demod_f32(const float* wsq, const float* style, float* demod, int batch, int out_ch,
                 int in_ch, float eps, rw_stream_t stream);

/* Repack a conv weight W[o][i][3][3] for the implicit-GEMM kernels.  wp receives
 * rw_packed_conv_weight_elems(out_ch, in_ch, mode) floats: first 9*Cin*Cout in slab order
 *   mode 0 (stride-1 conv, models.py:318-319):       wp[tap][i][o] = W[o][i][tap]
 *   mode 1 (stride-2 transposed conv, models.py:315-316), grouped by output parity
 *          phase (py,px): wp = [phase(0,0): 4 taps][phase(0,1): 2][phase(1,0): 2][phase(1,1): 1],
 *          each tap a contiguous [i][o] slab,
 * then (when Cout % 32 == 0 and Cin % 16 == 0, the shapes the halo-tile kernels take) the same
 * values in MFMA A-fragment order, so that a wave fetches its operand with 16-byte loads of 1 KiB
 * of consecutive addresses (IC = 16 input channels per chunk; 8 for mode 0 with Cout % 64 != 0):
 *   mode 0: wf[tap][i / IC][o / 32][kp / 4][lane][kp % 4],   kp < IC/2
 *   mode 1: wf[i / 16][o / 32][kp]{[slab / 4][lane][slab % 4] for slab < 8, then [lane] for slab 8}
 *   with value W[32 (o/32) + (lane & 31)][IC (i/IC) + 2 kp + (lane >> 5)][tap].
 * The scale 1/sqrt(9*Cin) is NOT folded in. */
long long rw_packed_conv_weight_elems(int out_ch, int in_ch, int mode);
int rw_pack_conv_weight_f32(const float* w, float* wp, int out_ch, int in_ch, int mode,
                            rw_stream_t stream);

/* Epilogue description shared by the two conv entry points.  y = acc * w_scale, then
 *   if demod: y *= demod[b][o]                                   (models.py:328)
 *   if noise: y += noise_w[0] * noise[b][pixel]                  (NoiseInjectionF :539-546)
 *   if act:   y = lrelu(y + bias[o], 0.2) * sqrt(2)              (FusedLeakyReLUF :622-626)
 * noise/bias/act are only legal for the stride-1 conv (for up layers the blur sits between). */
typedef struct rw_conv_epilogue {
  const float* style;    /* nullable: multiply the input by style[b][i] while loading (ApplyStyle fused) */
  const float* demod;    /* nullable */
  const float* noise;    /* nullable, (batch, out_h*out_w) */
  const float* noise_w;  /* device scalar, required iff noise */
  const float* bias;     /* nullable, (out_ch) */
  int act;               /* 0 / 1 */
} rw_conv_epilogue;

/* F.conv2d(x, scale*W, padding=1) [* demod]           (DemodulatedConv2dF, models.py:318-329)
 * x (B,Cin,H,W) -> y (B,Cout,H,W), wp from rw_pack_conv_weight_f32 mode 0.
 * impl: 0 = auto (fp32 MFMA implicit GEMM, v_mfma_f32_32x32x2_f32: halo-tile kernel when the map
 * is >= 24 wide (or 5..16 wide: column tiles of 2 x 16 / 4 x 8 pixels), else the im2col kernel, which splits K across the four waves of a workgroup when
 * the launch would otherwise leave most CUs idle), 1 = direct VALU kernel (cross-check), 2 = force
 * the im2col MFMA kernel, 3 = force the halo-tile MFMA kernel (RW_ERR_UNSUPPORTED if not applicable),
 * 4 = (transposed conv only) per-phase halo tiles, 5 = im2col MFMA kernel without split-K,
 * 6 = im2col MFMA kernel with split-K forced; transposed conv only: 7 = the quad tiles of the halo
 * kernel without output row 2H / column 2W (RW_ERR_UNSUPPORTED where the halo kernel does not apply), 8 = that row
 * and column only (disjoint writes: the two may be issued on different streams) -- three GEMMs over the last input row /
 * column of all images, any map size, in_ch % 16 == 0 and out_ch % 32 == 0. */
int rw_conv3x3_f32(const float* x, const float* wp, float* y, int batch, int in_ch, int out_ch,
                   int h, int w, float w_scale, const rw_conv_epilogue* ep, int impl,
                   rw_stream_t stream);

/* ToRGB (ToRGBF.forward, models.py:639-655) fused into the epilogue of the styled convolution that feeds it:
 *   rgb[b][c] = sum_o (scale * weight[c][o] * style[b][o]) * out[b][o] + bias[c] + skip[b][c]
 * computed from the activated outputs while they are still in registers.  y may be NULL: the feature map is
 * then not stored at all (the last layer of the generator, which only ToRGB consumes).
 * RW_ERR_UNSUPPORTED unless out_ch is 32 or 64 (the tile shapes in which one wave holds all out-channels of
 * its pixels), w >= 24 and in_ch % 16 == 0; callers then run rw_conv3x3_f32 and rw_to_rgb_f32. */
typedef struct rw_rgb_epilogue {
  const float* weight;   /* (3, out_ch) ToRGB conv weight */
  const float* style;    /* (batch, out_ch) ToRGB modulation */
  const float* bias;     /* (3) nullable */
  const float* skip;     /* (batch, 3, h, w) nullable: the upsampled running image */
  float* out;            /* (batch, 3, h, w) */
  float scale;           /* 1/sqrt(out_ch) */
} rw_rgb_epilogue;
int rw_conv3x3_to_rgb_f32(const float* x, const float* wp, float* y, int batch, int in_ch, int out_ch,
                          int h, int w, float w_scale, const rw_conv_epilogue* ep,
                          const rw_rgb_epilogue* rgb, rw_stream_t stream);

/* OPT-IN split-precision stride-1 convolution ("bf16x6"): same operation and epilogue as rw_conv3x3_f32,
 * computed on the bf16 matrix pipe with every fp32 operand split exactly into three bf16 pieces and the
 * six leading piece products accumulated in fp32 (relative error of a product < 2^-22; no range loss).
 * wb from rw_pack_conv_weight_bf16x3 (rw_packed_conv_weight_bf16x3_bytes bytes).  RW_ERR_UNSUPPORTED
 * unless w >= 24, in_ch % 16 == 0 and out_ch % 64 == 0 -- callers then use rw_conv3x3_f32, which is
 * also the default everywhere: nothing selects this path implicitly. */
long long rw_packed_conv_weight_bf16x3_bytes(int out_ch, int in_ch);
int rw_pack_conv_weight_bf16x3(const float* w, void* wb, int out_ch, int in_ch, rw_stream_t stream);
int rw_conv3x3_bf16x6_f32(const float* x, const void* wb, float* y, int batch, int in_ch, int out_ch,
                          int h, int w, float w_scale, const rw_conv_epilogue* ep, rw_stream_t stream);

/* The same stride-1 convolution (and the same fused epilogues) by the Winograd minimal-filtering algorithm
 * F(2x2, 3x3) in fp32: 16 instead of 36 multiplications per 2x2 output tile and channel pair, i.e. 2.25x fewer
 * matrix FLOPs for a result that is identical in exact arithmetic and of the direct kernel's error class in
 * fp32 (transform coefficients 0, +-1, +-1/2; fp32 MFMA accumulation).  rw_conv3x3_wino_supported() says which
 * shapes it takes (out_ch % 32 == 0, in_ch % 8 == 0, and w % 32 == 0 with h % 8 == 0, w == 16 with h % 16 == 0, or the
 * whole 8 x 8 / 4 x 4 maps -- several images per workgroup; these take ep->style == NULL, i.e. an input that already
 * carries its style, RW_ERR_UNSUPPORTED otherwise); elsewhere, and whenever the caller prefers the direct sum,
 * rw_conv3x3_f32 is the kernel.
 *   uf: rw_packed_conv_weight_wino_elems(out_ch, in_ch) = 16*out_ch*in_ch floats from rw_pack_conv_weight_wino_f32:
 *       U = G g G^T of every (o, i) filter in the A-fragment order of v_mfma_f32_16x16x4_f32
 *       uf[o / 32][i / 4][xi / 4][(o % 32) / 16][lane][xi % 4],  o = 32 (o/32) + 16 ((o%32)/16) + (lane & 15),
 *       i = 4 (i/4) + (lane >> 4), xi = 4 a + b the transform point (row a, column b of G g G^T).
 * rw_conv3x3_wino_to_rgb_f32: ToRGB in the epilogue as rw_conv3x3_to_rgb_f32 (out_ch == 32 only). */
int rw_conv3x3_wino_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_conv_weight_wino_elems(int out_ch, int in_ch);
int rw_pack_conv_weight_wino_f32(const float* w, float* uf, int out_ch, int in_ch, rw_stream_t stream);
int rw_conv3x3_wino_f32(const float* x, const float* uf, float* y, int batch, int in_ch, int out_ch, int h,
                        int w, float w_scale, const rw_conv_epilogue* ep, rw_stream_t stream);
int rw_conv3x3_wino_to_rgb_f32(const float* x, const float* uf, float* y, int batch, int in_ch, int out_ch,
                               int h, int w, float w_scale, const rw_conv_epilogue* ep,
                               const rw_rgb_epilogue* rgb, rw_stream_t stream);

/* The same convolution by Winograd F(4x4, 3x3) in fp32: 36 multiplications per 4x4 output tile and channel pair
 * (4x fewer matrix FLOPs than the direct sum, 1.78x fewer than F(2x2,3x3)).  Its transforms carry the constants
 * 4, 5, 8, 1/24: measured fp32 error 4e-6 .. 9e-6 of the output range per layer against 2e-7 .. 6e-7 for the two
 * kernels above.  The Python host makes it the DEFAULT inside the un-hooked forward of the whole generator (image
 * generation: the image tolerance of the path is 1e-3 L-inf, the measured deviation from the reference image 3e-5)
 * and nowhere else: a hooked or sliced model -- the statistics sweeps, goal maps, the solve's context and its
 * rendering -- runs F(2x2,3x3), so the same weights run hooked and un-hooked differ by 1e-5 .. 1e-4 on the image.
 * Shapes: out_ch % 32 == 0, in_ch % 8 == 0, w % 64 == 0, h % 8 == 0.
 *   uf: rw_packed_conv_weight_wino4_elems(out_ch, in_ch) = 36*out_ch*in_ch floats from
 *       rw_pack_conv_weight_wino4_f32: uf[o / 16][i / 4][xi / 4][lane][xi % 4], o = 16 (o/16) + (lane & 15),
 *       i = 4 (i/4) + (lane >> 4), xi = 6 a + b the transform point (row a, column b of G g G^T). */
int rw_conv3x3_wino4_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_conv_weight_wino4_elems(int out_ch, int in_ch);
int rw_pack_conv_weight_wino4_f32(const float* w, float* uf, int out_ch, int in_ch, rw_stream_t stream);
int rw_conv3x3_wino4_f32(const float* x, const float* uf, float* y, int batch, int in_ch, int out_ch, int h,
                         int w, float w_scale, const rw_conv_epilogue* ep, rw_stream_t stream);

/* rw_conv3x3_wino4_f32 with ToRGB in its epilogue, as rw_conv3x3_wino_to_rgb_f32 (models.py:639-655): the last styled
 * convolution of the generator; rgb->out = ToRGB(act(conv + noise + bias)) + rgb bias + skip, the feature map is not
 * written.  Shapes: out_ch == 32, in_ch % 8 == 0, in_ch <= 512, w % 64 == 0, h % 8 == 0; uf from
 * rw_pack_conv_weight_wino4_f32. */
int rw_conv3x3_wino4_to_rgb_supported(int out_ch, int in_ch, int h, int w);
int rw_conv3x3_wino4_to_rgb_f32(const float* x, const float* uf, int batch, int in_ch, int out_ch, int h, int w,
                                float w_scale, const rw_conv_epilogue* ep, const rw_rgb_epilogue* rgb,
                                rw_stream_t stream);

/* F.conv_transpose2d(x, scale*W^T, stride=2, padding=0) [* demod]     (models.py:315-316,328)
 * x (B,Cin,H,W) -> y (B,Cout,2H+1,2W+1), wp from rw_pack_conv_weight_f32 mode 1. */
int rw_conv_transpose3x3s2_f32(const float* x, const float* wp, float* y, int batch, int in_ch,
                               int out_ch, int h, int w, float w_scale, const rw_conv_epilogue* ep,
                               int impl, rw_stream_t stream);

/* The quads y < H, x < W of the same transposed convolution (everything but output row 2H and column 2W, which
 * rw_conv_transpose3x3s2_f32 impl 8 writes) by the minimal-filtering algorithm F(2,2) in fp32: 25 instead of 36
 * multiplications per 2x2 block of quads and channel pair; coefficients 0, +-1 (the direct sum's error class).
 * Shapes: out_ch % 32 == 0, 16 <= in_ch <= 512, in_ch % 8 == 0, and w % 32 == 0 with h % 4 == 0, w == 16 with h % 8 == 0,
 * or the whole 8 x 8 / 4 x 4 maps (two / eight images per workgroup; these take style == NULL, i.e. an input that
 * already carries its style, RW_ERR_UNSUPPORTED otherwise).
 *   uf: rw_packed_conv_transpose_wino_elems(out_ch, in_ch) = 28*out_ch*in_ch floats from
 *       rw_pack_conv_transpose_wino_f32 (w = the (1,out_ch,in_ch,3,3) parameter as rw_pack_conv_weight_f32 takes it):
 *       uf[o / 16][i / 4][q][lane][xi % 4], xi = 4 q + e < 25 the point (rw_upwino.hip lists them), 25..27 zero.
 *   style (batch x in_ch) and demod (batch x out_ch) as in rw_conv_epilogue, either may be NULL. */
int rw_conv_transpose3x3s2_wino_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_conv_transpose_wino_elems(int out_ch, int in_ch);
int rw_pack_conv_transpose_wino_f32(const float* w, float* uf, int out_ch, int in_ch, rw_stream_t stream);
int rw_conv_transpose3x3s2_wino_f32(const float* x, const float* uf, float* y, int batch, int in_ch, int out_ch,
                                    int h, int w, float w_scale, const float* style, const float* demod,
                                    rw_stream_t stream);

/* An upsampling StyledConv in ONE pass: F.conv_transpose2d(x, scale*W^T, stride=2) [* demod] -> Blur(pad 1,1) ->
 * NoiseInjectionF -> FusedLeakyReLUF  (models.py:315-316,328; 277-281; 539-546; 622-626):
 * x (B,Cin,H,W) -> y (B,Cout,2H,2W).  A stride-2 transposed 3x3 convolution followed by the 4x4 FIR is a stride-2
 * transposed convolution with their 6x6 composition, and each of its four output-parity phases is a 3x3 'same'
 * convolution of x: the phases run as 4*Cout virtual channels of the F(4x4,3x3) kernel above (its error class; like
 * it the host uses it inside the un-hooked whole-generator forward only), the (2H+1)x(2W+1) map is never written, there are no border strips.
 * Shapes: out_ch % 8 == 0, 8 <= in_ch <= 512, in_ch % 8 == 0, w % 64 == 0, h % 8 == 0.
 *   uf: rw_packed_conv_transpose_blur_wino4_elems(out_ch, in_ch) = 144*out_ch*in_ch floats from
 *       rw_pack_conv_transpose_blur_weight_wino4_f32(w, k4): w = the (1,out_ch,in_ch,3,3) parameter, k4 = the 4x4
 *       FIR buffer of the layer's Blur (already multiplied by 4); layout of rw_pack_conv_weight_wino4_f32 with
 *       virtual channel 4 o + 2 py + px.
 *   ep: style / demod / noise (B x 2H x 2W) + noise_w / bias + act as in rw_conv_epilogue.
 *   post_scale (batch x out_ch, nullable): a factor on the finished result -- the style of the convolution that
 *       consumes y, which then runs with style == NULL (the F(4x4,3x3) kernels skip the multiply in their loop). */
int rw_conv_transpose_blur_wino4_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_conv_transpose_blur_wino4_elems(int out_ch, int in_ch);
int rw_pack_conv_transpose_blur_weight_wino4_f32(const float* w, const float* k4, float* uf, int out_ch, int in_ch,
                                                 rw_stream_t stream);
int rw_conv_transpose3x3s2_blur_wino4_f32(const float* x, const float* uf, float* y, int batch, int in_ch,
                                          int out_ch, int h, int w, float w_scale, const rw_conv_epilogue* ep,
                                          const float* post_scale, rw_stream_t stream);

/* The three F(4x4,3x3) operations above with their 36 GEMMs on the 16-bit matrix pipe, fp32-equivalent by an EXACT
 * operand split ("H16", rw_wino4.hip): every transformed input V and weight U is written as the sum of two f16 numbers
 * (round to nearest twice: representation error <= 2^-22 relative), all four piece products are accumulated in fp32 by
 * v_mfma_f32_16x16x16_f16.  Per-product error <= 2^-21 of the product (fp32 multiply: 2^-24); accumulation, transforms
 * and epilogue are the fp32 kernels' -- same shapes, same results within the F(4x4,3x3) error class (tested at the same
 * bars), 36 MFMAs of ~17 cycles per k-quad instead of 32-cycle fp32 MFMAs that block the vector lanes.
 * Powers of two keep the pieces inside f16's normal range.  Neither of them is ever handed from one launch to the next
 * through a device scalar (round 4 did: a 4-byte value zeroed by a memset, raised with atomics and read back by the next
 * launch was occasionally read stale -- images 0.01 - 0.05 off; the forward of the reference is a pure function of its
 * inputs, utils/stylegan2/models.py:126-141, and so is this one now):
 *   uf: rw_packed_*_wino4h_elems floats from rw_pack_*_wino4h_f32: the wino4 layout with every float replaced by the
 *       32-bit word Uh | Ul << 16 of U * u_scale, + 4 trailing floats [1 / u_scale, u_scale, 0, 0] that NO kernel reads
 *       (they tell the format from the fp32 packing by size and let a host inspect what a buffer was packed with);
 *   u_scale (BY VALUE, pack entry points) / u_inv = 1 / u_scale (BY VALUE, convolution entry points): the power of two
 *       that rw_split_weight_scale() derives from max |U|; max |U| comes from rw_*_absmax_f32 (a bound, below), read
 *       back by the host ONCE per weight version;
 *   a BOUND on a map: RW_BOUND_LANES floats whose maximum is >= max |x| -- every wave of a consumer loads the vector
 *       (one float per lane, an ordinary vector load of data the previous launch stored plainly) and reduces it;
 *   x_amax (required): the bound of the input map (without the on-load style; the kernel multiplies by the style's
 *       largest factor itself) -- what the producer of x left in its y_amax, or rw_absmax_f32(x).  A bound that is too
 *       small overflows f16 (inf/NaN in the result); a bound that is 2^k too large costs k low bits of the smallest
 *       values only;
 *   y_amax (nullable): rw_bound_floats(elements of y) floats.  Every wave (or workgroup) of the producer stores ITS
 *       maximum into its own slot behind the first RW_BOUND_LANES floats -- plain stores, nothing is zeroed first,
 *       every slot that is read is written by the same launch -- and one 64-workgroup launch reduces the slots into
 *       y_amax[0 .. RW_BOUND_LANES): the bound of y.  Kernel boundaries order all of it like any feature map.
 * Everything else as in the fp32 entry points. */
#define RW_BOUND_LANES 64
/* floats of a y_amax buffer for a result of n_elems floats (64 + slots: every producer needs at most
 * 2048 + n_elems / 1024 + 1 of them; one that would need more measures its result with rw_absmax_f32 instead) */
long long rw_bound_floats(long long n_elems);
/* out (rw_bound_floats(n) floats) <- the bound of x[0 .. n) */
int rw_absmax_f32(const float* x, long long n, float* out, rw_stream_t stream);
/* u_scale = 2^(15 - e) with max |U| < 2^e (1 for max |U| == 0): |U u_scale| < 2^15 */
float rw_split_weight_scale(float u_absmax);
/* bound (rw_bound_floats(0) floats) <- max |U| over the transformed weights the matching rw_pack_* would store */
int rw_conv_weight_wino4h_absmax_f32(const float* w, int out_ch, int in_ch, float* bound, rw_stream_t stream);
int rw_conv_transpose_blur_weight_wino4h_absmax_f32(const float* w, const float* k4, int out_ch, int in_ch, float* bound,
                                                    rw_stream_t stream);
int rw_conv_transpose_weight_winoh_absmax_f32(const float* w, int out_ch, int in_ch, float* bound, rw_stream_t stream);
int rw_dconv_weight_absmax_f32(const float* w, int out_ch, int in_ch, float* bound, rw_stream_t stream);
int rw_dconv_transpose_blur_weight_absmax_f32(const float* w, const float* k4, int out_ch, int in_ch, float* bound,
                                              rw_stream_t stream);
long long rw_packed_conv_weight_wino4h_elems(int out_ch, int in_ch);
int rw_pack_conv_weight_wino4h_f32(const float* w, float* uf, int out_ch, int in_ch, float u_scale, rw_stream_t stream);
int rw_conv3x3_wino4h_f32(const float* x, const float* uf, float* y, int batch, int in_ch, int out_ch, int h,
                          int w, float w_scale, const rw_conv_epilogue* ep, float u_inv, const float* x_amax,
                          float* y_amax, rw_stream_t stream);
int rw_conv3x3_wino4h_to_rgb_f32(const float* x, const float* uf, int batch, int in_ch, int out_ch, int h, int w,
                                 float w_scale, const rw_conv_epilogue* ep, const rw_rgb_epilogue* rgb, float u_inv,
                                 const float* x_amax, rw_stream_t stream);
/* rw_conv3x3_wino4_to_rgb_f32 / rw_conv3x3_wino4h_to_rgb_f32 with the ToRGB's skip still one level down: skip_half
 * (batch, 3, h / 2, w / 2) and the 4 x 4 FIR k4 that upsamples it (up 2, pads 2 / 1), upsampled in the epilogue with the
 * bits of rw_upfirdn2d_f32; rgb->skip must be NULL.  Same image as with the materialised skip. */
int rw_conv3x3_wino4_to_rgb_up_f32(const float* x, const float* uf, int batch, int in_ch, int out_ch, int h, int w,
                                   float w_scale, const rw_conv_epilogue* ep, const rw_rgb_epilogue* rgb,
                                   const float* skip_half, const float* k4, rw_stream_t stream);
int rw_conv3x3_wino4h_to_rgb_up_f32(const float* x, const float* uf, int batch, int in_ch, int out_ch, int h, int w,
                                    float w_scale, const rw_conv_epilogue* ep, const rw_rgb_epilogue* rgb, float u_inv,
                                    const float* x_amax, const float* skip_half, const float* k4, rw_stream_t stream);
long long rw_packed_conv_transpose_blur_wino4h_elems(int out_ch, int in_ch);
int rw_pack_conv_transpose_blur_weight_wino4h_f32(const float* w, const float* k4, float* uf, int out_ch, int in_ch,
                                                  float u_scale, rw_stream_t stream);
int rw_conv_transpose3x3s2_blur_wino4h_f32(const float* x, const float* uf, float* y, int batch, int in_ch,
                                           int out_ch, int h, int w, float w_scale, const rw_conv_epilogue* ep,
                                           const float* post_scale, float u_inv, const float* x_amax,
                                           float* y_amax, rw_stream_t stream);

/* The same three operations as DIRECT sums on the 16-bit matrix pipe (rw_dconv.hip, round 4): no transform at all -- an
 * input value is scaled by style 2^eV and split into its f16 pair ONCE per workgroup while it is staged into LDS, and read
 * nine times as a ready operand of v_mfma_f32_16x16x32_f16 (a lane's eight k values = [Vh c0..c3, Vl c0..c3] of four input
 * channels against [Uh c0..c3] twice, then [Ul c0..c3] twice: all four piece products, fp32 accumulation).  4x the
 * multiplies of F(4x4,3x3) and none of its transforms.  Error class: the direct fp32 kernels' (per-product 2^-21, no transform constants).
 * Shapes: in_ch % 16 == 0 (<= 512), w % 32 == 0; rw_dconv3x3: out_ch % 32 == 0, h % 16 == 0; the transposed form:
 * out_ch % 16 == 0, h % 8 == 0; to_rgb: out_ch == 32.
 *   wp: rw_packed_dconv_*_elems floats from rw_pack_dconv_*_f32: wp[o / 16][9 (i / 16) + tap][Uh | Ul][lane = 16 ((i % 16) / 4)
 *       + o % 16][4 halves: channels 4 ((i % 16) / 4) + (0..3)] (the kernels double them into the operand) + 4 trailing
 *       floats [1 / u_scale, u_scale, 0, 0] (not read by any kernel).  The transposed form packs the four output-parity phases of conv_transpose (*) blur as
 *       blocks of 16 virtual channels: block 4 (o / 16) + 2 py + px.
 * Two kernel families behind the same entry points: one-role workgroups (two per CU), and -- where in_ch >= 32, the
 * epilogue carries a style, w % 64 == 0 and (rw_dconv3x3_f32) out_ch % 64 == 0, h % 8 == 0 -- workgroups of eight
 * multiplying and four staging waves (RW_DCONV_V=1 forces the first).  Measured on MI355X: as fast as the split F(4x4,3x3)
 * kernels on the 512^2 / 1024^2 layers, not faster (the 16-bit pipe retires an MFMA per 20 cycles and SIMD at ~1.7 GHz
 * under this load: DESIGN.md section 4.4) -- the Python host leaves them opt-in (RW_MM_DIRECT16=1).
 * u_scale / u_inv / x_amax / y_amax / ep / post_scale / rgb: as in the wino4h entry points. */
int rw_dconv3x3_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_dconv_weight_elems(int out_ch, int in_ch);
int rw_pack_dconv_weight_f32(const float* w, float* wp, int out_ch, int in_ch, float u_scale, rw_stream_t stream);
int rw_dconv3x3_f32(const float* x, const float* wp, float* y, int batch, int in_ch, int out_ch, int h, int w,
                    float w_scale, const rw_conv_epilogue* ep, float u_inv, const float* x_amax, float* y_amax,
                    rw_stream_t stream);
/* rw_dconv3x3_f32 that ALSO leaves the channel sums of the ToRGB which reads its result (ToRGBF.forward, models.py:639-655;
 * the reference's generator applies it to the output of every second styled convolution, :126-131): rgb->out receives
 * rw_dconv3x3_rgb_partials(out_ch) = out_ch / 32 partial images, layout (partial, batch, 3, h, w) -- one per wave's 32
 * out-channels, summed while the activated values are in registers; rgb->weight (3, out_ch), rgb->style (batch, out_ch),
 * rgb->scale as in rw_rgb_epilogue, rgb->bias / rgb->skip are NOT used here.  rw_rgb_combine_f32 finishes the ToRGB:
 *   out[b][c][p] = sum_k partial[k][b][c][p] + bias[c] + skip[b][c][p]      (bias, skip nullable; hw % 4 == 0).
 * The feature map y is written as by rw_dconv3x3_f32 (the next layer reads it); the second pass over it (rw_to_rgb_f32)
 * disappears.  Same shapes as rw_dconv3x3_f32, and the same choice of kernel: with a style on load (ep->style), in_ch >= 32,
 * 64 | out_ch, 8 | h, 64 | w the specialised persistent kernel (twelve waves per compute unit), the one-role kernels otherwise
 * (RW_DCONV_V=1: always) -- y and the partial images are bit-identical to rw_dconv3x3_f32's y + a float32 channel sum. */
int rw_dconv3x3_rgb_partials(int out_ch);
int rw_dconv3x3_rgb_partial_f32(const float* x, const float* wp, float* y, int batch, int in_ch, int out_ch, int h, int w,
                                float w_scale, const rw_conv_epilogue* ep, const rw_rgb_epilogue* rgb, float u_inv,
                                const float* x_amax, float* y_amax, rw_stream_t stream);
int rw_rgb_combine_f32(const float* partials, int n_part, const float* bias, const float* skip, float* y, int batch,
                       int64_t hw, rw_stream_t stream);
/* The same with the skip still one level down: skip_half (batch, 3, h / 2, w / 2) is upsampled inside the kernel by the
 * 4 x 4 FIR k4 (rw_upfirdn2d_f32 with up 2, pads 2 / 1: same taps, same order) -- bit-identical to rw_upfirdn2d_f32 +
 * rw_rgb_combine_f32, one launch and one h x w image less.  w % 4 == 0, h % 2 == 0. */
int rw_rgb_combine_up_f32(const float* partials, int n_part, const float* bias, const float* skip_half, const float* k4,
                          float* y, int batch, int h, int w, rw_stream_t stream);
int rw_dconv3x3_to_rgb_supported(int out_ch, int in_ch, int h, int w);
int rw_dconv3x3_to_rgb_f32(const float* x, const float* wp, int batch, int in_ch, int out_ch, int h, int w,
                           float w_scale, const rw_conv_epilogue* ep, const rw_rgb_epilogue* rgb, float u_inv,
                           const float* x_amax, rw_stream_t stream);
int rw_dconv_transpose_blur_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_dconv_transpose_blur_weight_elems(int out_ch, int in_ch);
int rw_pack_dconv_transpose_blur_weight_f32(const float* w, const float* k4, float* wp, int out_ch, int in_ch,
                                            float u_scale, rw_stream_t stream);
int rw_dconv_transpose3x3s2_blur_f32(const float* x, const float* wp, float* y, int batch, int in_ch, int out_ch, int h,
                                     int w, float w_scale, const rw_conv_epilogue* ep, const float* post_scale,
                                     float u_inv, const float* x_amax, float* y_amax, rw_stream_t stream);

/* The upsampling StyledConv in one pass at the transposed convolution's OWN multiply count (rw_tconv.hip, round 5):
 * utils/stylegan2/models.py:313-316 F.conv_transpose2d(stride=2) as a direct sum on the 16-bit matrix pipe (exact f16 operand
 * split, fp32 accumulation; 9 multiplies per input position and channel pair where the phase kernels above spend 36), its
 * (2H+1) x (2W+1) result kept in LDS, the 4x4 FIR of Blur(pad 1,1) (:275-281) read from there, NoiseInjection (:539-546),
 * FusedLeakyReLU (:232-257) and post_scale in the same epilogue: x (B, in_ch, H, W) -> y (B, out_ch, 2H, 2W).
 *   wp: rw_packed_dconv_weight_elems floats from rw_pack_dconv_weight_f32 -- the PLAIN packing of dconv.weight (no
 *       composition with the blur), u_inv its scale; k4: the 4x4 FIR buffer (already multiplied by 4);
 *   shapes: in_ch % 16 == 0 (<= 512), out_ch % 16 == 0, h % 16 == 0, w % 32 == 0;
 *   ep / post_scale / x_amax / y_amax: as in rw_dconv_transpose3x3s2_blur_f32;
 *   the kernel's form is picked by in_ch (32 .. 128: one persistent workgroup per CU with specialised waves; otherwise one
 *   8-wave workgroup per CU and tile); environment RW_TCONV_TY = 0 / 16 / 8 forces a form, RW_TCONV_GRID the persistent
 *   form's workgroup count (diagnostics). */
int rw_tconv_blur_supported(int out_ch, int in_ch, int h, int w);
int rw_tconv_blur_f32(const float* x, const float* wp, const float* k4, float* y, int batch, int in_ch, int out_ch, int h,
                      int w, float w_scale, const rw_conv_epilogue* ep, const float* post_scale, float u_inv,
                      const float* x_amax, float* y_amax, rw_stream_t stream);
/* The STAGED forms of rw_tconv_blur_f32 (round 12).  The one-workgroup-per-tile forms (RW_TCONV_TY 8 / 16 / 32) convert the
 * whole in_ch window once per 16 (32) out-channels; with a scratch buffer they convert the map ONCE -- a streaming pre-pass
 * writes it as ready operand words, rw_tconv_stage_bytes(batch, in_ch, out_ch, h, w) bytes (as many as the map; 0 where
 * the launch would not take a staged form: its shape, its form, the environment) -- and the
 * convolution copies its windows from there into LDS.  Same bits: the pre-pass runs the other form's arithmetic.
 *   rw_tconv_stage_buffer(stream, ptr, bytes): the scratch of `stream` on the current device (16-byte aligned; the caller
 *   owns it and keeps it alive until the launches that use it have run; ptr NULL with bytes 0 forgets it).  This is the one
 *   piece of state the library keeps, and it decides nothing about results.  Not to be called while the stream is being
 *   captured.  rw_tconv_blur_f32 takes the staged form when the stream's buffer is large enough, the form is one of the
 *   three and in_ch >= RW_TCONV_STAGED_MIN_IN (environment; default 256); RW_TCONV_STAGED = 0 turns it off.  Both launches
 *   go to `stream`, back to back.  The two entries join under ABI 11 like the other added entries. */
long long rw_tconv_stage_bytes(int batch, int in_ch, int out_ch, int h, int w);
int rw_tconv_stage_buffer(rw_stream_t stream, void* ptr, long long bytes);

/* rw_conv_transpose3x3s2_wino_f32 (the F(2,2) quads of the stride-2 transposed convolution) with its 25 GEMMs on the
 * 16-bit matrix pipe and the exact f16 operand split of the wino4h entry points (rw_upwino.hip): one
 * v_mfma_f32_16x16x32_f16 per point takes the two k-quads of an 8-channel interval (25 MFMAs of ~17 cycles per 8
 * channels against 50 fp32 MFMAs of 32 that block the vector lanes).  Coefficients 0, +-1 as before: the direct sum's
 * error class plus <= 2^-21 per product (tested at the fp32 kernel's bars).  Wide maps only: w % 32 == 0, h % 4 == 0,
 * 16 <= in_ch <= 512, in_ch % 8 == 0, out_ch % 32 == 0.
 *   uf: rw_packed_conv_transpose_winoh_elems = 16*out_ch*in_ch + 4 floats from rw_pack_conv_transpose_winoh_f32 (the
 *       25 points carry 16 distinct weights): uf[o / 16][i / 8][wi = 0..15][lane = 16 ((i % 8) % 4) + o % 16]
 *       [{0: Uh, 1: Ul}], each 32-bit word the f16 pair of channels (i, i + 4) of the interval; trailer
 *       [1 / u_scale, u_scale, 0, 0] (not read by any kernel);
 *   u_scale / u_inv / x_amax (the bound of x before the style): as for rw_conv3x3_wino4h_f32. */
int rw_conv_transpose3x3s2_winoh_supported(int out_ch, int in_ch, int h, int w);
long long rw_packed_conv_transpose_winoh_elems(int out_ch, int in_ch);
int rw_pack_conv_transpose_winoh_f32(const float* w, float* uf, int out_ch, int in_ch, float u_scale, rw_stream_t stream);
int rw_conv_transpose3x3s2_winoh_f32(const float* x, const float* uf, float* y, int batch, int in_ch, int out_ch,
                                     int h, int w, float w_scale, const float* style, const float* demod, float u_inv,
                                     const float* x_amax, rw_stream_t stream);

/* NoiseInjectionF (models.py:535-546): y[b][c][p] = x[b][c][p] + noise_w[0] * noise[b][p] */
int rw_noise_add_f32(const float* x, const float* noise, const float* noise_w, float* y,
                     int batch, int channels, int64_t hw, rw_stream_t stream);

/* BlurF(pad=(1,1)) -> NoiseInjectionF -> FusedLeakyReLUF in one pass for upsampling layers
 * (models.py:277-281,481-485,539-546,622-626): x (B,C,2H+1,2W+1) -> y (B,C,2H,2W);
 * k4 = the 4x4 FIR buffer (already multiplied by 4). */
int rw_blur_noise_act_f32(const float* x, const float* k4, const float* noise, const float* noise_w,
                          const float* bias, float* y, int batch, int channels, int out_h, int out_w,
                          rw_stream_t stream);
/* The same with a per (image, channel) factor on the result (batch x channels, nullable): the style of the
 * convolution that consumes y, handed over pre-multiplied. */
int rw_blur_noise_act_scaled_f32(const float* x, const float* k4, const float* noise, const float* noise_w,
                                 const float* bias, const float* post_scale, float* y, int batch, int channels,
                                 int out_h, int out_w, rw_stream_t stream);
/* ... and y_amax (nullable, rw_bound_floats(batch * channels * out_h * out_w) floats) receives the bound of the result,
 * post_scale included: the x_amax of a split-operand (wino4h / winoh) convolution that reads y. */
int rw_blur_noise_act_amax_f32(const float* x, const float* k4, const float* noise, const float* noise_w,
                               const float* bias, const float* post_scale, float* y, int batch, int channels,
                               int out_h, int out_w, float* y_amax, rw_stream_t stream);

/* ToRGBF (models.py:628-655): y[b][c][p] = sum_i (W[c][i]*style[b][i]*w_scale) x[b][i][p]
 * + bias[c] + skip[b][c][p]; out channels = 3, skip nullable. */
int rw_to_rgb_f32(const float* x, const float* w, const float* style, const float* bias,
                  const float* skip, float* y, int batch, int in_ch, int64_t hw, float w_scale,
                  rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Key statistics -- replaces RunningSecondMoment.add (utils/runningstats.py:1086-1097,
 * progress_addbmm :1181-1190) and RunningVariance.add's reductions (:763-788)
 * ------------------------------------------------------------------------------------- */

/* mom2 (C,C) += a^T a on fp32 MFMA.
 *   layout 0: a is (rows, C) row-major, as the reference passes it
 *             (rewrite/ganrewrite.py:90-93);
 *   layout 1: a is (batch, C, hw) NCHW, rows = batch*hw -- the key map as the generator
 *             produced it (no permute copy).
 * workspace: >= rw_second_moment_workspace_bytes(C, rows) bytes of device scratch = ksplit * C * C * 4, one C x C slab
 *   per row slice: with tiles of 128 channels (64 when C < 128), pairs = tiles (tiles + 1) / 2 and chunks of 16 rows,
 *   ksplit = min(512 / pairs, max(chunks / 8, 1)), at least 1 (integer divisions).
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null a / mom2 / workspace, rows or C < 1, a layout outside {0, 1}.
 * RW_ERR_UNSUPPORTED (nothing launched): layout 0 with C % 4 != 0; layout 1 with hw % 16 != 0 or rows % hw != 0. */
int64_t rw_second_moment_workspace_bytes(int channels, int64_t rows);
int rw_second_moment_f32(const float* a, float* mom2, int64_t rows, int channels, int64_t hw,
                         int layout, void* workspace, rw_stream_t stream);

/* per-channel sum and sum of squares over rows (same layouts, any C and hw); sums (2,C) are OVERWRITTEN.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null a / sums, rows or C < 1, layout 1 with rows % hw != 0. */
int rw_channel_sums_f32(const float* a, float* sums, int64_t rows, int channels, int64_t hw,
                        int layout, int square_input, rw_stream_t stream);

/* The same reductions about a pivot, for a centred sum of squares that does not cancel against mean^2
 * (RunningVariance.add, utils/runningstats.py:770-777: (a - batch_mean).pow(2).sum(0)).  v is the sample, squared when
 * square_input; the pivot p_c is the mean of the first v of channel c (layout 1: min(hw, 256) pixels of image 0; layout
 * 0: min(rows, 16) rows).  moments (3,C) are OVERWRITTEN:
 *   moments[0][c] = p_c,   moments[1][c] = sum (v - p_c),   moments[2][c] = sum (v - p_c)^2
 * so that mean = p + S1 / n and sum (v - mean)^2 = S2 - S1^2 / n.  The map is read once.  Same layouts, same refusals as
 * rw_channel_sums_f32. */
int rw_channel_moments_f32(const float* a, float* moments, int64_t rows, int channels, int64_t hw,
                           int layout, int square_input, rw_stream_t stream);

/* Search (rewrite/ganrewrite.py:582-594, :610-650): the response of every pixel of a key map to K query keys,
 *   heat[b][k][p] = sum_c keys[k][c] * a[b][c][p],     peak[b][k] = max_p heat[b][k][p]
 * a (images, C, hw) NCHW as the generator left it, keys (K, C), heat (images, K, hw), peak (images, K) nullable.
 * a is read once for all K keys.  The sum of a pixel runs over the channels in order, one fused multiply-add each: a
 * row of heat is bit-identical whatever images, K, the key's slot or the alignment of the pointers, and peak is the
 * plain maximum of the heat row.  RW_ERR_BAD_ARGUMENT (nothing launched) for a null a / keys / heat, images, channels
 * or hw < 1, K outside 1 .. RW_KEY_RESPONSE_MAX_KEYS, or C * hw / K * hw / K * C / images past 31 bits. */
#define RW_KEY_RESPONSE_MAX_KEYS 8
int rw_key_response_f32(const float* a, const float* keys, float* heat, float* peak,
                        int64_t images, int channels, int64_t hw, int n_keys, rw_stream_t stream);

/* Overlays: the bytes of ImageVisualizer.masked_image (utils/imgviz.py:56-122, border_from_mask :309-330, the centred
 * bilinear grid of utils/upsample.py:124-156) and of renormalize.as_image (utils/renormalize.py:15-19) for a batch, in
 * one launch.  image (images, 3, H, W) float32 in the generator's range, out (images, H, W, 3) uint8.
 *   bytes:   s = trunc(clamp(x * 127.5f + 127.5f, 0, 255)), product and sum rounded separately (no fused multiply-add).
 *   inside:  mode 0: no selector, every pixel shows s.
 *            mode 2: selector = bytes (images, H, W), non-zero = inside (sel_height, sel_width must be H, W).
 *            mode 1: selector = float32 heat maps (images, h, w), inside = up(y, x) > level (NaN compares false) with
 *                    up bilinear, zeros outside the map: fy = (y + 1/2) h / H - 1/2, rows floor(fy) and floor(fy) + 1
 *                    weighted 1 - (fy - floor(fy)) and fy - floor(fy); the same along x.
 *   outline: border = not inside, and some pixel of the image within Chebyshev distance `thickness` is inside
 *            (= border_from_mask(mask, thickness, outside=True)); thickness 0: none.
 *   blend:   border pixels show border_rgb, inside pixels s (or inside_rgb when it is >= 0), every other pixel
 *            trunc(clamp(outside_bright * s, 0, 255)), one float32 product.  Colours: r | g << 8 | b << 16.
 * The inside bit of a pixel depends on (y, x), the sizes, the selector and level alone: an image's bytes are the same
 * alone or in a batch and whatever the alignment of the pointers.  Every byte of out is written exactly once.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null image / out, images, H or W < 1, 3 * H * W past 31 bits, a mode outside
 * 0 .. 2, mode != 0 with a null selector, mode 2 with a selector that is not H x W, thickness outside
 * 0 .. RW_RENDER_MAX_THICKNESS, a non-finite outside_bright, mode 1 with h * w, (2 H + 1) h or (2 W + 1) w past 31 bits.
 * RW_ERR_UNSUPPORTED (nothing launched): mode 1 with h < 2 or w < 2 (the host grid degenerates to a constant). */
#define RW_RENDER_MAX_THICKNESS 8
int rw_render_bytes_f32(const float* image, const void* selector, uint8_t* out, int64_t images, int height, int width,
                        int mode, int sel_height, int sel_width, float level, int thickness, uint32_t border_rgb,
                        int32_t inside_rgb, float outside_bright, rw_stream_t stream);

/* PNG encoding of bytes that are on the device: the per-byte work of renormalize.as_url's img.save(format='png')
 * (utils/renormalize.py:22-32) and of SaveImageWorker.work (utils/imgsave.py:58-66), for image (images, H, W, 3) uint8 --
 * what rw_render_bytes_f32 writes.  The PNG is 8-bit truecolour, not interlaced: signature, IHDR, one IDAT, IEND.
 *   stream:   H rows of a filter type byte and 3 W residuals.  The type of a row is libpng's heuristic: the smallest, over
 *             types 0 .. 4, sum of |residual as a signed byte|, ties to the lowest type; the prior row of row 0 is zero.
 *   segments: the stream is cut into segments of S = rw_png_segment_bytes() bytes, nseg = ceil(H (1 + 3 W) / S).
 *   IDAT:     a zlib stream: 78 01; per segment one deflate block with dynamic Huffman codes and LITERALS ONLY (HDIST = 0,
 *             one distance code of length 0: RFC 1951 3.2.7), its end-of-block, and an empty stored block (000, pad to the
 *             byte, 00 00 FF FF), so that every segment is a whole number of bytes and stands alone; then 01 00 00 FF FF
 *             and the Adler-32.  No LZ77 matches: flat images cost at least one bit per byte.
 * The host does the O(256)-per-image work between the calls: from hist it builds one complete prefix code per image
 * (lengths <= 15, symbol 256 counted once per segment), the complete code-length code (<= 7) and the bits of the block
 * header; it frames the chunks (CRC-32) and folds the segments' Adler sums.
 *   rw_png_filter_u8   row_type (images, H) bytes; stream (images, nseg S) bytes, 16-byte aligned -- of every 16-byte
 *                      piece that starts inside an image's stream all 16 bytes are written, zeros past its end;
 *                      hist_part (images, nseg, 256) and hist (images, 256) counts of the stream's bytes;
 *                      adler (images, nseg, 2): s1 = sum d_k and s2 = sum (n - k) d_k mod 65521 over the n bytes d_0 ..
 *                      of a segment (a, b) -> (a + s1, b + n a + s2) folds a segment into a running Adler-32.
 *   rw_png_encode_u8   table (images, rw_png_table_words()) uint32: [0] the bits of the block header (at most 2048),
 *                      [1 + s] for s = 0 .. 256 the code of symbol s, bit-reversed (as it lies in the stream), | its length
 *                      << 16, [258 ..] the header's bits, first bit in bit 0.  coded (images, nseg, C) bytes with
 *                      C = rw_png_segment_capacity(), 16-byte aligned: a segment's bytes from the start of its slot;
 *                      lengths (images, nseg) their number.
 *   rw_png_compact_u8  offsets (segments) uint64 scratch; head (segments, 3) uint32 = length, s1, s2; bytes: the
 *                      segments back to back, in order.  A segment that would end past `capacity` bytes is left out (its
 *                      length is still reported).  The host sizes `bytes` from hist and its code lengths.
 * Histograms and sums follow the rule of the bounds: LDS atomics inside a workgroup, plain stores of per-workgroup
 * partials, a small launch that adds them in order; no global atomics, nothing zeroed first, one writer per byte.  All of
 * it is integer work: an image's PNG is the same on every run, alone or in a batch.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null pointer, images < 1, a grid past 31 bits, a stream / coded pointer that
 * is not 16-byte aligned.  RW_ERR_UNSUPPORTED (nothing launched): H or W < 1, a stream of 2^31 bytes or more. */
int64_t rw_png_segment_bytes(void);
int64_t rw_png_segment_capacity(void);
int64_t rw_png_table_words(void);
int rw_png_filter_u8(const uint8_t* image, uint8_t* row_type, uint8_t* stream, uint32_t* hist_part, uint32_t* hist,
                     uint32_t* adler, int64_t images, int height, int width, rw_stream_t stream_);
int rw_png_encode_u8(const uint8_t* stream, const uint32_t* table, uint8_t* coded, uint32_t* lengths, int64_t images,
                     int height, int width, rw_stream_t stream_);
int rw_png_compact_u8(const uint8_t* coded, const uint32_t* lengths, const uint32_t* adler, uint64_t* offsets,
                      uint32_t* head, uint8_t* bytes, int64_t capacity, int64_t segments, rw_stream_t stream_);

/* PNG decoding on the device: the way back -- what PIL.Image.open(path).convert('RGB') does for every file that
 * compute_dl reads (metrics/distances.py:67-70) and what renormalize.from_url does for a data URL (utils/renormalize.py),
 * for a batch of files of ONE shape (H, W, channels), 8 bits a sample, not interlaced: channels 1 (grey), 3 (truecolour)
 * or 4 (truecolour with alpha).  The host reads the chunks (signature, IHDR, CRC-32 of every chunk, the IDATs joined,
 * IEND), checks the two bytes of the zlib header and hands over the RAW DEFLATE stream of each file (RFC 1951: the IDAT
 * payload without its 2-byte header and 4-byte Adler trailer); it compares the trailer with the sums below.
 *   rw_png_inflate_u8   coded: one buffer that holds every stream; span (images, 2) uint64 = offset into coded and length
 *                       of each stream (any alignment; nothing outside a span is read).  One wave inflates one stream
 *                       into stream + image * stride, `expect` = H (1 + channels W) bytes of it; stride >= expect, a
 *                       multiple of 16, stream 16-byte aligned.  status (images, 4) uint32 = code, bytes produced, s1, s2:
 *                       s1 = sum d_k and s2 = sum (n - k) d_k mod 65521 over the n bytes produced, so the stream's
 *                       Adler-32 is (1 + s1) mod 65521 | ((n + s2) mod 65521) << 16 -- one step of the fold of
 *                       rw_png_filter_u8's sums.  What is accepted is what zlib accepts (stored, fixed and dynamic
 *                       blocks; its rules for code-length sets: rewriting_amd/csrc/rw_inflate_core.h); bytes after the
 *                       final block are ignored.  The first defect ends a stream; the bytes before it are stored.
 *   rw_png_unfilter_u8  the five filters of the PNG specification (section 9) undone, mod 256, bytes per pixel = channels;
 *                       out (images, H, W, 3) uint8, the layout of rw_render_bytes_f32: grey is written to all three
 *                       channels, alpha is dropped (PIL's convert('RGB') for modes L and RGBA).  An image whose status
 *                       code is not RW_PNG_OK is skipped: its pixels are written as zeros.  A filter type above 4 sets
 *                       RW_PNG_BAD_FILTER (the row is read as type 0; the image is not to be used).
 * Both are integer work and one writer per byte: an image's result is the same on every run, alone or in a batch.  No
 * global atomics, nothing zeroed first; neither kernel reads what it wrote to global memory.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null pointer, images < 1 or a grid past 31 bits, stride below the stream's
 * length, stride or stream not 16-byte aligned (inflate).  RW_ERR_UNSUPPORTED (nothing launched): channels outside
 * {1, 3, 4}, H or W < 1, expect < 1, a stream H (1 + channels W) of 2^31 bytes or more, W above 16 384 (the unfilter keeps
 * one row of 4 W bytes in LDS). */
#define RW_PNG_OK 0
#define RW_PNG_TRUNCATED 1        /* the coded bytes end inside a block */
#define RW_PNG_BAD_BLOCK_TYPE 2   /* BTYPE 3 */
#define RW_PNG_STORED_LENGTH 3    /* LEN is not the complement of NLEN */
#define RW_PNG_BAD_CODELEN_SET 4  /* code-length code over-subscribed or incomplete; repeat without a length, repeat past the count */
#define RW_PNG_BAD_LITLEN_SET 5   /* literal/length lengths over-subscribed or incomplete; more than 286 of them */
#define RW_PNG_BAD_DIST_SET 6     /* distance lengths over-subscribed or incomplete; more than 30 of them */
#define RW_PNG_NO_END_OF_BLOCK 7  /* symbol 256 has no code */
#define RW_PNG_BAD_SYMBOL 8       /* literal/length 286, 287, distance 30, 31, or bits that are no code of an incomplete set */
#define RW_PNG_DISTANCE_TOO_FAR 9 /* a match reaches before the first byte */
#define RW_PNG_OUTPUT_OVER 10     /* more output than expect */
#define RW_PNG_OUTPUT_UNDER 11    /* the final block ends with less output than expect */
#define RW_PNG_BAD_FILTER 12      /* a row's filter type is above 4 */
int rw_png_inflate_u8(const uint8_t* coded, const uint64_t* span, uint8_t* stream, int64_t stride, int64_t expect,
                      uint32_t* status, int64_t images, rw_stream_t stream_);
int rw_png_unfilter_u8(const uint8_t* stream, int64_t stride, uint32_t* status, uint8_t* out, int64_t images, int height,
                       int width, int channels, rw_stream_t stream_);

/* Tiles at the UI's size: the PIL.Image.resize(size, resample=BILINEAR) of renormalize.as_url(img, size=...)
 * (utils/renormalize.py:22-32), byte for byte, for image (images, H, W, 3) uint8 -- what rw_render_bytes_f32 writes --
 * into out (images, OH, OW, 3) uint8, which rw_png_filter_u8 reads.  Pillow's 8-bit resampler is integer arithmetic over
 * fixed-point coefficients that the host computes in double (precompute_coeffs + normalize_coeffs_8bpc, bilinear filter,
 * support 1).  For one axis of length n resized to m:
 *   scale = n / m;  fs = max(scale, 1.0);  support = fs;  K = 2 * ceil(support) + 1
 *   for o in 0 .. m - 1:
 *     center = (o + 0.5) * scale
 *     first  = max(int(center - support + 0.5), 0)
 *     count  = min(int(center + support + 0.5), n) - first
 *     w[j]   = tri((j + first - center + 0.5) * (1.0 / fs))  for j < count;   tri(v) = 1 - |v| if |v| < 1 else 0
 *     w[j]  /= sum(w)                                         (if the sum is not 0)
 *     k[j]   = int(0.5 + w[j] * 2^22)   (int(-0.5 + ...) for a negative w[j]);   k[j] = 0 for count <= j < K
 *   out[o] = clamp((2^21 + sum_j k[j] * in[first + j]) >> 22, 0, 255)          (int32, arithmetic shift)
 * All but the last line is IEEE double in this operation order, int() truncates toward zero, and it is the HOST's work
 * (rewriting_amd/resample.py): the entry takes the tables, kx (OW, kx_width) / ky (OH, ky_width) int32 and bounds_x
 * (OW, 2) / bounds_y (OH, 2) int32 = first, count, and applies the last line.  A picture is resized along x first, into
 * scratch (images, H, OW, 3) uint8, rounded to bytes there, then along y into out: the rounding between the passes is
 * part of the result.  An axis that keeps its length is not touched: its pass is skipped and its tables are not read
 * (they and, unless both axes change, scratch may be NULL).  The three channels are independent.  The sum fits int32:
 * 255 (2^22 + K / 2) + 2^21 < 2^31.  Two plain launches at most; no allocation, memset, atomic or stream drain; every
 * byte of out has one writer, and a picture's bytes are the same alone or in a batch.
 * The tables are signed and the shift is arithmetic (Pillow's other separable filters would go through unchanged), and
 * the kernels never read outside the picture whatever the tables hold: count is clamped to 0 .. K, first and first + j
 * to the axis, the sum wraps.  A wrong table gives a wrong picture, never a fault.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null image / out, a null table of an axis that changes or its width < 1, a
 * null scratch when both axes change, images < 1, OH == H and OW == W (nothing to compute: the picture is the caller's),
 * a grid past 31 bits.  RW_ERR_UNSUPPORTED (nothing launched): any extent < 1; a picture, resized picture or scratch
 * picture of 2^31 bytes or more. */
int rw_resize_bilinear_u8(const uint8_t* image, const int32_t* kx, const int32_t* bounds_x, const int32_t* ky,
                          const int32_t* bounds_y, uint8_t* scratch, uint8_t* out, int64_t images, int height, int width,
                          int out_height, int out_width, int kx_width, int ky_width, rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The rank-constrained solve -- replaces the body of ProgressiveGanRewriter.insert
 * (rewrite/ganrewrite.py:254-298) and of linear_insert (:201-252) for a SeqStyleGAN2 layer
 * (stride-1 or upsampling): forward of target_model, L1 loss, backward to dconv.weight,
 * torch.optim.Adam step, projection.
 * Arithmetic: SURVEY.md section 10.
 * ------------------------------------------------------------------------------------- */

typedef struct rw_solve_problem {
  /* shapes */
  int out_ch, in_ch, h, w, rank;
  /* constants of the layer / goal (device) */
  const float* key;      /* (in_ch, h, w)   goal_in.fmap  = adain output crop            */
  const float* style;    /* (in_ch)         goal_in.style                               */
  const float* val;      /* (out_ch, h, w)  goal_out.fmap                               */
  const float* bias;     /* (out_ch)        activate.bias; NULL = the target is the demodulated
                          *                 convolution alone (SeqTinyStyleGanRewriter, ganrewrite.py:731-738):
                          *                 no blur / noise / bias / activation, val is (out_ch, conv map) */
  const float* noise;    /* (h*w)           RandomState(0).randn(1,h*w)  (quirk Q1)     */
  const float* noise_w;  /* device scalar   noise.weight                                */
  const float* context;  /* (rank, in_ch)   orthonormal rows                            */
  const float* ortho;    /* (out_ch,in_ch,9) W0 - P(W0), nullable when !low_rank_insert  */
  /* state (device, updated in place) */
  float* weight;         /* (out_ch,in_ch,3,3) dconv.weight[0]                          */
  float* exp_avg;        /* Adam m */
  float* exp_avg_sq;     /* Adam v */
  /* per-step tables (device, length niter), computed on the host in double like torch.optim.Adam */
  const float* step_size;   /* lr / (1 - beta1^t)      */
  const float* bc2_sqrt;    /* sqrt(1 - beta2^t)       */
  int32_t* step_counter;    /* device int: index of the LAST step taken; the library pre-increments it, so it
                             * starts at -1 and step t reads step_size[t], bc2_sqrt[t], writes losses[t] */
  float* losses;            /* (niter) l1 loss of every step, written by the library        */
  /* scratch (device); element counts from rw_solve_scratch_elems().  P64 = ceil64(positions of the map the
   * convolution writes): h*w, or (2h+1)*(2w+1) for an upsampling target */
  float* conv;           /* (ksplit, out_ch, P64)  partial conv sums                      */
  float* wsq;            /* (ksplit, out_ch)                                              */
  float* gd;             /* (out_ch, P64)  g_pre*demod, zero padded                       */
  float* c2;             /* (2*out_ch)     s^2 * demod^3 * sum_p g_pre*conv | per-channel loss */
  float* grad;           /* (out_ch,in_ch,9) only for low_rank_gradient, else nullable     */
  int ksplit;
  float beta1, beta2, eps, w_scale;
  int low_rank_gradient;
  float one_minus_beta1, one_minus_beta2;   /* (1 - beta) evaluated in double on the host */
  /* upsampling (odd) layers: target = conv_transpose2d stride 2 -> blur -> noise -> activate
   * (utils/stylegan2/models.py:315-316,277-281).  key is (in_ch,h,w); val is (out_ch,2h,2w);
   * noise is (2h*2w); conv/gd rows are padded counts of the (2h+1)x(2w+1) pre-blur map. */
  int upsample;
  const float* blur_k;   /* (4,4) FIR buffer of the layer's BlurF, required iff upsample */
  /* linear_insert (rewrite/ganrewrite.py:201-252): optimise Lambda (out_ch,rank,3,3) with
   * weight = ortho(=W0) + Lambda.context; exp_avg / exp_avg_sq then hold Lambda's Adam state. */
  int linear_insert;
  float* lambda;
} rw_solve_problem;

/* split-K factor for a convolution-output map of h x w positions ((2h+1) x (2w+1) of the key for upsampling) */
int rw_solve_ksplit(int out_ch, int in_ch, int h, int w);
/* 1 when rw_solve_step_f32 takes this shape (h, w of the key crop), 0 otherwise -- like every other *_supported
 * entry point: out_ch % 64, in_ch % 16, <= 64 KB of LDS for the blur staging of an upsampling target (plain == 0)
 * and for the rank-r projection (constrained != 0).  rw_solve_step_f32 runs the same check before its first launch
 * and returns RW_ERR_UNSUPPORTED / RW_ERR_BAD_ARGUMENT. */
int rw_solve_supported(int out_ch, int in_ch, int h, int w, int upsample, int plain, int constrained);
/* sizes[0..4] = element counts of conv, wsq, gd, c2, grad for this shape; sizes[5] = the split-K factor they were
 * sized for, i.e. the value rw_solve_problem.ksplit must carry (the caller passes long long sizes[6]) */
int rw_solve_scratch_elems(int out_ch, int in_ch, int h, int w, int upsample, long long* sizes);
/* one iteration `it` (loss, gradient, Adam); project != 0 also applies W <- ortho + P(W) */
int rw_solve_step_f32(const rw_solve_problem* p, int project, rw_stream_t stream);
/* The same solve as ONE launch for iterations [it_begin, it_end) of niter (rewrite/ganrewrite.py:271-294 incl. the
 * projection rule `it % piter == 0 or it == niter - 1` when low_rank_insert != 0): every workgroup owns two out-channels
 * for the whole run, weight and Adam moments stay in registers, the key crop in LDS; no scratch of rw_solve_problem but
 * lpart (niter * out_ch floats) is used, the step counter is not touched, losses[it] is written for the iterations
 * run, state is read from / written back to weight, exp_avg, exp_avg_sq (consecutive calls continue each other).
 * rw_solve_run_supported: 1 for stride-1 targets (with or without bias), in_ch % 64 == 0, in_ch <= 512,
 * out_ch % 2 == 0, rank <= 8, no linear_insert, and either in_ch * ((h+2)(w+1) + 3 | 1) floats + scratch within 160 KB of
 * LDS (the crop resident) or w <= 16 (the crop streamed, see below); else 0 and rw_solve_step_f32 is the way. */
int rw_solve_run_supported(int out_ch, int in_ch, int h, int w, int rank, int upsample, int linear_insert);
/* Round 4: crops that do not fit the LDS (w <= 16: the watermark erase's whole 16 x 16 maps of 512 channels) run in one
 * launch too -- every thread streams ITS channel's crop row by row from a position-major copy (built in `lpart`'s tail),
 * and with low_rank_gradient the gradient phase needs no key at all (it correlates g with the one-channel maps
 * d_r^T key).  rw_solve_run_scratch_elems: floats of `lpart` = niter * out_ch (rounded up to 4) + that copy where the
 * crop is streamed. */
long long rw_solve_run_scratch_elems(int out_ch, int in_ch, int h, int w, int niter);
int rw_solve_run_f32(const rw_solve_problem* p, int it_begin, int it_end, int niter, int piter, int low_rank_insert,
                     float* lpart, rw_stream_t stream);
/* W <- W - P(W) + amount*P(1)  (zero(), ganrewrite.py:190-195) and ortho = W - P(W) helpers */
int rw_project_weight_f32(const float* w, const float* context, const float* base, float* out,
                          int out_ch, int in_ch, int taps, int rank, float scale_w, rw_stream_t stream);

/* ---- gradients of the demodulated 3x3 convolution (the autograd path of `insert` on targets the fused solver does
 * not restate: rewrite/ganrewrite.py:265-283 through utils/stylegan2/models.py:313-329).  Backward-to-input needs
 * no entry point of its own: it is rw_conv3x3_f32 on the transposed (stride 1: and flipped) weights.
 *
 * rw_conv_wgrad_f32: dw[o][i][tap] = scale * sum_{b, p} (g[b][o][p] * gscale[b][o]) * (xcol_b[(i, tap)][p] * xscale[b][i])
 *   g  (batch, out_ch, CH, CW)  gradient w.r.t. the map the convolution writes: (h, w), or (2h+1, 2w+1) when
 *                               upsample != 0 (the stride-2 transposed convolution)
 *   x  (batch, in_ch, h, w)     the convolution's input map;  gscale (batch, out_ch), xscale (batch, in_ch): nullable
 *   scratch  rw_conv_wgrad_ksplit(...) * out_ch * in_ch * 9 floats (split-K partial sums, reduced in a fixed order)
 *   dw (out_ch, in_ch, 3, 3) is overwritten. */
int rw_conv_wgrad_ksplit(int batch, int in_ch, int out_ch, int h, int w, int upsample);
int rw_conv_wgrad_f32(const float* g, const float* x, const float* gscale, const float* xscale, float* scratch,
                      float* dw, int batch, int in_ch, int out_ch, int h, int w, int upsample, float scale,
                      rw_stream_t stream);
/* out[r] = sum_j a[r][j] * b[r][j] for `rows` rows of length n (per-(image, channel) sums over a feature map) */
int rw_rowdot_f32(const float* a, const float* b, float* out, long long rows, long long n, rw_stream_t stream);

/* ---- gradients of ToRGB (a loss on the IMAGE: rewrite/ganrewrite.py:300-331 through utils/stylegan2/models.py:394-425,
 * 639-655 -- the 1x1 modulated convolution without demodulation, y[b][c][p] = sum_i w_scale w[c][i] style[b][i] x[b][i][p]
 * + bias[c] + skip[b][c][p]).  g (batch, 3, hw) is the gradient w.r.t. y; d bias is rw_bias_grad_f32, d skip is g itself.
 *
 * rw_to_rgb_input_grad_f32: gx[b][i][p] = w_scale * style[b][i] * sum_{c < 3} w[c][i] * g[b][c][p]; gx (batch, in_ch, hw) is
 *   overwritten.  16-byte accesses where hw % 4 == 0, a scalar form otherwise (as rw_to_rgb_f32).
 * rw_to_rgb_weight_sums_f32: t[b][c][i] = sum_p g[b][c][p] * x[b][i][p], t (batch, 3, in_ch) overwritten -- from it
 *   d w[c][i] = w_scale sum_b t[b][c][i] style[b][i] and d style[b][i] = w_scale sum_c t[b][c][i] w[c][i] (host side).
 *   One pass over x (batch, in_ch, hw); scratch holds rw_to_rgb_weight_sums_scratch_elems(batch, in_ch, hw) floats of
 *   per-workgroup partial sums that a second launch adds in a fixed order: no atomics, nothing to zero, two runs agree
 *   bit for bit (as rw_conv_wgrad_f32).  batch <= 65535. */
int rw_to_rgb_input_grad_f32(const float* g, const float* w, const float* style, float* gx, int batch, int in_ch,
                             int64_t hw, float w_scale, rw_stream_t stream);
long long rw_to_rgb_weight_sums_scratch_elems(int batch, int in_ch, int64_t hw);
int rw_to_rgb_weight_sums_f32(const float* g, const float* x, float* scratch, float* t, int batch, int in_ch, int64_t hw,
                              rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The perceptual network of the overfit loss: VF = vgg16(pretrained=True).features up to layer '20'
 * (rewrite/ganrewrite.py:303-304), used as 1e-2 * mse_loss(VF(gt), VF(pred)) (:316-317).  Its eight convolutions with 64 .. 512
 * channels are rw_conv3x3_wino_f32 / rw_conv3x3_f32 with w_scale 1 and no epilogue; the four entries below are the rest.
 * float32 only, on the caller's stream, no atomics, nothing zeroed or drained: two runs give the same bits.  They join
 * under ABI 11 like the other added entries.
 * ------------------------------------------------------------------------------------- */

/* What follows each convolution of VF (rewrite/ganrewrite.py:303-304,316-317: nn.ReLU after a biased nn.Conv2d, nn.MaxPool2d(2, 2)
 * after three of them), in one pass:  y[b][c][p] = max(x[b][c][p] + bias[c], 0)  and, when pooled is not NULL,
 * pooled[b][c][i][j] = the maximum of y over rows 2i, 2i + 1 and columns 2j, 2j + 1; pooled is (batch, ch, h / 2, w / 2),
 * rounded down: an odd last row or column belongs to no window.  y may be NULL when pooled is given (the full-size map is
 * then not stored), and y may be x.  16-byte accesses where w % 4 == 0 and x, y, pooled are 16-byte aligned, a scalar
 * form elsewhere.  RW_ERR_BAD_ARGUMENT (nothing launched): a null x / bias, y and pooled both null, an extent < 1. */
int rw_bias_relu_pool_f32(const float* x, const float* bias, float* y, float* pooled, int batch, int ch, int h, int w,
                          rw_stream_t stream);

/* The adjoint of rw_bias_relu_pool_f32 with respect to x (rewrite/ganrewrite.py:303-304,316-317: loss.backward() through VF),
 * from the saved y (batch, ch, h, w).  pooled == 0: g is (batch, ch, h, w) and gx = y > 0 ? g : 0.  pooled == 1: g is
 * (batch, ch, h / 2, w / 2); gx[p] = g[window of p] if y[p] > 0 and p is the FIRST maximum of its window in row-major order
 * (torch's tie rule: four equal positive values send the gradient to the top-left one, an all-zero window sends nothing),
 * else 0; positions in no window get 0.  gx (batch, ch, h, w) must be neither g nor y.  RW_ERR_BAD_ARGUMENT otherwise. */
int rw_bias_relu_pool_grad_f32(const float* g, const float* y, float* gx, int batch, int ch, int h, int w, int pooled,
                               rw_stream_t stream);

/* The first layer of VF (rewrite/ganrewrite.py:303-304,316-317: features[0], features[1]):
 *   y = relu(F.conv2d(x (batch, 3, h, w_), w (out_ch, 3, 3, 3) as stored, padding=1) + bias[o])
 * 27 multiply-adds per output in the order (channel, ky, kx), then the bias.  One workgroup owns a 16 x 64 pixel tile of an
 * image for all out-channels, whose weights sit in LDS.  RW_ERR_UNSUPPORTED (nothing launched): out_ch > 64, batch > 65535,
 * h * w_ >= 2^31.  The MFMA forms do not take in_ch == 3. */
int rw_conv3x3_rgb_f32(const float* x, const float* w, const float* bias, float* y, int batch, int out_ch, int h, int w_,
                       rw_stream_t stream);

/* Its adjoint to the image (rewrite/ganrewrite.py:303-304,316-317): gx (batch, 3, h, w_) = the correlation of
 * g (batch, out_ch, h, w_) -- the gradient at the layer's output, already masked by its ReLU -- with the transposed, tap-flipped
 * weights: gx[b][c][p] = sum_o sum_{ky,kx} w[o][c][ky][kx] g[b][o][py - ky + 1][px - kx + 1], out-channels in ascending
 * order.  w as stored, (out_ch, 3, 3, 3).  Refusals as rw_conv3x3_rgb_f32. */
int rw_conv3x3_rgb_input_grad_f32(const float* g, const float* w, float* gx, int batch, int out_ch, int h, int w_,
                                  rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LPIPS and the masked edit distances (metrics/distances.py:18-59: PerceptualLoss -- models.PerceptualLoss(model='net-lin',
 * net='vgg', spatial=True), sum(loss * w) / sum(w); :96-136: compute_dl).  The VGG16 convolutions are the entries above; these are
 * what follows them.  float32 only, forward only but for the two adjoints at the section's end, on the caller's stream, no atomics, nothing zeroed or drained, every sum in a
 * fixed order: two runs give the same bits.  They join under ABI 11 like the other added entries.
 * ------------------------------------------------------------------------------------- */

/* One tap of LPIPS v0.1 (metrics/distances.py:23-26,51: the lpips(im0, im1) call):
 *   d[b][p] = sum_c lin[c] (f0[b][c][p] / (sqrt(sum_c f0[b][c][p]^2) + 1e-10) - f1[b'][c][p] / (sqrt(sum_c f1[b'][c][p]^2) + 1e-10))^2
 * f0 (batch, ch, hw), f1 (f1_batch, ch, hw) with f1_batch == batch or 1 (b' = 0: broadcast), lin (ch), d (batch, hw).  Any ch >= 1
 * and hw >= 1.  Formed from the normalised difference as written (never from its expansion, which cancels for nearly equal
 * maps); a pixel whose vector is zero in both maps gives 0.  Up to 8192 channels a workgroup stages its run of pixels of both
 * maps in LDS, so that every value is read from memory once; above, the maps are read twice.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null pointer, an extent < 1, f1_batch neither batch nor 1. */
int rw_lpips_tap_f32(const float* f0, const float* f1, const float* lin, float* d, int batch, int f1_batch, int ch,
                     int64_t hw, rw_stream_t stream);

/* Floats of the scratch buffer rw_lpips_combine_f32 (with sums) and rw_masked_l1_rgb_f32 need for `batch` images of hw pixels:
 * one pair per workgroup, stored plainly.  -1: refused (batch < 1, hw < 1 or hw above 256 * 28 * 4096 pixels -- a term of a sum
 * passes through at most 62 additions, metrics/distances.py:53-54's sums over an image are never serial). */
long long rw_lpips_reduce_scratch_elems(int batch, int64_t hw);

/* The tap maps of one LPIPS evaluation: d[k] is (batch, h[k], w[k]). */
#define RW_LPIPS_MAX_TAPS 8
typedef struct rw_lpips_maps {
  const float* d[RW_LPIPS_MAX_TAPS];
  int h[RW_LPIPS_MAX_TAPS];
  int w[RW_LPIPS_MAX_TAPS];
  int n;
} rw_lpips_maps;

/* spatial=True LPIPS and its weighted mean (metrics/distances.py:51-55):
 *   out[b][y][x] = sum_k F.interpolate(d_k, size=(h, w), mode='bilinear', align_corners=False)[b][y][x]
 *   sums[b] = (sum_p out[b][p] weight[b'][p], sum_p weight[b'][p])
 * The per-axis tables come from the host (float64, rounded once): for tap k, idx + k (2h + 2w) holds the rows' first and
 * second index (h each), then the columns' (w each); lam + k (h + w) the rows' weight of the second index, then the
 * columns'.  Indices are clamped into the tap's map.  out (batch, h, w) and sums (batch, 2) are both optional, not both
 * null; weight (weight_batch, h, w), weight_batch == batch or 1, nullable: all ones.  sums needs scratch of
 * rw_lpips_reduce_scratch_elems(batch, h * w) floats.  RW_ERR_BAD_ARGUMENT: null tables, n outside 1 .. RW_LPIPS_MAX_TAPS,
 * a null or empty tap, sums without scratch; RW_ERR_UNSUPPORTED: batch > 65535, an image the reduction refuses. */
int rw_lpips_combine_f32(const rw_lpips_maps* taps, const int* idx, const float* lam, const float* weight, int weight_batch,
                         float* out, float* sums, float* scratch, int batch, int h, int w, rw_stream_t stream);

/* LPIPS as a loss -- the perceptual term of the overfit loop (rewrite/ganrewrite.py:316-317) with the metric of
 * metrics/distances.py:18-59 in place of the feature difference: the adjoints of the two entries above to the FIRST image's
 * side.  The rules of this section hold: float32, fixed summation order, no atomics, nothing zeroed beforehand, the caller's
 * stream, the same bits run to run. */

/* The adjoint of rw_lpips_tap_f32 to f0 (metrics/distances.py:18-59, rewrite/ganrewrite.py:316-317).  With r0 = sqrt(sum_c f0_c^2),
 * den0 = r0 + 1e-10 (r1, den1 likewise of f1), t_c = f0_c / den0 - f1_c / den1 and S = sum_c lin_c t_c f0_c per pixel:
 *   out[b][j][p] = acc[b][j][p] + gd[b][p] (2 / den0) (lin_j t_j - f0_j S / (r0 den0))
 * gd (batch, hw) is the gradient at d; acc (batch, ch, hw) is nullable (zeros) and out may be acc.  relu_mask != 0: an element
 * with f0 <= 0 gets exactly acc (the taps are ReLU outputs).  A pixel with r0 == 0 contributes EXACTLY 0: the formula's
 * derivative there is a 1 / 1e-10 spike and torch's autograd of it returns NaN (sqrt'(0) * 0); inside the module every
 * element of such a pixel is masked by its ReLU.  t_c is formed from the normalised difference, as in the forward.  Domain and
 * tiles as rw_lpips_tap_f32: any ch >= 1 and hw >= 1, f1_batch == batch or 1; up to 8192 channels both maps are read from
 * memory once and out is written once, above that the maps are read three times.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null f0, f1, lin, gd or out, an extent < 1, f1_batch neither batch nor 1. */
int rw_lpips_tap_grad_f32(const float* f0, const float* f1, const float* lin, const float* gd, const float* acc, float* out,
                          int batch, int f1_batch, int ch, int64_t hw, int relu_mask, rw_stream_t stream);

/* The gradients at the tap maps: d[k] (batch, h[k], w[k]) is WRITTEN. */
typedef struct rw_lpips_grad_maps {
  float* d[RW_LPIPS_MAX_TAPS];
  int h[RW_LPIPS_MAX_TAPS];
  int w[RW_LPIPS_MAX_TAPS];
  int n;
} rw_lpips_grad_maps;

/* The adjoint of rw_lpips_combine_f32's weighted sum to every tap map (metrics/distances.py:18-59, rewrite/ganrewrite.py:316-317):
 *   d[k][b][i][j] = gscale[b] sum_{oy in R_y(i)} wy(oy, i) sum_{ox in R_x(j)} wx(ox, j) weight[b'][oy][ox]
 * w(o, i) = (1 - lam_o) [i0_o == i] + lam_o [i1_o == i] from idx and lam, the forward's tables; R(i) = [lo, hi) is the run of
 * outputs that touch input i, from rng: tap after tap, the rows' lo (h[k]), the rows' hi (h[k]), the columns' lo (w[k]), the
 * columns' hi (w[k]) -- 2 sum_k (h[k] + w[k]) ints.  Indices and ranges are clamped: a wrong table gives a wrong picture, never
 * an access outside a map.  A row's columns are summed first, then the rows.  weight (weight_batch, h, w) is nullable: all
 * ones; gscale (batch) is the upstream gradient of an image's mean over its sum of weights.  Identity tables at a tap's own
 * size give the adjoint of spatial=False's mean.
 * RW_ERR_BAD_ARGUMENT (nothing launched): null grads, tables, rng or gscale, n outside 1 .. RW_LPIPS_MAX_TAPS, a null or empty
 * map, an extent < 1, weight_batch neither batch nor 1; RW_ERR_UNSUPPORTED: batch > 65535. */
int rw_lpips_combine_grad_f32(const rw_lpips_grad_maps* grads, const int* idx, const float* lam, const int* rng,
                              const float* weight, int weight_batch, const float* gscale, int batch, int h, int w,
                              rw_stream_t stream);

/* compute_dl's pixel mode (metrics/distances.py:131-133): sums[b] = (sum_p mask[b'][p] sum_c |a[b][c][p] - b[b][c][p]|, sum_p mask[b'][p])
 * for a, b (batch, 3, hw) and mask (mask_batch, hw) float32, mask_batch == batch or 1.  scratch as above. */
int rw_masked_l1_rgb_f32(const float* a, const float* b, const float* mask, int mask_batch, float* sums, float* scratch,
                         int batch, int64_t hw, rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Generator forward in float64 -- the reference's generator runs after .double(): its two native ops dispatch double
 * (above) and everything else is torch.  These entries are the double forms of that torch arithmetic: every pointer is a
 * DEVICE pointer to contiguous float64, every scalar a double, every product and accumulation is in double.  The _f64
 * twins take the arguments of their _f32 entries (the glue ops are the same kernel bodies, instantiated for double).
 * Forward only, one module per launch.
 * ------------------------------------------------------------------------------------- */

/* PixelNormL: y = x * rsqrt(mean(x^2, dim=1) + eps)      (models.py:609-614) */
int rw_pixel_norm_f64(const double* x, double* y, int batch, int dim, double eps, rw_stream_t stream);

/* EqualLinear.forward (models.py:503-511), as rw_equal_linear_f32; any in_dim. */
int rw_equal_linear_f64(const double* x, const double* w, const double* bias, double* y,
                        int batch, int in_dim, int out_dim, int64_t x_stride,
                        double w_scale, double b_scale, int act, double alpha, double act_scale,
                        rw_stream_t stream);

/* AdjustLatent (models.py:570-583), as rw_adjust_latent_f32; avg nullable. */
int rw_adjust_latent_f64(const double* w, const double* avg, double* out, int batch, int n_latent,
                         int dim, double psi, rw_stream_t stream);

/* ApplyStyle (models.py:616-620): y[b][c][p] = style[b][c] * x[b][c][p]. */
int rw_style_mul_f64(const double* x, const double* style, double* y, int batch, int channels,
                     int64_t hw, rw_stream_t stream);

/* wsq[o][i] = sum_{ky,kx} (w_scale * W[o][i][ky][kx])^2 and demod[b][o] = rsqrt(sum_i style[b][i]^2 * wsq[o][i] + eps)
 * -- the demodulation factor of DemodulatedConv2dF.forward (models.py:320-328). */
int rw_weight_sqsum_f64(const double* w, double* wsq, int out_ch, int in_ch, int taps, double w_scale,
                        rw_stream_t stream);
int rw_demod_f64(const double* wsq, const double* style, double* demod, int batch, int out_ch,
                 int in_ch, double eps, rw_stream_t stream);

/* F.conv2d(x * style, w_scale * W, padding=1) * demod                    (models.py:318-319,328)
 * F.conv_transpose2d(x * style, w_scale * W^T, stride=2) * demod         (models.py:315-316,328)
 * x (B,Cin,H,W) -> y (B,Cout,H,W) / (B,Cout,2H+1,2W+1).  w is the parameter AS STORED, (out_ch, in_ch, 3, 3): nothing is
 * packed.  style (B,Cin) nullable: multiplied into x while it is loaded (ApplyStyle, models.py:616-620); demod (B,Cout)
 * nullable.  No noise / bias / activation epilogue and no impl argument: the double path runs module by module.
 * Every shape is taken: in_ch % 4 == 0 and out_ch % 16 == 0 run as an implicit GEMM on v_mfma_f64_16x16x4_f64 (the input
 * window staged in LDS, edges masked), any other shape as one thread per output element.  RW_ERR_UNSUPPORTED where one
 * image's input or output maps, or the weight, have 2^31 elements or more. */
int rw_conv3x3_f64(const double* x, const double* w, double* y, int batch, int in_ch, int out_ch,
                   int h, int w_in, double w_scale, const double* style, const double* demod,
                   rw_stream_t stream);
int rw_conv_transpose3x3s2_f64(const double* x, const double* w, double* y, int batch, int in_ch,
                               int out_ch, int h, int w_in, double w_scale, const double* style,
                               const double* demod, rw_stream_t stream);

/* NoiseInjectionF (models.py:535-546): y[b][c][p] = x[b][c][p] + noise_w[0] * noise[b][p]; the reference's float32 noise
 * rows are widened by the caller (torch's promotion, models.py:539-546). */
int rw_noise_add_f64(const double* x, const double* noise, const double* noise_w, double* y,
                     int batch, int channels, int64_t hw, rw_stream_t stream);

/* ToRGBF (models.py:628-655), as rw_to_rgb_f32; in_ch <= 2048. */
int rw_to_rgb_f64(const double* x, const double* w, const double* style, const double* bias,
                  const double* skip, double* y, int batch, int in_ch, int64_t hw, double w_scale,
                  rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The Frechet distance on the device -- replaces numpy.cov's consumers and scipy.linalg.sqrtm in
 * calculate_frechet_distance (metrics/fid.py:60-61,137-187):
 *   d^2 = |mu1 - mu2|^2 + Tr S1 + Tr S2 - 2 Tr sqrt(S1 S2),   Tr sqrt(S1 S2) = sum_i sqrt(mu_i(F^T S2 F)),  S1 = F F^T,
 * an eigenvalue problem of two symmetric PSD matrices, solved by a float64 block one-sided (Hestenes) Jacobi iteration.
 * Every pointer is a DEVICE pointer to contiguous float64 unless stated.  The entries are added at ABI 11 as the PNG and
 * resize entries were: an entry that is only added changes no existing call.
 *
 * The working arrays g and v are n x n, row-major, ROW j holding COLUMN j of G and of V: g starts as the symmetric
 * matrix S (zero-padded to n, a multiple of the block width and at least two blocks), v as the identity; at convergence
 * the column norms of G = S V are the eigenvalues and V the eigenvectors.
 *
 * Rotation rule, stated once.  Columns x, y with squared norms a, b and inner product gamma are rotated when
 *   |gamma| > RW_JACOBI_TOL(n) sqrt(a) sqrt(b)      and      max(a, b) > RW_JACOBI_FLOOR(n)^2 max_j |column j of S|^2.
 * TOL: a computed inner product of n terms differs from the exact one by at most n eps |x| |y| (eps = 2^-52), so a cosine
 * below n eps is not known to differ from zero, and a rotation by it would be repeated for ever.  sqrt(a) sqrt(b) is
 * formed, not sqrt(a b): the product of two squared norms overflows for large inputs.  FLOOR: a column that is zero in exact
 * arithmetic (a rank-deficient S) carries the rounding of the rotations that emptied it, n eps of the largest column at
 * most per sweep; two such columns have a cosine of order one and would rotate for ever, and their norms are below what
 * the input determines (the eigenvalue they stand for is known to n eps lambda_max only).  The largest column of the
 * INPUT is the reference: it lies within sqrt(n) of lambda_max and needs no reduction during the iteration.
 * ------------------------------------------------------------------------------------- */
#define RW_JACOBI_TOL(n)   ((double)(n) * 0x1p-52)
#define RW_JACOBI_FLOOR(n) ((double)(n) * 0x1p-52)

/* One step (one launch) of a sweep: workgroup k takes the block pair k of round `step` of the circle method over the
 * n / block column blocks (rounded up to even; blocks - 1 steps make a sweep in which every block meets every other once,
 * the block that meets the dummy of an odd count has a bye), forms the Gram matrix of its 2 block columns on
 * v_mfma_f64_16x16x4_f64, diagonalises it in LDS (bounded cyclic two-sided Jacobi, rotations accumulated from the identity,
 * columns then ordered by decreasing norm) and applies the factor to its columns of g and, if v is not NULL, of v.
 * block is 8 or 16.  norms_sq (n): rw_colnorm_f64(mode 1) of the INPUT, the same for every step.  slots: m / 2 ints for
 * THIS step, m = blocks rounded up to even; workgroup k stores its rotation count to slots[k] with a plain store (0 for a
 * bye), or -1 if its columns hold a non-finite value -- it then changes nothing.  No atomics; no workgroup waits for
 * another.  RW_ERR_BAD_ARGUMENT: a null g, norms_sq or slots, block not 8 or 16, n < 2 block or no multiple of it, step
 * outside 0 .. m - 2; RW_ERR_UNSUPPORTED: g or v not 32-byte aligned. */
int rw_jacobi_step_f64(double* g, double* v, int n, int block, int step, const double* norms_sq, int* slots,
                       rw_stream_t stream);

/* The slots of a sweep reduced: out[0] = the sum of the counts, out[1] = how many slots say non-finite (out: two 64-bit
 * integers on the device).  What the host reads once per sweep. */
int rw_jacobi_count_i32(const int* slots, int64_t nslots, long long* out, rw_stream_t stream);

/* out[j] = the norm of row j of g (n x n) -- column j of G, the eigenvalue at convergence (mode 0); its square (mode 1);
 * its square root (mode 2: the scale of F = V diag(sqrt(lambda))).  One wave per row, a fixed order of the sum. */
int rw_colnorm_f64(const double* g, double* out, int n, int mode, rw_stream_t stream);

/* C (m x n) = diag(row_scale) op(A) op(B) diag(col_scale), all row-major: op(A) is m x k (trans_a: A is stored k x m),
 * op(B) is k x n (trans_b: B is stored n x k); row_scale (m) and col_scale (n) nullable.  v_mfma_f64_16x16x4_f64, no split
 * of k: the same bits from run to run.  It forms T = diag(sqrt(lambda)) V^T S2 and B = T V diag(sqrt(lambda)).  C must not
 * alias A or B. */
int rw_gemm_f64(const double* a, const double* b, double* c, int m, int n, int k, int trans_a, int trans_b,
                const double* row_scale, const double* col_scale, rw_stream_t stream);

/* out[0 .. 4] = { d^2, |mu1 - mu2|^2, Tr S1, Tr S2, sum_i sqrt(max(ev[i], 0)) } with
 * d^2 = ((|mu1 - mu2|^2 + Tr S1) + Tr S2) - 2 sum sqrt(ev) (the order of metrics/fid.py:186-187); mu (n), S (n x n), ev (n_ev).
 * One workgroup, every sum in a fixed order. */
int rw_frechet_finish_f64(const double* mu1, const double* mu2, const double* s1, const double* s2, const double* ev,
                          int n, int n_ev, double* out, rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The Inception-v3 pool3 features of the FID row (metrics/fid.py:67-84,90-131: the activations of pool_3 that
 * calculate_activation_statistics, :40-62, reduces; :190-193: the images clamped on their way in).  rewriting_amd/inception.py
 * walks the network over these four entries.  float32, NCHW, contiguous, on the caller's stream; no atomics, no memsets,
 * every sum in a fixed order: two runs give the same bits.  A shape an entry does not take is refused before any launch,
 * never clamped.  They join at ABI 11 like the entries before them: added only, no existing call changes.
 * ------------------------------------------------------------------------------------- */

/* Floats of the packed form of a (out_ch, in_ch, kh, kw) weight: K = in_ch kh kw rounded up to 16 times out_ch rounded up to
 * 64; 0 for a shape the convolution refuses (kh or kw outside 1 .. 7, an extent < 1). */
long long rw_conv2d_packed_weight_elems(int out_ch, int in_ch, int kh, int kw);

/* wp[k][m] = weight[m][k], k = (channel, tap row, tap column) as stored, zero in the padding: what rw_conv2d_f32 reads
 * with 16-byte loads and no bound.  Once per weight version (the batch-norm fold of metrics/fid.py:31-37's frozen graph is
 * the host's, before this). */
int rw_pack_conv2d_weight_f32(const float* weight, float* wp, int out_ch, int in_ch, int kh, int kw, rw_stream_t stream);

/* y[:, c_off : c_off + out_ch] = act(conv2d(x, weight, stride, padding (ph, pw)) + bias) for x (batch, in_ch, h, w) and y
 * (batch, c_total, oh, ow), oh = (h + 2 ph - kh) / stride + 1: the convolutions of the pool_3 graph (metrics/fid.py:67-84),
 * whose blocks concatenate by writing their slice.  wp from rw_pack_conv2d_weight_f32, 16-byte aligned; bias (out_ch)
 * nullable; relu 0 / 1.  An implicit GEMM over K = in_ch kh kw on v_mfma_f32_32x32x2_f32 -- exact f32 products, chains of
 * 64 products from zero added to the total in ascending k; ragged out_ch, positions and K are masked, a tap outside the
 * map is an exact zero and reads nothing.  The other channels of y are not touched.  y must not overlap x.
 * RW_ERR_BAD_ARGUMENT (nothing launched): a null x / wp / y, an extent < 1, a slice outside 0 .. c_total.
 * RW_ERR_UNSUPPORTED (nothing launched): kh or kw > 7, a stride outside {1, 2}, ph >= kh or pw >= kw or negative, a map
 * smaller than the kernel, wp not 16-byte aligned, batch oh ow or h w above 2^30, out_ch above 64 x 65535. */
int rw_conv2d_f32(const float* x, const float* wp, const float* bias, float* y, int batch, int in_ch, int h, int w,
                  int out_ch, int kh, int kw, int stride, int ph, int pw, int relu, int c_off, int c_total,
                  rw_stream_t stream);

/* The 3 x 3 poolings of the pool_3 graph (metrics/fid.py:67-84) into y[:, c_off : c_off + ch] of (batch, c_total, oh, ow).
 * mode 0: max, stride 2, no padding, oh = (h - 3) / 2 + 1 (RW_ERR_UNSUPPORTED for h or w < 3); mode 1: average, stride 1,
 * pad 1, divided by the number of taps inside the map (count_include_pad=False, the FID graph's variant); mode 2: max,
 * stride 1, pad 1.  A padded tap is never looked at: an all-negative window stays negative.  Taps in ascending (row,
 * column) order. */
int rw_pool3x3_f32(const float* x, float* y, int batch, int ch, int h, int w, int mode, int c_off, int c_total,
                   rw_stream_t stream);

/* y (batch, ch) = the mean of every h x w map of x: pool_3 itself (metrics/fid.py:69-70).  One wave per map, lane l sums the
 * elements l, l + 64, ... and the lanes are added by a fixed butterfly, in double, rounded once.  RW_ERR_UNSUPPORTED: h w
 * above 2^24. */
int rw_global_avgpool_f32(const float* x, float* y, int batch, int ch, int h, int w, rw_stream_t stream);

/* y (batch, 3, out_h, out_w) = the network's input from images: float (batch, 3, in_h, in_w) clamped to [-1, 1]
 * (metrics/fid.py:190-193, pt_to_np) when is_bytes == 0, bytes (batch, in_h, in_w, 3) mapped by x / 127.5 - 1 otherwise (what
 * rw_render_bytes_f32 and rw_png_unfilter_u8 leave).  Resized with the arithmetic of F.interpolate(mode='bilinear',
 * align_corners=False): source coordinate (d + 0.5) in / out - 0.5 clamped at 0, no antialiasing -- NOT the Pillow tables of
 * rw_resize_bilinear_u8.  An image of the output's size passes through with the same bits. */
int rw_inception_input_f32(const void* images, float* y, int batch, int in_h, int in_w, int out_h, int out_w, int is_bytes,
                           rw_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The face-parsing BiSeNet of the edit-distance rows for faces (metrics/load_seg.py:11-35 FaceSegementer.segment_batch;
 * metrics/face-parsing.PyTorch/model.py, resnet.py) and the "pixels correctly modified" count of
 * metrics/seg_correct_mod.py:40-65.  rewriting_amd/faceparse.py walks the network over rw_conv2d_f32, rw_global_avgpool_f32
 * and these entries.  float32, NCHW, contiguous, on the caller's stream; no atomics, no memsets, every sum in a fixed order:
 * two runs give the same bits.  A shape an entry does not take is refused before any launch, never clamped; an INDEX read
 * from a table is clamped into the map it addresses, so that a wrong table gives a wrong picture and never a read outside
 * it.  They join at ABI 11 like the entries before them: added only, no existing call changes.
 * ------------------------------------------------------------------------------------- */

/* y = act((conv2d(x) + bias) + res) with res and y (batch, out_ch, oh, ow): the tail of a BasicBlock (resnet.py:36-48).
 * rw_conv2d_f32's kernel, sums and refusals (its c_off = 0, c_total = out_ch); the sum in k, then + bias, then + res, then
 * the ReLU.  y may be res itself (every element is read and then written by the same thread); y must not overlap x.
 * RW_ERR_BAD_ARGUMENT: a null res (rw_conv2d_f32 is the form without one). */
int rw_conv2d_add_f32(const float* x, const float* wp, const float* bias, const float* res, float* y, int batch, int in_ch,
                      int h, int w, int out_ch, int kh, int kw, int stride, int ph, int pw, int relu, rw_stream_t stream);

/* y (batch, ch, oh, ow) = F.max_pool2d(x, 3, 2, 1), oh = (h - 1) / 2 + 1: the pooling of the ResNet stem (resnet.py:64,74),
 * any h, w >= 1.  A padded tap is never looked at: an all-negative window stays negative.  RW_ERR_UNSUPPORTED: h or w above
 * 2^20. */
int rw_maxpool3x3s2p1_f32(const float* x, float* y, int batch, int ch, int h, int w, rw_stream_t stream);

/* y[b, c, oy, ox] = x[b, c, r, q] s + a with r = row[oy], q = col[ox]: every element-wise step of the context path and the
 * fusion module (model.py:76-83 the gate of an attention-refinement module, :111-122 its sum with the pooled vector or the
 * coarser map and the nearest-neighbour step to the next size, :203-209 feat atten + feat) and the image's nearest-neighbour
 * resize to the working size (load_seg.py:27).  x (batch, ch, h, w), y (batch, ch, oh, ow).
 *   row (oh), col (ow): int32 nearest-neighbour tables made by the host; a null table keeps that axis' index and needs
 *     oh == h (ow == w).  Entries are clamped into the map.
 *   s = 1 / (1 + expf(-gate[b, c])), gate (batch, ch); a null gate: no multiply at all.
 *   a = add_map[b, c, r, q] (a map of x's size; it may be x) or add_vec[b, c] or, both null, nothing.
 * The product is rounded, then the sum (torch's mul followed by add; no fused multiply-add).  With gate and both adds null it
 * is a gather and equals F.interpolate(x, size) of float32 bit for bit.  Columns that keep their index, w a multiple of 4 and
 * 16-byte aligned pointers take 16-byte accesses.  y must not overlap x or add_map.
 * RW_ERR_BAD_ARGUMENT: add_map and add_vec both given; a null table on an axis that changes its size.
 * RW_ERR_UNSUPPORTED: a side above 2^20, a map above 2^30 elements, batch ch above 2^31 - 1. */
int rw_gate_resample_f32(const float* x, const float* gate, const float* add_map, const float* add_vec, const int* row,
                         const int* col, float* y, int batch, int ch, int h, int w, int oh, int ow, rw_stream_t stream);

/* y (batch, ch, oh, ow) = F.interpolate(x, (oh, ow), mode='bilinear', align_corners=True) (model.py:251).  idx int32
 * (2 oh + 2 ow): the rows' i0, the rows' i1, the columns' i0, the columns' i1; lam float32 (oh + ow): the rows', the
 * columns' -- made by the host (faceparse.align_corners_table), laid out as rw_lpips_combine_f32 reads its own.  The value is
 * (1 - lr) ((1 - lc) v00 + lc v01) + lr ((1 - lc) v10 + lc v11), every product and sum rounded on its own.  A map of the
 * output's size passes through bit for bit. */
int rw_bilinear_ac_f32(const float* x, float* y, int batch, int ch, int h, int w, int oh, int ow, const int* idx,
                       const float* lam, rw_stream_t stream);

/* labels (batch, 1, OH, OW) int64: at each pixel the lowest class index that attains the maximum of the n samples
 * rw_bilinear_ac_f32 would take of logits (batch, n, h, w) at the working-size pixel (pick_row[oy], pick_col[ox]) of its
 * (H, W) output -- the argmax(0) of load_seg.py:30-31 followed by the nearest-neighbour F.interpolate(masks, og_size).long()
 * of :33-34, without the (n, H, W) scores in memory; the same device function forms the sample, so the labels equal the
 * arg-max of that entry's output bit for bit.  idx, lam: that entry's tables for (h, w) -> (H, W); pick_row (OH), pick_col
 * (OW): int32 nearest tables, a null one needs OH == H (OW == W).  A NaN wins, the first one first, as in numpy.argmax.
 * RW_ERR_UNSUPPORTED: n above 64. */
int rw_seg_labels_i64(const float* logits, long long* labels, int batch, int n, int h, int w, int H, int W, const int* idx,
                      const float* lam, const int* pick_row, const int* pick_col, int OH, int OW, rw_stream_t stream);

/* out (batch, 2) int64 = (total, count) of seg_correct_mod.py:51-62 per image: count = the pixels whose `before` label is one
 * of src, total = those of them whose `after` label is one of tgt.  before, after: int64 device maps of hw labels per image,
 * image b at before + b before_stride (elements) -- a channel of a (B, C, H, W) tensor without a copy.  src (n_src), tgt
 * (n_tgt): HOST arrays of 1 .. 16 int64 labels each, copied into the launch.  One workgroup per image, integer sums.
 * RW_ERR_BAD_ARGUMENT: a null pointer, an empty set, a stride below hw.  RW_ERR_UNSUPPORTED: a set above 16 labels. */
int rw_seg_correct_counts_i64(const long long* before, const long long* after, int batch, long long hw,
                              long long before_stride, long long after_stride, const long long* src, int n_src,
                              const long long* tgt, int n_tgt, long long* out, rw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* REWRITING_HIP_H */
