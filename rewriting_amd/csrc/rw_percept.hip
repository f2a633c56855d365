// The perceptual network of the overfit loss: VF = torchvision's vgg16().features up to layer 20 (rewrite/ganrewrite.py:303-304),
// used as 1e-2 * mse(VF(gt), VF(pred)) (:316-317).  Nine stride-1 3x3 convolutions, each followed by a bias and a ReLU, three
// of them also by a 2x2 max-pool; the network is frozen, so the only adjoint is the one to the input.  The eight convolutions
// with 64 .. 512 channels are the plain forms of rw_wino.hip / rw_conv.hip (w_scale 1, no epilogue); this file adds what those
// do not have:
//
//   bias_relu_pool        y = max(x + bias[c], 0) and, optionally, its 2x2 / stride-2 maximum, in ONE streaming pass
//   bias_relu_pool_grad   the adjoint of that w.r.t. x from the saved y: it only ROUTES values (first maximum of a window in
//                         row-major order, torch's tie rule)
//   conv3x3_rgb           the first layer, 3 -> out_ch channels (27 taps per output, store-bound), bias + ReLU fused
//   conv3x3_rgb_input_grad   its adjoint to the image, out_ch -> 3 channels (9 out_ch terms per output, read-bound)
//
// float32 only, one form per kernel (nothing here is a template over the element type).  Every sum runs in a fixed order, no
// atomics, nothing zeroed beforehand, nothing but launches on the caller's stream: two runs give the same bits.
#include "rw_common.h"

__device__ __forceinline__ float pc_relu(float v) { return v > 0.f ? v : 0.f; }

// ---------------------------------------------------------------------------------------
// bias + ReLU (+ max-pool).  A work item is a block of two rows of one plane: V4 -- four columns of each (16-byte accesses;
// w % 4 == 0 and 16-byte aligned pointers), else two columns (any w, any alignment).  The item reads its values before it
// writes any and no other item reads them, so y may be x.  An odd last row / column is activated and stored like the rest
// and belongs to no pooling window (nn.MaxPool2d(2, 2): floor).
// ---------------------------------------------------------------------------------------
template <bool V4>
__global__ void __launch_bounds__(256) percept_act_pool_kernel(const float* x, const float* __restrict__ bias, float* y,
                                                               float* __restrict__ pooled, int ch, int h, int w, int64_t items) {
  const int rp = (h + 1) >> 1, cq = V4 ? (w >> 2) : ((w + 1) >> 1);
  const int oh = h >> 1, ow = w >> 1;
  const int64_t hw = (int64_t)h * w;
  for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < items; item += (int64_t)gridDim.x * 256) {
    const int q = (int)(item % cq);
    const int64_t t = item / cq;
    const int r = (int)(t % rp);
    const int64_t plane = t / rp;
    const float bv = bias ? bias[plane % ch] : 0.f;
    const int r0 = 2 * r;
    const bool has1 = r0 + 1 < h;
    const int64_t at = plane * hw + (int64_t)r0 * w;
    if (V4) {
      float4 a = *reinterpret_cast<const float4*>(x + at + 4 * q);
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has1) b = *reinterpret_cast<const float4*>(x + at + w + 4 * q);
      a.x = pc_relu(a.x + bv); a.y = pc_relu(a.y + bv); a.z = pc_relu(a.z + bv); a.w = pc_relu(a.w + bv);
      b.x = pc_relu(b.x + bv); b.y = pc_relu(b.y + bv); b.z = pc_relu(b.z + bv); b.w = pc_relu(b.w + bv);
      if (y) {
        *reinterpret_cast<float4*>(y + at + 4 * q) = a;
        if (has1) *reinterpret_cast<float4*>(y + at + w + 4 * q) = b;
      }
      if (pooled && has1) {
        float2 m;
        m.x = fmaxf(fmaxf(a.x, a.y), fmaxf(b.x, b.y));
        m.y = fmaxf(fmaxf(a.z, a.w), fmaxf(b.z, b.w));
        *reinterpret_cast<float2*>(pooled + plane * ((int64_t)oh * ow) + (int64_t)r * ow + 2 * q) = m;
      }
    } else {
      const int c0 = 2 * q;
      const bool hasc = c0 + 1 < w;
      const float v00 = pc_relu(x[at + c0] + bv);
      const float v01 = hasc ? pc_relu(x[at + c0 + 1] + bv) : 0.f;
      const float v10 = has1 ? pc_relu(x[at + w + c0] + bv) : 0.f;
      const float v11 = (has1 && hasc) ? pc_relu(x[at + w + c0 + 1] + bv) : 0.f;
      if (y) {
        y[at + c0] = v00;
        if (hasc) y[at + c0 + 1] = v01;
        if (has1) y[at + w + c0] = v10;
        if (has1 && hasc) y[at + w + c0 + 1] = v11;
      }
      if (pooled && has1 && hasc)
        pooled[plane * ((int64_t)oh * ow) + (int64_t)r * ow + q] = fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
    }
  }
}

extern "C" int rw_bias_relu_pool_f32(const float* x, const float* bias, float* y, float* pooled, int batch, int ch, int h,
                                     int w, rw_stream_t stream) {
  RW_CHECK_ARG(x && bias && (y || pooled) && batch > 0 && ch > 0 && h > 0 && w > 0);
  const bool v4 = w % 4 == 0 && rw_aligned16(x) && rw_aligned16(y) && rw_aligned16(pooled);
  const int64_t items = (int64_t)batch * ch * ((h + 1) / 2) * (v4 ? w / 4 : (w + 1) / 2);
  const dim3 grid((unsigned)rw_stream_grid(items, 256));
  if (v4)
    hipLaunchKernelGGL(percept_act_pool_kernel<true>, grid, dim3(256), 0, rw_s(stream), x, bias, y, pooled, ch, h, w, items);
  else
    hipLaunchKernelGGL(percept_act_pool_kernel<false>, grid, dim3(256), 0, rw_s(stream), x, bias, y, pooled, ch, h, w, items);
  return RW_LAUNCH_RESULT();
}

// The adjoint.  Not pooled: gx = y > 0 ? g : 0.  Pooled: g has the pooled size, and of the four positions of a window the
// FIRST maximum of y in row-major order (strict comparisons, as torch's max_pool2d picks its index) receives the window's
// gradient if its y is positive; everything else, and the odd last row / column, receives 0.
__device__ __forceinline__ int pc_first_max(float v00, float v01, float v10, float v11) {
  int k = 0;
  float m = v00;
  if (v01 > m) { m = v01; k = 1; }
  if (v10 > m) { m = v10; k = 2; }
  if (v11 > m) { m = v11; k = 3; }
  return m > 0.f ? k : -1;
}

template <bool V4>
__global__ void __launch_bounds__(256) percept_act_pool_grad_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                                    float* __restrict__ gx, int h, int w, int pooled,
                                                                    int64_t items) {
  const int rp = (h + 1) >> 1, cq = V4 ? (w >> 2) : ((w + 1) >> 1);
  const int oh = h >> 1, ow = w >> 1;
  const int64_t hw = (int64_t)h * w;
  for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < items; item += (int64_t)gridDim.x * 256) {
    const int q = (int)(item % cq);
    const int64_t t = item / cq;
    const int r = (int)(t % rp);
    const int64_t plane = t / rp;
    const int r0 = 2 * r;
    const bool has1 = r0 + 1 < h;
    const int64_t at = plane * hw + (int64_t)r0 * w;
    if (V4) {
      const float4 a = *reinterpret_cast<const float4*>(y + at + 4 * q);
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has1) b = *reinterpret_cast<const float4*>(y + at + w + 4 * q);
      float4 ga = make_float4(0.f, 0.f, 0.f, 0.f), gb = ga;
      if (!pooled) {
        const float4 ta = *reinterpret_cast<const float4*>(g + at + 4 * q);
        ga.x = a.x > 0.f ? ta.x : 0.f; ga.y = a.y > 0.f ? ta.y : 0.f; ga.z = a.z > 0.f ? ta.z : 0.f; ga.w = a.w > 0.f ? ta.w : 0.f;
        if (has1) {
          const float4 tb = *reinterpret_cast<const float4*>(g + at + w + 4 * q);
          gb.x = b.x > 0.f ? tb.x : 0.f; gb.y = b.y > 0.f ? tb.y : 0.f; gb.z = b.z > 0.f ? tb.z : 0.f; gb.w = b.w > 0.f ? tb.w : 0.f;
        }
      } else if (has1) {
        const float2 gw = *reinterpret_cast<const float2*>(g + plane * ((int64_t)oh * ow) + (int64_t)r * ow + 2 * q);
        const int k0 = pc_first_max(a.x, a.y, b.x, b.y), k1 = pc_first_max(a.z, a.w, b.z, b.w);
        ga.x = k0 == 0 ? gw.x : 0.f; ga.y = k0 == 1 ? gw.x : 0.f; gb.x = k0 == 2 ? gw.x : 0.f; gb.y = k0 == 3 ? gw.x : 0.f;
        ga.z = k1 == 0 ? gw.y : 0.f; ga.w = k1 == 1 ? gw.y : 0.f; gb.z = k1 == 2 ? gw.y : 0.f; gb.w = k1 == 3 ? gw.y : 0.f;
      }
      *reinterpret_cast<float4*>(gx + at + 4 * q) = ga;
      if (has1) *reinterpret_cast<float4*>(gx + at + w + 4 * q) = gb;
    } else {
      const int c0 = 2 * q;
      const bool hasc = c0 + 1 < w;
      float o00 = 0.f, o01 = 0.f, o10 = 0.f, o11 = 0.f;
      if (!pooled) {
        o00 = y[at + c0] > 0.f ? g[at + c0] : 0.f;
        if (hasc) o01 = y[at + c0 + 1] > 0.f ? g[at + c0 + 1] : 0.f;
        if (has1) o10 = y[at + w + c0] > 0.f ? g[at + w + c0] : 0.f;
        if (has1 && hasc) o11 = y[at + w + c0 + 1] > 0.f ? g[at + w + c0 + 1] : 0.f;
      } else if (has1 && hasc) {
        const float gw = g[plane * ((int64_t)oh * ow) + (int64_t)r * ow + q];
        const int k = pc_first_max(y[at + c0], y[at + c0 + 1], y[at + w + c0], y[at + w + c0 + 1]);
        o00 = k == 0 ? gw : 0.f; o01 = k == 1 ? gw : 0.f; o10 = k == 2 ? gw : 0.f; o11 = k == 3 ? gw : 0.f;
      }
      gx[at + c0] = o00;
      if (hasc) gx[at + c0 + 1] = o01;
      if (has1) gx[at + w + c0] = o10;
      if (has1 && hasc) gx[at + w + c0 + 1] = o11;
    }
  }
}

extern "C" int rw_bias_relu_pool_grad_f32(const float* g, const float* y, float* gx, int batch, int ch, int h, int w,
                                          int pooled, rw_stream_t stream) {
  RW_CHECK_ARG(g && y && gx && batch > 0 && ch > 0 && h > 0 && w > 0 && (pooled == 0 || pooled == 1));
  RW_CHECK_ARG(g != gx && y != gx);
  const bool v4 = w % 4 == 0 && rw_aligned16(g) && rw_aligned16(y) && rw_aligned16(gx);
  const int64_t items = (int64_t)batch * ch * ((h + 1) / 2) * (v4 ? w / 4 : (w + 1) / 2);
  const dim3 grid((unsigned)rw_stream_grid(items, 256));
  if (v4)
    hipLaunchKernelGGL(percept_act_pool_grad_kernel<true>, grid, dim3(256), 0, rw_s(stream), g, y, gx, h, w, pooled, items);
  else
    hipLaunchKernelGGL(percept_act_pool_grad_kernel<false>, grid, dim3(256), 0, rw_s(stream), g, y, gx, h, w, pooled, items);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// The first layer and its adjoint.  A workgroup owns a PC_TH x PC_TW pixel tile of one image for ALL out-channels; a thread
// owns four consecutive pixels of a row (one 16-byte access where w % 4 == 0 and the pointer is aligned).  The weights of all
// out-channels sit in LDS as [o][28] (27 taps and the bias: seven 16-byte broadcast reads per out-channel), the input
// window with its halo of one pixel at row pitch PC_XW (a multiple of 4: a thread's six columns are a 16- and an 8-byte
// read); positions outside the image are zeros (padding = 1).
// ---------------------------------------------------------------------------------------
#define PC_TW 64
#define PC_TH 16
#define PC_XH (PC_TH + 2)
#define PC_XUSED (PC_TW + 2)
#define PC_XW 68
#define PC_MAX_OUT 64
#define PC_SLOTS ((PC_XH * PC_XUSED + 255) / 256)

__device__ __forceinline__ void pc_stage_weights(float (*ws)[28], const float* __restrict__ wt, const float* __restrict__ bias,
                                                 int out_ch) {
  for (int t = threadIdx.x; t < out_ch * 28; t += 256) {
    const int o = t / 28, k = t - 28 * o;
    ws[o][k] = k < 27 ? wt[o * 27 + k] : (bias ? bias[o] : 0.f);
  }
}

// y[b][o][p] = max(bias[o] + sum_{c, ky, kx} w[o][c][ky][kx] x[b][c][py + ky - 1][px + kx - 1], 0): 27 multiply-adds in
// the order (c, ky, kx), then the bias
__global__ void __launch_bounds__(256) percept_conv_rgb_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                               const float* __restrict__ bias, float* __restrict__ y,
                                                               int out_ch, int h, int w, int tiles_x, int vec) {
  __shared__ float xs[3][PC_XH][PC_XW];
  __shared__ __attribute__((aligned(16))) float ws[PC_MAX_OUT][28];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, b = blockIdx.y;
  const int y0 = ty * PC_TH, x0 = tx * PC_TW;
  const int64_t hw = (int64_t)h * w;
  pc_stage_weights(ws, wt, bias, out_ch);
  const float* xb = x + (int64_t)b * 3 * hw;
  for (int t = threadIdx.x; t < 3 * PC_XH * PC_XUSED; t += 256) {
    const int c = t / (PC_XH * PC_XUSED), rem = t - c * (PC_XH * PC_XUSED);
    const int r = rem / PC_XUSED, cc = rem - r * PC_XUSED;
    const int iy = y0 - 1 + r, ix = x0 - 1 + cc;
    const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < w;
    xs[c][r][cc] = ok ? xb[c * hw + (int64_t)iy * w + ix] : 0.f;
  }
  __syncthreads();
  const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
  const int oy = y0 + r, ox = x0 + c4;
  if (oy >= h || ox >= w) return;
  float in[3][3][6];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int j = 0; j < 6; ++j) in[c][ky][j] = xs[c][r + ky][c4 + j];
  float* yb = y + (int64_t)b * out_ch * hw + (int64_t)oy * w + ox;
  for (int o = 0; o < out_ch; ++o) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float wv = ws[o][c * 9 + ky * 3 + kx];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(wv, in[c][ky][kx + j], acc[j]);
        }
    const float bv = ws[o][27];
    float4 v;
    v.x = pc_relu(acc[0] + bv); v.y = pc_relu(acc[1] + bv); v.z = pc_relu(acc[2] + bv); v.w = pc_relu(acc[3] + bv);
    float* yo = yb + (int64_t)o * hw;
    if (vec) {
      *reinterpret_cast<float4*>(yo) = v;
    } else {
      yo[0] = v.x;
      if (ox + 1 < w) yo[1] = v.y;
      if (ox + 2 < w) yo[2] = v.z;
      if (ox + 3 < w) yo[3] = v.w;
    }
  }
}

// gx[b][c][p] = sum_o sum_{ky, kx} w[o][c][ky][kx] g[b][o][py - ky + 1][px - kx + 1]: the planes of g stream through a
// two-deep LDS ring (the next plane's window is fetched into registers before the sums of this one and stored after them:
// one barrier per out-channel), out-channels in ascending order.
__global__ void __launch_bounds__(256) percept_conv_rgb_input_grad_kernel(const float* __restrict__ g, const float* __restrict__ wt,
                                                                          float* __restrict__ gx, int out_ch, int h, int w,
                                                                          int tiles_x, int vec) {
  __shared__ float gs[2][PC_XH][PC_XW];
  __shared__ __attribute__((aligned(16))) float ws[PC_MAX_OUT][28];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, b = blockIdx.y;
  const int y0 = ty * PC_TH, x0 = tx * PC_TW;
  const int64_t hw = (int64_t)h * w;
  pc_stage_weights(ws, wt, nullptr, out_ch);
  // the thread's slots of the window: the same for every plane
  int goff[PC_SLOTS], lds[PC_SLOTS];
  bool ok[PC_SLOTS];
#pragma unroll
  for (int s = 0; s < PC_SLOTS; ++s) {
    const int pos = threadIdx.x + 256 * s;
    const int r = pos / PC_XUSED, cc = pos - r * PC_XUSED;
    const int iy = y0 - 1 + r, ix = x0 - 1 + cc;
    ok[s] = pos < PC_XH * PC_XUSED && iy >= 0 && iy < h && ix >= 0 && ix < w;
    goff[s] = ok[s] ? iy * w + ix : 0;
    lds[s] = pos < PC_XH * PC_XUSED ? r * PC_XW + cc : -1;
  }
  const float* gb = g + (int64_t)b * out_ch * hw;
  float held[PC_SLOTS];
  auto fetch = [&](int o) __attribute__((always_inline)) {
    const float* plane = gb + (int64_t)o * hw;
#pragma unroll
    for (int s = 0; s < PC_SLOTS; ++s) held[s] = ok[s] ? plane[goff[s]] : 0.f;
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < PC_SLOTS; ++s)
      if (lds[s] >= 0) (&gs[buf][0][0])[lds[s]] = held[s];
  };
  const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
  float acc[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[c][j] = 0.f;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int o = 0; o < out_ch; ++o) {
    const int buf = o & 1;
    if (o + 1 < out_ch) fetch(o + 1);
    float in[3][6];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int j = 0; j < 6; ++j) in[dy][j] = gs[buf][r + dy][c4 + j];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float wv = ws[o][c * 9 + (2 - dy) * 3 + (2 - dx)];       // window row r + dy is image row py + dy - 1 = py - ky + 1
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[c][j] = fmaf(wv, in[dy][dx + j], acc[c][j]);
        }
    if (o + 1 < out_ch) stash(buf ^ 1);
    __syncthreads();
  }
  const int oy = y0 + r, ox = x0 + c4;
  if (oy >= h || ox >= w) return;
  float* xb = gx + (int64_t)b * 3 * hw + (int64_t)oy * w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* xo = xb + c * hw;
    if (vec) {
      *reinterpret_cast<float4*>(xo) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    } else {
      xo[0] = acc[c][0];
      if (ox + 1 < w) xo[1] = acc[c][1];
      if (ox + 2 < w) xo[2] = acc[c][2];
      if (ox + 3 < w) xo[3] = acc[c][3];
    }
  }
}

// what both take: every out-channel's weights in LDS, one image's planes below 2^31 elements (the window's offsets are int),
// a grid the launch can express
static int pc_rgb_refusal(int batch, int out_ch, int h, int w, int64_t* tiles_x, int64_t* tiles) {
  if (out_ch > PC_MAX_OUT || batch > 65535 || (int64_t)h * w >= (1LL << 31)) return RW_ERR_UNSUPPORTED;
  *tiles_x = rw_cdiv(w, PC_TW);
  *tiles = *tiles_x * rw_cdiv(h, PC_TH);
  return *tiles >= (1LL << 31) ? RW_ERR_UNSUPPORTED : 0;
}

extern "C" int rw_conv3x3_rgb_f32(const float* x, const float* w, const float* bias, float* y, int batch, int out_ch, int h,
                                  int w_, rw_stream_t stream) {
  RW_CHECK_ARG(x && w && bias && y && batch > 0 && out_ch > 0 && h > 0 && w_ > 0);
  int64_t tiles_x, tiles;
  const int refused = pc_rgb_refusal(batch, out_ch, h, w_, &tiles_x, &tiles);
  if (refused) return refused;
  const int vec = w_ % 4 == 0 && rw_aligned16(y);
  hipLaunchKernelGGL(percept_conv_rgb_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, rw_s(stream), x, w, bias, y,
                     out_ch, h, w_, (int)tiles_x, vec);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_conv3x3_rgb_input_grad_f32(const float* g, const float* w, float* gx, int batch, int out_ch, int h, int w_,
                                             rw_stream_t stream) {
  RW_CHECK_ARG(g && w && gx && batch > 0 && out_ch > 0 && h > 0 && w_ > 0);
  int64_t tiles_x, tiles;
  const int refused = pc_rgb_refusal(batch, out_ch, h, w_, &tiles_x, &tiles);
  if (refused) return refused;
  const int vec = w_ % 4 == 0 && rw_aligned16(gx);
  hipLaunchKernelGGL(percept_conv_rgb_input_grad_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, rw_s(stream), g,
                     w, gx, out_ch, h, w_, (int)tiles_x, vec);
  return RW_LAUNCH_RESULT();
}
