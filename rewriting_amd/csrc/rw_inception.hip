// The Inception-v3 pool3 feature extractor of the FID row (metrics/fid.py:40-62,90-131,190-193): a general convolution as an
// implicit GEMM on the fp32-input MFMA, the 3x3 poolings, the global average and the network's input (clamp or byte map,
// bilinear resize with the arithmetic of F.interpolate(align_corners=False)).
//
// The convolution.  D (out_ch x positions) = Wp^T (out_ch x K) X (K x positions), K = in_ch kh kw in the order of the
// stored weight (channel, then tap row, then tap column), positions = batch oh ow flattened -- so that the 1 x 1 maps at the
// end of a 75 x 75 input still fill a tile with the images of the batch.  A workgroup of four waves owns IC_BM = 64
// out-channels x 128 positions; a wave a 32 x 64 piece of it, two 32 x 32 tiles of v_mfma_f32_32x32x2_f32 that share the
// weight operand (NT = 2).  A launch that would have fewer than IC_WIDE_MIN_WORKGROUPS = 256 such workgroups -- the small
// maps of a small batch, where a few workgroups would walk a long K one after the other -- takes 64 x 64 tiles instead, one
// 32 x 32 tile per wave (NT = 1): twice the workgroups, half the chain per chunk; every output is the same sum in the same
// order in both forms.  K is walked in chunks of IC_KC = 16:
//   * the weight chunk is 16 rows of the packed weight Wp (Kp x Mp, zero padded to multiples of IC_KC and IC_BM by
//     rw_pack_conv2d_weight_f32): 16-byte loads with no bound to check;
//   * the input chunk is gathered: thread t keeps ONE position (t & 127; NT = 1: t & 63) for the whole walk and takes the
//     rows (t >> 7) + 2 j (NT = 1: (t >> 6) + 4 j) of every chunk -- a wave-uniform k, decoded into (channel, tap) on the scalar unit.  A tap outside the
//     map, a k >= K and a position >= N are exact zeros and read nothing;
//   * the next chunk's loads are issued before the current chunk's MFMAs and land in LDS after them.
// The sum.  A product chain in one accumulator is a k-ordered fmaf chain; at K = 4032 (448 x 9) its rounding walks to
// about 1.5e-6 of the result.  Here a chain runs over IC_KB = 4 chunks (64 products) from zero and is then added to the
// total -- two levels, both in ascending k, the same order in every run: about 3e-7 at K = 4032 by the same estimate
// (DESIGN.md section 8.11).  No atomics, no memsets, no split over workgroups.
// Epilogue: + bias[m], then + res (the shortcut of a residual block, face-parsing.PyTorch/resnet.py:36-48; nullable), optional
// ReLU, stored to channel c_off + m of an output with c_total channels.  res has the output's own layout and may be the
// output itself: every element is read and then written by the same thread.
#include <math.h>
#include "rw_common.h"

#define IC_BM 64
#define IC_WIDE_MIN_WORKGROUPS 256
#define IC_KC 16
#define IC_KB 4
#define IC_MAX_TAP 7

struct ic_conv_problem {
  const float* x;
  const float* wp;
  const float* bias;
  const float* res;          // nullable: added after the bias, before the ReLU; indexed as y is
  float* y;
  int in_ch, h, w, out_ch, kh, kw, stride, ph, pw, oh, ow, relu, c_off, c_total;
  int K, Kp, Mp, N;
};

// NT: 32 x 32 tiles per wave along the positions; the workgroup's tile is IC_BM x BN, BN = 64 NT
template <int NT> __global__ void __launch_bounds__(256) conv2d_f32_kernel(ic_conv_problem p) {
  constexpr int BN = 64 * NT, RS = 256 / BN, ROWS = IC_KC / RS;     // a thread gathers the rows kq + RS j, j < ROWS
  __shared__ __attribute__((aligned(16))) float As[IC_KC][IC_BM];
  __shared__ float Bs[IC_KC][BN];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = (int)blockIdx.y * IC_BM, n0 = (int)blockIdx.x * BN;
  const int ohw = p.oh * p.ow, khw = p.kh * p.kw;
  const int64_t plane = (int64_t)p.h * p.w;

  // the position this thread gathers for
  const int gn = n0 + (tid & (BN - 1));
  const bool gvalid = gn < p.N;
  const int gb = gvalid ? gn / ohw : 0;
  const int gpos = gvalid ? gn - gb * ohw : 0;
  const int goy = gpos / p.ow, gox = gpos - goy * p.ow;
  const int iy0 = goy * p.stride - p.ph, ix0 = gox * p.stride - p.pw;
  const float* xb = p.x + (int64_t)gb * p.in_ch * plane;
  const int kq = NT == 2 ? wave >> 1 : wave;     // tid / BN
  // the piece of the weight chunk this thread copies: row tid >> 4, columns 4 (tid & 15) ..
  const int ak = tid >> 4, am = (tid & 15) * 4;

  float bv[ROWS];
  rw_f32x4 av;
  auto fetch = [&](int k0) {
    av = *(const rw_f32x4*)(p.wp + (int64_t)(k0 + ak) * p.Mp + m0 + am);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const int k = k0 + kq + RS * j;            // wave-uniform
      const int c = k / khw, tap = k - c * khw;
      const int ky = tap / p.kw, kx = tap - ky * p.kw;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = gvalid && k < p.K && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
      bv[j] = ok ? xb[(int64_t)c * plane + (int64_t)iy * p.w + ix] : 0.f;
    }
  };

  rw_f32x16 acc[NT], part[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[j][r] = 0.f; part[j][r] = 0.f; }

  const int chunks = p.Kp / IC_KC;
  fetch(0);
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();                             // the MFMAs of the chunk before have read the tiles
    *(rw_f32x4*)&As[ak][am] = av;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) Bs[kq + RS * j][tid & (BN - 1)] = bv[j];
    __syncthreads();
    if (ch + 1 < chunks) fetch((ch + 1) * IC_KC);
#pragma unroll
    for (int s = 0; s < IC_KC / 2; ++s) {
      const int kr = 2 * s + (lane >> 5);
      const float a = As[kr][wm * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        part[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kr][wn * 32 * NT + 32 * j + (lane & 31)], part[j], 0, 0, 0);
    }
    if ((ch & (IC_KB - 1)) == IC_KB - 1 || ch + 1 == chunks) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[j][r] += part[j][r]; part[j][r] = 0.f; }
    }
  }

#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wn * 32 * NT + 32 * j + (lane & 31);
    if (n >= p.N) continue;
    const int b = n / ohw, pos = n - b * ohw;
    const int64_t yo = ((int64_t)b * p.c_total + p.c_off) * ohw + pos;
    float* yb = p.y + yo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + rw_mfma32_row(r, lane >> 5);
      if (m >= p.out_ch) continue;
      float v = acc[j][r] + (p.bias ? p.bias[m] : 0.f);
      if (p.res) v += p.res[yo + (int64_t)m * ohw];
      if (p.relu) v = fmaxf(v, 0.f);
      yb[(int64_t)m * ohw] = v;
    }
  }
}

// wp[k][m] = weight[m][k] for k < K, m < out_ch; zero in the padding
__global__ void __launch_bounds__(256) pack_conv2d_weight_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                                                 int out_ch, int K, int Kp, int Mp) {
  const int64_t total = (int64_t)Kp * Mp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i / Mp), m = (int)(i - (int64_t)k * Mp);
    wp[i] = (k < K && m < out_ch) ? w[(int64_t)m * K + k] : 0.f;
  }
}

static inline bool ic_weight_shape_ok(int out_ch, int in_ch, int kh, int kw) {
  return out_ch >= 1 && in_ch >= 1 && kh >= 1 && kw >= 1 && kh <= IC_MAX_TAP && kw <= IC_MAX_TAP &&
         (int64_t)in_ch * kh * kw <= (1 << 24) && out_ch <= (1 << 24);
}

extern "C" long long rw_conv2d_packed_weight_elems(int out_ch, int in_ch, int kh, int kw) {
  if (!ic_weight_shape_ok(out_ch, in_ch, kh, kw)) return 0;
  return rw_cdiv((int64_t)in_ch * kh * kw, IC_KC) * IC_KC * rw_cdiv(out_ch, IC_BM) * IC_BM;
}

extern "C" int rw_pack_conv2d_weight_f32(const float* weight, float* wp, int out_ch, int in_ch, int kh, int kw,
                                         rw_stream_t stream) {
  RW_CHECK_ARG(weight && wp);
  if (!ic_weight_shape_ok(out_ch, in_ch, kh, kw)) return RW_ERR_UNSUPPORTED;
  const int K = in_ch * kh * kw;
  const int Kp = (int)rw_cdiv(K, IC_KC) * IC_KC, Mp = (int)rw_cdiv(out_ch, IC_BM) * IC_BM;
  pack_conv2d_weight_kernel<<<rw_stream_grid((int64_t)Kp * Mp, 256), 256, 0, rw_s(stream)>>>(weight, wp, out_ch, K, Kp, Mp);
  return RW_LAUNCH_RESULT();
}

static int ic_conv2d(const float* x, const float* wp, const float* bias, const float* res, float* y, int batch, int in_ch,
                     int h, int w, int out_ch, int kh, int kw, int stride, int ph, int pw, int relu, int c_off, int c_total,
                     rw_stream_t stream) {
  RW_CHECK_ARG(x && wp && y && batch >= 1 && h >= 1 && w >= 1);
  RW_CHECK_ARG(out_ch >= 1 && in_ch >= 1 && kh >= 1 && kw >= 1);
  RW_CHECK_ARG(c_off >= 0 && c_total >= 1 && (int64_t)c_off + out_ch <= c_total);
  if (!ic_weight_shape_ok(out_ch, in_ch, kh, kw)) return RW_ERR_UNSUPPORTED;
  if (stride != 1 && stride != 2) return RW_ERR_UNSUPPORTED;
  if (ph < 0 || pw < 0 || ph >= kh || pw >= kw) return RW_ERR_UNSUPPORTED;
  if (h + 2 * ph < kh || w + 2 * pw < kw) return RW_ERR_UNSUPPORTED;          // no output position
  if (!rw_aligned16(wp)) return RW_ERR_UNSUPPORTED;
  const int oh = (h + 2 * ph - kh) / stride + 1, ow = (w + 2 * pw - kw) / stride + 1;
  const int64_t N = (int64_t)batch * oh * ow;
  if (N > (1 << 30) || (int64_t)h * w > (1 << 30)) return RW_ERR_UNSUPPORTED;  // positions and a plane in 31 bits
  ic_conv_problem p;
  p.x = x; p.wp = wp; p.bias = bias; p.res = res; p.y = y;
  p.in_ch = in_ch; p.h = h; p.w = w; p.out_ch = out_ch; p.kh = kh; p.kw = kw; p.stride = stride; p.ph = ph; p.pw = pw;
  p.oh = oh; p.ow = ow; p.relu = relu ? 1 : 0; p.c_off = c_off; p.c_total = c_total;
  p.K = in_ch * kh * kw;
  p.Kp = (int)rw_cdiv(p.K, IC_KC) * IC_KC;
  p.Mp = (int)rw_cdiv(out_ch, IC_BM) * IC_BM;
  p.N = (int)N;
  const int m_tiles = p.Mp / IC_BM;
  if (m_tiles > 65535) return RW_ERR_UNSUPPORTED;
  // 128 positions per workgroup where that still gives every CU of a whole chip a workgroup, 64 below (the same bits)
  if (rw_cdiv(N, 128) * m_tiles >= IC_WIDE_MIN_WORKGROUPS)
    conv2d_f32_kernel<2><<<dim3((unsigned)rw_cdiv(N, 128), (unsigned)m_tiles), 256, 0, rw_s(stream)>>>(p);
  else
    conv2d_f32_kernel<1><<<dim3((unsigned)rw_cdiv(N, 64), (unsigned)m_tiles), 256, 0, rw_s(stream)>>>(p);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_conv2d_f32(const float* x, const float* wp, const float* bias, float* y, int batch, int in_ch, int h,
                             int w, int out_ch, int kh, int kw, int stride, int ph, int pw, int relu, int c_off,
                             int c_total, rw_stream_t stream) {
  return ic_conv2d(x, wp, bias, nullptr, y, batch, in_ch, h, w, out_ch, kh, kw, stride, ph, pw, relu, c_off, c_total, stream);
}

// y = act((conv + bias) + res): the tail of a BasicBlock (face-parsing.PyTorch/resnet.py:36-48); res and y (batch, out_ch, oh, ow)
extern "C" int rw_conv2d_add_f32(const float* x, const float* wp, const float* bias, const float* res, float* y, int batch,
                                 int in_ch, int h, int w, int out_ch, int kh, int kw, int stride, int ph, int pw, int relu,
                                 rw_stream_t stream) {
  RW_CHECK_ARG(res);
  return ic_conv2d(x, wp, bias, res, y, batch, in_ch, h, w, out_ch, kh, kw, stride, ph, pw, relu, 0, out_ch, stream);
}

// ---------------------------------------------------------------------------------------
// The 3x3 poolings: one thread per output element, the taps in ascending (row, column) order
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pool3x3_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int batch, int ch,
                                                          int h, int w, int oh, int ow, int mode, int c_off, int c_total) {
  const int stride = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
  const int64_t total = (int64_t)batch * ch * oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % ow);
    int64_t t = i / ow;
    const int oy = (int)(t % oh);
    t /= oh;
    const int c = (int)(t % ch), b = (int)(t / ch);
    const float* xp = x + ((int64_t)b * ch + c) * h * w;
    float m = -INFINITY, sum = 0.f;
    int count = 0;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * stride - pad + ky;
      if (iy < 0 || iy >= h) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * stride - pad + kx;
        if (ix < 0 || ix >= w) continue;
        const float v = xp[(int64_t)iy * w + ix];
        if (v > m || v != v) m = v;              // a padded tap is never looked at; a NaN wins, as in max_pool2d
        sum += v;
        ++count;
      }
    }
    y[(((int64_t)b * c_total + c_off + c) * oh + oy) * ow + ox] = mode == 1 ? sum / (float)count : m;
  }
}

extern "C" int rw_pool3x3_f32(const float* x, float* y, int batch, int ch, int h, int w, int mode, int c_off, int c_total,
                              rw_stream_t stream) {
  RW_CHECK_ARG(x && y && batch >= 1 && ch >= 1 && h >= 1 && w >= 1 && mode >= 0 && mode <= 2);
  RW_CHECK_ARG(c_off >= 0 && c_total >= 1 && (int64_t)c_off + ch <= c_total);
  if (mode == 0 && (h < 3 || w < 3)) return RW_ERR_UNSUPPORTED;               // no window
  const int oh = mode == 0 ? (h - 3) / 2 + 1 : h, ow = mode == 0 ? (w - 3) / 2 + 1 : w;
  const int64_t total = (int64_t)batch * ch * oh * ow;
  pool3x3_f32_kernel<<<rw_stream_grid(total, 256), 256, 0, rw_s(stream)>>>(x, y, batch, ch, h, w, oh, ow, mode, c_off,
                                                                           c_total);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// The global average: one wave per (image, channel); lane l sums the elements l, l + 64, ... in ascending order, the
// lanes are added by a butterfly -- a fixed order.  The sum is kept in double and rounded once, as the host's mean of a
// float tensor is (the kernel is bound by its loads: the wider adds cost nothing).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) global_avgpool_f32_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 int64_t maps, int64_t hw) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= maps) return;                       // wave-uniform
  const float* xp = x + map * hw;
  double sum = 0.0;
  for (int64_t i = lane; i < hw; i += 64) sum += (double)xp[i];
  sum = rw_wave_sum(sum);
  if (lane == 0) y[map] = (float)(sum / (double)hw);
}

extern "C" int rw_global_avgpool_f32(const float* x, float* y, int batch, int ch, int h, int w, rw_stream_t stream) {
  RW_CHECK_ARG(x && y && batch >= 1 && ch >= 1 && h >= 1 && w >= 1);
  const int64_t maps = (int64_t)batch * ch, hw = (int64_t)h * w;
  if (rw_cdiv(maps, 4) > 0x7fffffff || hw > (1 << 24)) return RW_ERR_UNSUPPORTED;   // hw exact as a float
  global_avgpool_f32_kernel<<<(unsigned)rw_cdiv(maps, 4), 256, 0, rw_s(stream)>>>(x, y, maps, hw);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// The network's input: y (B, 3, out_h, out_w) float from float (B, 3, in_h, in_w) clamped to [-1, 1] or from bytes
// (B, in_h, in_w, 3) mapped by x / 127.5 - 1, resized with the arithmetic of F.interpolate(mode='bilinear',
// align_corners=False): scale = in / out in float, source = scale (d + 0.5) - 0.5 clamped at 0, no antialiasing; an axis
// that keeps its size takes its sample as it is.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void ic_source(int d, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  if (in == out) { i0 = i1 = d; l0 = 1.f; l1 = 0.f; return; }
  const float scale = (float)in / (float)out;
  float src = scale * ((float)d + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)floorf(src);
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  l0 = 1.f - l1;
}

template <bool BYTES>
__global__ void __launch_bounds__(256) inception_input_kernel(const void* __restrict__ images, float* __restrict__ y, int batch,
                                                              int ih, int iw, int oh, int ow) {
  const int64_t total = (int64_t)batch * 3 * oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % ow);
    int64_t t = i / ow;
    const int oy = (int)(t % oh);
    t /= oh;
    const int c = (int)(t % 3), b = (int)(t / 3);
    auto sample = [&](int sy, int sx) -> float {
      if (BYTES) {
        const unsigned char v = ((const unsigned char*)images)[(((int64_t)b * ih + sy) * iw + sx) * 3 + c];
        return (float)v / 127.5f - 1.f;
      }
      const float v = ((const float*)images)[(((int64_t)b * 3 + c) * ih + sy) * iw + sx];
      return fminf(fmaxf(v, -1.f), 1.f);
    };
    float v;
    if (ih == oh && iw == ow) {
      v = sample(oy, ox);
    } else {
      int y0, y1, x0, x1;
      float hy0, hy1, wx0, wx1;
      ic_source(oy, ih, oh, y0, y1, hy0, hy1);
      ic_source(ox, iw, ow, x0, x1, wx0, wx1);
      v = hy0 * (wx0 * sample(y0, x0) + wx1 * sample(y0, x1)) + hy1 * (wx0 * sample(y1, x0) + wx1 * sample(y1, x1));
    }
    y[i] = v;
  }
}

extern "C" int rw_inception_input_f32(const void* images, float* y, int batch, int in_h, int in_w, int out_h, int out_w,
                                      int is_bytes, rw_stream_t stream) {
  RW_CHECK_ARG(images && y && batch >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1);
  if (in_h > (1 << 20) || in_w > (1 << 20) || out_h > (1 << 20) || out_w > (1 << 20)) return RW_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)batch * 3 * out_h * out_w;
  const int grid = rw_stream_grid(total, 256);
  if (is_bytes)
    inception_input_kernel<true><<<grid, 256, 0, rw_s(stream)>>>(images, y, batch, in_h, in_w, out_h, out_w);
  else
    inception_input_kernel<false><<<grid, 256, 0, rw_s(stream)>>>(images, y, batch, in_h, in_w, out_h, out_w);
  return RW_LAUNCH_RESULT();
}
