// hipcc-flags: -fno-slp-vectorize
// The float64 forward of the generator: the _f64 twins of the mapping-network pieces, ApplyStyle, the demodulation
// factors, NoiseInjectionF and ToRGB, and the two 3x3 convolutions on v_mfma_f64_16x16x4_f64.  Every operand, every
// product and every accumulation is a double; nothing here is shared with the fp32 path, which this file leaves as it
// is.  The double path runs module by module (no epilogues, no packed weights, no routes) and sets no speed bar: the
// kernels are the plain forms of their fp32 twins.
#include "rw_common.h"

typedef double rw_f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double rw_wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// one 4-byte index inside an image's maps: what the kernels below use per lane
static inline bool rw_fits_31(int64_t n) { return n > 0 && n < (1LL << 31); }

// ---------------------------------------------------------------------------------------
// Mapping network pieces
// ---------------------------------------------------------------------------------------
// PixelNormL (models.py:609-614): one wave per latent row.
__global__ void __launch_bounds__(256) pixel_norm_f64_kernel(const double* __restrict__ x, double* __restrict__ y,
                                                             int batch, int dim, double eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= batch) return;
  const double* xr = x + (int64_t)row * dim;
  double ss = 0.0;
  for (int i = lane; i < dim; i += 64) { const double v = xr[i]; ss += v * v; }
  ss = rw_wave_sum_f64(ss);
  const double r = 1.0 / sqrt(ss / (double)dim + eps);
  for (int i = lane; i < dim; i += 64) y[(int64_t)row * dim + i] = xr[i] * r;
}

extern "C" int rw_pixel_norm_f64(const double* x, double* y, int batch, int dim, double eps, rw_stream_t stream) {
  RW_CHECK_ARG(x && y && batch > 0 && dim > 0);
  hipLaunchKernelGGL(pixel_norm_f64_kernel, dim3((batch + 3) / 4), dim3(256), 0, rw_s(stream), x, y, batch, dim, eps);
  return RW_LAUNCH_RESULT();
}

// EqualLinear (models.py:503-511): one wave per (batch row, output feature), any in_dim; the weight is scaled
// before the product, as the reference scales it before F.linear.
__global__ void __launch_bounds__(256) equal_linear_f64_kernel(
    const double* __restrict__ x, const double* __restrict__ w, const double* __restrict__ bias,
    double* __restrict__ y, int batch, int in_dim, int out_dim, int64_t x_stride, double w_scale,
    double b_scale, int act, double alpha, double act_scale) {
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (idx >= (int64_t)batch * out_dim) return;
  const int b = (int)(idx / out_dim), o = (int)(idx % out_dim);
  const double* xr = x + (int64_t)b * x_stride;
  const double* wr = w + (int64_t)o * in_dim;
  double acc = 0.0;
  for (int i = lane; i < in_dim; i += 64) acc += xr[i] * (wr[i] * w_scale);
  acc = rw_wave_sum_f64(acc);
  if (lane == 0) {
    double v = acc + (bias ? bias[o] * b_scale : 0.0);
    if (act) v = ((v > 0.0) ? v : v * alpha) * act_scale;
    y[idx] = v;
  }
}

extern "C" int rw_equal_linear_f64(const double* x, const double* w, const double* bias, double* y,
                                   int batch, int in_dim, int out_dim, int64_t x_stride,
                                   double w_scale, double b_scale, int act, double alpha,
                                   double act_scale, rw_stream_t stream) {
  RW_CHECK_ARG(x && w && y && batch > 0 && in_dim > 0 && out_dim > 0 && x_stride >= in_dim);
  const int64_t waves = (int64_t)batch * out_dim;
  if (!rw_fits_31(rw_cdiv(waves, 4))) return RW_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(equal_linear_f64_kernel, dim3((unsigned)rw_cdiv(waves, 4)), dim3(256), 0, rw_s(stream), x, w, bias,
                     y, batch, in_dim, out_dim, x_stride, w_scale, b_scale, act, alpha, act_scale);
  return RW_LAUNCH_RESULT();
}

// AdjustLatent (models.py:570-583)
__global__ void __launch_bounds__(256) adjust_latent_f64_kernel(const double* __restrict__ w,
                                                                const double* __restrict__ avg,
                                                                double* __restrict__ out, int batch, int n_latent,
                                                                int dim, double psi) {
  const int64_t total = (int64_t)batch * n_latent * dim;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(idx % dim);
    const int b = (int)(idx / ((int64_t)n_latent * dim));
    double v = w[(int64_t)b * dim + d];
    if (avg) { const double a = avg[d]; v = a + psi * (v - a); }
    out[idx] = v;
  }
}

extern "C" int rw_adjust_latent_f64(const double* w, const double* avg, double* out, int batch, int n_latent, int dim,
                                    double psi, rw_stream_t stream) {
  RW_CHECK_ARG(w && out && batch > 0 && n_latent > 0 && dim > 0);
  const int64_t total = (int64_t)batch * n_latent * dim;
  hipLaunchKernelGGL(adjust_latent_f64_kernel, dim3(rw_stream_grid(total, 256)), dim3(256), 0, rw_s(stream), w, avg,
                     out, batch, n_latent, dim, psi);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// ApplyStyle / NoiseInjectionF
// ---------------------------------------------------------------------------------------
// y[row][p] = style[row] * x[row][p]                                  (ApplyStyle, rows = b*C + c)
// y[b][c][p] = x[b][c][p] + nw * noise[b][p]                          (NoiseInjectionF)
template <int MODE>  // 0 = style multiply, 1 = noise add
__global__ void __launch_bounds__(256) row_broadcast_f64_kernel(
    const double* __restrict__ x, const double* __restrict__ aux, const double* __restrict__ nw_ptr,
    double* __restrict__ y, int64_t rows, int channels, int64_t hw) {
  const int64_t total = rows * hw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double nw = (MODE == 1) ? nw_ptr[0] : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / hw;
    if (MODE == 0) {
      y[i] = aux[row] * x[i];
    } else {
      const int64_t b = row / channels;
      y[i] = x[i] + nw * aux[b * hw + (i - row * hw)];
    }
  }
}

extern "C" int rw_style_mul_f64(const double* x, const double* style, double* y, int batch, int channels, int64_t hw,
                                rw_stream_t stream) {
  RW_CHECK_ARG(x && style && y && batch > 0 && channels > 0 && hw > 0);
  const int64_t rows = (int64_t)batch * channels;
  hipLaunchKernelGGL(row_broadcast_f64_kernel<0>, dim3(rw_stream_grid(rows * hw, 256)), dim3(256), 0, rw_s(stream), x,
                     style, (const double*)nullptr, y, rows, channels, hw);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_noise_add_f64(const double* x, const double* noise, const double* noise_w, double* y, int batch,
                                int channels, int64_t hw, rw_stream_t stream) {
  RW_CHECK_ARG(x && noise && noise_w && y && batch > 0 && channels > 0 && hw > 0);
  const int64_t rows = (int64_t)batch * channels;
  hipLaunchKernelGGL(row_broadcast_f64_kernel<1>, dim3(rw_stream_grid(rows * hw, 256)), dim3(256), 0, rw_s(stream), x,
                     noise, noise_w, y, rows, channels, hw);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// Demodulation factors (DemodulatedConv2dF.forward, models.py:320-328)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) weight_sqsum_f64_kernel(const double* __restrict__ w, double* __restrict__ wsq,
                                                               int64_t pairs, int taps, double w_scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int t = 0; t < taps; ++t) { const double v = w_scale * w[i * taps + t]; acc += v * v; }
    wsq[i] = acc;
  }
}

extern "C" int rw_weight_sqsum_f64(const double* w, double* wsq, int out_ch, int in_ch, int taps, double w_scale,
                                   rw_stream_t stream) {
  RW_CHECK_ARG(w && wsq && out_ch > 0 && in_ch > 0 && taps > 0);
  const int64_t pairs = (int64_t)out_ch * in_ch;
  hipLaunchKernelGGL(weight_sqsum_f64_kernel, dim3(rw_stream_grid(pairs, 256)), dim3(256), 0, rw_s(stream), w, wsq,
                     pairs, taps, w_scale);
  return RW_LAUNCH_RESULT();
}

// one wave per (b, o)
__global__ void __launch_bounds__(256) demod_f64_kernel(const double* __restrict__ wsq, const double* __restrict__ style,
                                                        double* __restrict__ demod, int batch, int out_ch, int in_ch,
                                                        double eps) {
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (idx >= (int64_t)batch * out_ch) return;
  const int b = (int)(idx / out_ch), o = (int)(idx % out_ch);
  double acc = 0.0;
  for (int i = lane; i < in_ch; i += 64) {
    const double s = style[(int64_t)b * in_ch + i];
    acc += (s * s) * wsq[(int64_t)o * in_ch + i];
  }
  acc = rw_wave_sum_f64(acc);
  if (lane == 0) demod[idx] = 1.0 / sqrt(acc + eps);
}

extern "C" int rw_demod_f64(const double* wsq, const double* style, double* demod, int batch, int out_ch, int in_ch,
                            double eps, rw_stream_t stream) {
  RW_CHECK_ARG(wsq && style && demod && batch > 0 && out_ch > 0 && in_ch > 0);
  const int64_t waves = (int64_t)batch * out_ch;
  if (!rw_fits_31(rw_cdiv(waves, 4))) return RW_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(demod_f64_kernel, dim3((unsigned)rw_cdiv(waves, 4)), dim3(256), 0, rw_s(stream), wsq, style, demod,
                     batch, out_ch, in_ch, eps);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// ToRGB (models.py:628-655): one pixel per thread, the 3 x C modulated weight rows of this image in LDS.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) to_rgb_f64_kernel(const double* __restrict__ x, const double* __restrict__ w,
                                                         const double* __restrict__ style,
                                                         const double* __restrict__ bias,
                                                         const double* __restrict__ skip, double* __restrict__ y,
                                                         int in_ch, int64_t hw, double w_scale) {
  extern __shared__ double wm64[];  // [3][in_ch]
  const int b = blockIdx.y;
  for (int t = threadIdx.x; t < 3 * in_ch; t += 256) wm64[t] = w_scale * w[t] * style[(int64_t)b * in_ch + t % in_ch];
  __syncthreads();
  const double* xb = x + (int64_t)b * in_ch * hw;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < hw; q += (int64_t)gridDim.x * 256) {
    double a[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int i = 0; i < in_ch; ++i) {
      const double v = xb[(int64_t)i * hw + q];
      a[0] += wm64[i] * v; a[1] += wm64[in_ch + i] * v; a[2] += wm64[2 * in_ch + i] * v;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t off = ((int64_t)b * 3 + c) * hw + q;
      double o = a[c] + (bias ? bias[c] : 0.0);
      if (skip) o += skip[off];
      y[off] = o;
    }
  }
}

extern "C" int rw_to_rgb_f64(const double* x, const double* w, const double* style, const double* bias,
                             const double* skip, double* y, int batch, int in_ch, int64_t hw, double w_scale,
                             rw_stream_t stream) {
  RW_CHECK_ARG(x && w && style && y && batch > 0 && in_ch > 0 && hw > 0);
  if (batch > 65535 || (int64_t)3 * in_ch * sizeof(double) > 48 * 1024) return RW_ERR_UNSUPPORTED;   // in_ch <= 2048
  int gs = (int)rw_cdiv(hw, 256);
  if (gs > 2048) gs = 2048;
  hipLaunchKernelGGL(to_rgb_f64_kernel, dim3(gs, batch), dim3(256), 3 * in_ch * sizeof(double), rw_s(stream), x, w,
                     style, bias, skip, y, in_ch, hw, w_scale);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// The 3x3 convolutions (DemodulatedConv2dF, models.py:313-329) on the weight as stored, W[o][i][ky][kx]:
//   stride 1 (UP = false):  y[b][o][oy][ox] = w_scale demod[b][o] sum_{i,ky,kx} W[o][i][ky][kx] s[b][i] x[b][i][oy+ky-1][ox+kx-1]
//   transposed (UP = true): y[b][o][2 iy + ky][2 ix + kx] += w_scale demod[b][o] W[o][i][ky][kx] s[b][i] x[b][i][iy][ix]
//
// The MFMA form (in_ch % 4 == 0, out_ch % 16 == 0) is an implicit GEMM on v_mfma_f64_16x16x4_f64, D (16 x 16) += A (16 x
// 4) B (4 x 16): rows = out-channels, columns = 16 pixels along x, k = 4 input channels of one tap.  Lane l gives
// A[row = l & 15][k = l >> 4] and B[k = l >> 4][column = l & 15], one double each, and receives
// D[row = (l >> 4) + 4 r][column = l & 15] in result r = 0 .. 3 -- the f64 map, which is NOT the row = 4 (l >> 4) + r of
// every other 16 x 16 MFMA.
//
// Tile: a workgroup of four waves takes four output rows x 16 columns (stride 1) or four output rows x 16 column PAIRS
// (transposed: the even and the odd output column of 16 input columns j; row oy = 2 m + py uses the taps ky = py mod 2
// only, column 2 j + px the taps kx = px mod 2 only, so no product with an inserted zero is formed) x 16 NACC
// out-channels; wave v owns row v.  Per chunk of KC = 8 input channels the input window (style applied on load, zeros
// outside the map) and the 16 NACC x KC x 9 weights are staged in LDS; one B operand feeds NACC MFMAs.
// ---------------------------------------------------------------------------------------
#define RW64_KC 8
#define RW64_WROW (RW64_KC * 9 + 1)      // (+1: out-channel rows start in different banks)
#define RW64_XROWS 6
#define RW64_XCOLS 18

struct rw_conv_f64_problem {
  const double* x; const double* w; double* y; const double* style; const double* demod;
  int in_ch, out_ch, h, w_in, oh, ow;
  double w_scale;
};

template <bool UP, int NACC>
__global__ void __launch_bounds__(256) conv3x3_f64_mfma_kernel(const rw_conv_f64_problem p, int tiles_x) {
  __shared__ double xs[RW64_KC][RW64_XROWS][RW64_XCOLS];
  __shared__ double ws[16 * NACC][RW64_WROW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int oc0 = blockIdx.y * 16 * NACC, b = blockIdx.z;
  // the window of the input this tile reads: rows gy0 .. gy0 + xrows - 1, columns gx0 .. gx0 + xcols - 1
  const int xrows = UP ? 3 : 6, xcols = UP ? 17 : 18;
  const int gy0 = UP ? 2 * ty - 1 : 4 * ty - 1, gx0 = 16 * tx - 1;
  const double* xb = p.x + (int64_t)b * p.in_ch * p.h * p.w_in;
  const double* sb = p.style ? p.style + (int64_t)b * p.in_ch : nullptr;

  rw_f64x4 acc[UP ? 2 : 1][NACC];
#pragma unroll
  for (int q = 0; q < (UP ? 2 : 1); ++q)
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[q][a] = rw_f64x4{0.0, 0.0, 0.0, 0.0};

  const int py = wv & 1;                  // transposed: the parity of this wave's output row (the tile starts on an even one)
  for (int c0 = 0; c0 < p.in_ch; c0 += RW64_KC) {
    __syncthreads();
    for (int idx = tid; idx < RW64_KC * xrows * xcols; idx += 256) {
      const int c = idx / (xrows * xcols), rem = idx - c * (xrows * xcols);
      const int r = rem / xcols, col = rem - r * xcols;
      const int ch = c0 + c, gy = gy0 + r, gx = gx0 + col;
      double v = 0.0;
      if (ch < p.in_ch && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w_in) {
        v = xb[((int64_t)ch * p.h + gy) * p.w_in + gx];
        if (sb) v *= sb[ch];
      }
      xs[c][r][col] = v;
    }
    for (int idx = tid; idx < 16 * NACC * RW64_KC * 9; idx += 256) {
      const int o = idx / (RW64_KC * 9), r = idx - o * (RW64_KC * 9);
      const int ch = c0 + r / 9;
      ws[o][r] = (ch < p.in_ch) ? p.w[((int64_t)(oc0 + o) * p.in_ch + c0) * 9 + r] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < RW64_KC / 4; ++ks) {
      if (c0 + 4 * ks >= p.in_ch) break;            // in_ch % 4 == 0: whole k steps only
      const int c = 4 * ks + kq;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        if (UP && (ky & 1) != py) continue;         // uniform over the wave
        // LDS row of the input this tap reads for the wave's output row
        const int r = UP ? (wv >> 1) + 1 - (ky == 2) : wv + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int col = UP ? n + 1 - (kx == 2) : n + kx;
          const double bv = xs[c][r][col];
#pragma unroll
          for (int a = 0; a < NACC; ++a) {
            const double av = ws[16 * a + n][c * 9 + ky * 3 + kx];
            acc[UP ? (kx & 1) : 0][a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[UP ? (kx & 1) : 0][a], 0, 0, 0);
          }
        }
      }
    }
  }
  // results: acc[q][a][r] = y[oc0 + 16 a + kq + 4 r][oy][ox],  ox = 16 tx + n (stride 1) / 2 (16 tx + n) + q (transposed)
  const int oy = 4 * ty + wv;
  if (oy >= p.oh) return;
  double* yb = p.y + (int64_t)b * p.out_ch * p.oh * p.ow;
#pragma unroll
  for (int q = 0; q < (UP ? 2 : 1); ++q) {
    const int ox = UP ? 2 * (16 * tx + n) + q : 16 * tx + n;
    if (ox >= p.ow) continue;
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = oc0 + 16 * a + kq + 4 * r;
        double v = acc[q][a][r] * p.w_scale;
        if (p.demod) v *= p.demod[(int64_t)b * p.out_ch + o];
        yb[((int64_t)o * p.oh + oy) * p.ow + ox] = v;
      }
  }
}

// Any shape: one thread per output element, the sum in the order (i, ky, kx).
template <bool UP>
__global__ void __launch_bounds__(256) conv3x3_f64_plain_kernel(const rw_conv_f64_problem p, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(idx % p.ow);
    const int oy = (int)((idx / p.ow) % p.oh);
    const int o = (int)((idx / ((int64_t)p.ow * p.oh)) % p.out_ch);
    const int b = (int)(idx / ((int64_t)p.ow * p.oh * p.out_ch));
    const double* xb = p.x + (int64_t)b * p.in_ch * p.h * p.w_in;
    const double* wo = p.w + (int64_t)o * p.in_ch * 9;
    double acc = 0.0;
    for (int i = 0; i < p.in_ch; ++i) {
      const double s = p.style ? p.style[(int64_t)b * p.in_ch + i] : 1.0;
      const double* xi = xb + (int64_t)i * p.h * p.w_in;
      for (int ky = 0; ky < 3; ++ky) {
        int iy;
        if (UP) { if (((oy - ky) & 1) || oy - ky < 0) continue; iy = (oy - ky) >> 1; } else iy = oy + ky - 1;
        if (iy < 0 || iy >= p.h) continue;
        for (int kx = 0; kx < 3; ++kx) {
          int ix;
          if (UP) { if (((ox - kx) & 1) || ox - kx < 0) continue; ix = (ox - kx) >> 1; } else ix = ox + kx - 1;
          if (ix < 0 || ix >= p.w_in) continue;
          acc += wo[i * 9 + ky * 3 + kx] * (s * xi[(int64_t)iy * p.w_in + ix]);
        }
      }
    }
    double v = acc * p.w_scale;
    if (p.demod) v *= p.demod[(int64_t)b * p.out_ch + o];
    p.y[idx] = v;
  }
}

template <bool UP>
static int rw_conv_f64(const double* x, const double* w, double* y, int batch, int in_ch, int out_ch, int h, int w_in,
                       double w_scale, const double* style, const double* demod, rw_stream_t stream) {
  RW_CHECK_ARG(x && w && y && batch > 0 && in_ch > 0 && out_ch > 0 && h > 0 && w_in > 0);
  rw_conv_f64_problem p;
  p.x = x; p.w = w; p.y = y; p.style = style; p.demod = demod;
  p.in_ch = in_ch; p.out_ch = out_ch; p.h = h; p.w_in = w_in;
  p.oh = UP ? 2 * h + 1 : h; p.ow = UP ? 2 * w_in + 1 : w_in;
  p.w_scale = w_scale;
  // the kernels index inside one image's maps, and inside the weight, with 31 bits
  if (!rw_fits_31((int64_t)in_ch * h * w_in) || !rw_fits_31((int64_t)out_ch * p.oh * p.ow) ||
      !rw_fits_31((int64_t)out_ch * in_ch * 9))
    return RW_ERR_UNSUPPORTED;
  if (in_ch % 4 == 0 && out_ch % 16 == 0) {
    const int tiles_x = (int)rw_cdiv(UP ? w_in + 1 : w_in, 16), tiles_y = (int)rw_cdiv(p.oh, 4);
    if (!rw_fits_31((int64_t)tiles_x * tiles_y) || batch > 65535) return RW_ERR_UNSUPPORTED;
    const int nacc = UP ? (out_ch % 32 == 0 ? 2 : 1) : (out_ch % 64 == 0 ? 4 : out_ch % 32 == 0 ? 2 : 1);
    if (out_ch / (16 * nacc) > 65535) return RW_ERR_UNSUPPORTED;
    const dim3 grid(tiles_x * tiles_y, out_ch / (16 * nacc), batch);
    if (nacc == 4) {
      if constexpr (!UP) hipLaunchKernelGGL((conv3x3_f64_mfma_kernel<UP, 4>), grid, dim3(256), 0, rw_s(stream), p, tiles_x);
    } else if (nacc == 2) {
      hipLaunchKernelGGL((conv3x3_f64_mfma_kernel<UP, 2>), grid, dim3(256), 0, rw_s(stream), p, tiles_x);
    } else {
      hipLaunchKernelGGL((conv3x3_f64_mfma_kernel<UP, 1>), grid, dim3(256), 0, rw_s(stream), p, tiles_x);
    }
    return RW_LAUNCH_RESULT();
  }
  const int64_t total = (int64_t)batch * out_ch * p.oh * p.ow;
  hipLaunchKernelGGL(conv3x3_f64_plain_kernel<UP>, dim3(rw_stream_grid(total, 256)), dim3(256), 0, rw_s(stream), p, total);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_conv3x3_f64(const double* x, const double* w, double* y, int batch, int in_ch, int out_ch, int h,
                              int w_in, double w_scale, const double* style, const double* demod, rw_stream_t stream) {
  return rw_conv_f64<false>(x, w, y, batch, in_ch, out_ch, h, w_in, w_scale, style, demod, stream);
}

extern "C" int rw_conv_transpose3x3s2_f64(const double* x, const double* w, double* y, int batch, int in_ch, int out_ch,
                                          int h, int w_in, double w_scale, const double* style, const double* demod,
                                          rw_stream_t stream) {
  return rw_conv_f64<true>(x, w, y, batch, in_ch, out_ch, h, w_in, w_scale, style, demod, stream);
}
