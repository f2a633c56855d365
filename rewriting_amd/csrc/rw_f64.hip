// hipcc-flags: -fno-slp-vectorize
// What only the float64 forward of the generator has: the two 3x3 convolutions on v_mfma_f64_16x16x4_f64 (and their
// any-shape form).  Every operand, every product and every accumulation is a double.  The glue ops of the double path
// -- the mapping-network pieces, ApplyStyle, the demodulation factors, NoiseInjectionF, ToRGB -- are the double
// instantiations of the bodies in rw_ops.hip.  The double path runs module by module (no epilogues, no packed weights,
// no routes) and sets no speed bar.
#include "rw_common.h"

typedef double rw_f64x4 __attribute__((ext_vector_type(4)));

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
