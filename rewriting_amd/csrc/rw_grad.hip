// Gradient kernels of the demodulated 3x3 convolution (DemodulatedConv2dF, utils/stylegan2/models.py:291-329) for the
// autograd path: `insert` on a target the fused solver does not restate (several layers, a hooked module, a goal
// batch > 1) runs the reference's loop -- loss.backward() through the module chain (rewrite/ganrewrite.py:265-283) --
// and torch.autograd then needs, per convolution,
//
//   d fmap  = the SAME forward kernels on the transposed (and, stride 1, flipped) weights   (host side: hip.py)
//   d W     = s * sum_{b,p} (g[b,o,p] demod[b,o]) xcol_b[(i,tap), p]                          (rw_conv_wgrad_f32, here)
//             - s^2 W[o,i,t] sum_b sigma[b,i]^2 demod[b,o]^2 sum_p g[b,o,p] y[b,o,p]          (rw_rowdot_f32 + host)
//
// (Q3: the demodulation factor is differentiable).  The weight gradient is the GEMM of the
// solver's K3 (rw_solve.hip) without its Adam epilogue, generalised to a batch and to maps of any size: M = out
// channels, N = (in channel, tap) columns, K = batch x conv-output positions, fp32 MFMA, split-K over workgroups
// with the partial sums reduced in a fixed order (no atomics: the result is deterministic).  The gathered column, the
// extent of the convolution's map and the MFMA row map are rw_common.h's (rw_conv_gather, rw_conv_extent, rw_mfma32_row),
// shared with the solver; the K loop with its operand ring is written out as in K1 / K3 (rw_solve.hip says why).
//
// At the end of the file: the two adjoints of ToRGB (models.py:394-425, 639-655) that a loss on the IMAGE needs -- the
// gradient to the feature map (streaming: 3 planes in, in_ch planes out) and the per-image sums  g . x  over the pixels
// from which the host forms the gradients of the ToRGB weight and of its style (utils/stylegan2/grad.py: ToRGB).
#include "rw_common.h"

#define WG_KC 16        // K chunk: conv-output positions per staging step
#define WG_BM 64        // out channels per workgroup
#define WG_BN 64        // (i, tap) columns per workgroup
#define WG_DEPTH 4      // chunks of operands in flight

struct WgradProblem {
  const float* g;       // (batch, out_ch, CH, CW): gradient w.r.t. the convolution's output map
  const float* x;       // (batch, in_ch, h, w): the (modulated) input map
  const float* gscale;  // (batch, out_ch) factor on g (the demodulation factor), nullable
  const float* xscale;  // (batch, in_ch) factor on x (a style applied on load), nullable
  float* part;          // (ksplit, out_ch, 9 in_ch) partial sums
  int batch, in_ch, out_ch, h, w, upsample, ksplit;
};

__global__ void __launch_bounds__(256) conv_wgrad_kernel(const WgradProblem p) {
  __shared__ float As[2][WG_KC][WG_BM + 4];
  __shared__ float Bs[2][WG_KC][WG_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;      // wave tile: 32 out channels x 32 columns
  const int frow = lane >> 5, fcol = lane & 31;
  const int o0 = blockIdx.x * WG_BM, k0 = blockIdx.y * WG_BN, ks = blockIdx.z;
  const int CW = rw_conv_extent(p.upsample, p.w), P = rw_conv_extent(p.upsample, p.h) * CW;
  const int K = 9 * p.in_ch;
  const int cpb = (P + WG_KC - 1) / WG_KC;                     // chunks per batch item (none straddles two items)
  const int chunks = cpb * p.batch;
  const int cbeg = (int)((int64_t)chunks * ks / p.ksplit), cend = (int)((int64_t)chunks * (ks + 1) / p.ksplit);

  // A staging: thread -> (out channel o0 + tid / 4, four consecutive positions); B: thread -> (column tid % 64,
  // positions tid / 64 + 4 j)
  const int arow = tid >> 2, apart = (tid & 3) * 4;
  const int ao = o0 + arow;
  const bool a_ok = ao < p.out_ch;
  const int bcol = tid & 63, bp0 = tid >> 6;
  const int kmine = k0 + bcol;
  const bool col_ok = kmine < K;
  const int ci = col_ok ? kmine / 9 : 0, ctap = col_ok ? kmine - 9 * ci : 0;
  const int64_t hw = (int64_t)p.h * p.w;

  float areg[WG_DEPTH][4], breg[WG_DEPTH][4];
  auto fetch = [&](int c, int slot) __attribute__((always_inline)) {
    const int b = c / cpb, p0 = (c - b * cpb) * WG_KC;
    const float gs = (a_ok && p.gscale) ? p.gscale[(int64_t)b * p.out_ch + ao] : 1.f;
    const float* gr = p.g + ((int64_t)b * p.out_ch + (a_ok ? ao : 0)) * P;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = p0 + apart + e;
      areg[slot][e] = (a_ok && n < P) ? gr[n] * gs : 0.f;
    }
    const float xs = (col_ok && p.xscale) ? p.xscale[(int64_t)b * p.in_ch + ci] : 1.f;
    const float* xi = p.x + ((int64_t)b * p.in_ch + ci) * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = p0 + bp0 + 4 * j;
      float v = 0.f;
      if (n < P && col_ok) {
        const int y = n / CW;
        v = rw_conv_gather(p, xi, ctap, y, n - y * CW) * xs;
      }
      breg[slot][j] = v;
    }
  };
  auto stash = [&](int buf, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) As[buf][apart + e][arow] = areg[slot][e];
#pragma unroll
    for (int j = 0; j < 4; ++j) Bs[buf][bp0 + 4 * j][bcol] = breg[slot][j];
  };

  rw_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int d = 0; d < WG_DEPTH; ++d)
    if (cbeg + d < cend) fetch(cbeg + d, d);
  if (cbeg < cend) stash(0, 0);
  __syncthreads();
  for (int base = cbeg; base < cend; base += WG_DEPTH) {
#pragma unroll
    for (int d = 0; d < WG_DEPTH; ++d) {
      const int c = base + d;
      if (c < cend) {                                // uniform
        const int buf = d & 1;                       // WG_DEPTH is even
        if (c + WG_DEPTH < cend) fetch(c + WG_DEPTH, d);
#pragma unroll
        for (int kp = 0; kp < WG_KC / 2; ++kp) {
          const float af = As[buf][2 * kp + frow][wm0 + fcol];
          const float bf = Bs[buf][2 * kp + frow][wn0 + fcol];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc, 0, 0, 0);
        }
        if (c + 1 < cend) stash(buf ^ 1, (d + 1) % WG_DEPTH);
        __syncthreads();
      }
    }
  }
  float* out = p.part + (int64_t)ks * p.out_ch * K;
  const int k = k0 + wn0 + fcol;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = o0 + wm0 + rw_mfma32_row(r, frow);
    if (o < p.out_ch && k < K) out[(int64_t)o * K + k] = acc[r];
  }
}

// out[e] = scale * sum_s part[s][e], s in order (deterministic)
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                           int64_t n, int ksplit, float scale) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    float acc = 0.f;
    for (int s = 0; s < ksplit; ++s) acc += part[(int64_t)s * n + e];
    out[e] = acc * scale;
  }
}

extern "C" int rw_conv_wgrad_ksplit(int batch, int in_ch, int out_ch, int h, int w, int upsample) {
  if (batch <= 0 || in_ch <= 0 || out_ch <= 0 || h <= 0 || w <= 0) return 0;
  const int CH = rw_conv_extent(upsample, h), CW = rw_conv_extent(upsample, w);
  const int64_t blocks = rw_cdiv(out_ch, WG_BM) * rw_cdiv(9 * (int64_t)in_ch, WG_BN);
  const int64_t chunks = rw_cdiv((int64_t)CH * CW, WG_KC) * batch;
  int64_t ks = rw_cdiv(1024, blocks);                 // ~4 workgroups per CU
  if (ks > 64) ks = 64;
  if (ks > chunks) ks = chunks;
  if (ks < 1) ks = 1;
  return (int)ks;
}

extern "C" int rw_conv_wgrad_f32(const float* g, const float* x, const float* gscale, const float* xscale,
                                 float* scratch, float* dw, int batch, int in_ch, int out_ch, int h, int w,
                                 int upsample, float scale, rw_stream_t stream) {
  RW_CHECK_ARG(g && x && scratch && dw && batch > 0 && in_ch > 0 && out_ch > 0 && h > 0 && w > 0);
  WgradProblem p;
  p.g = g; p.x = x; p.gscale = gscale; p.xscale = xscale; p.part = scratch;
  p.batch = batch; p.in_ch = in_ch; p.out_ch = out_ch; p.h = h; p.w = w; p.upsample = upsample ? 1 : 0;
  p.ksplit = rw_conv_wgrad_ksplit(batch, in_ch, out_ch, h, w, upsample);
  hipStream_t s = rw_s(stream);
  const dim3 grid((unsigned)rw_cdiv(out_ch, WG_BM), (unsigned)rw_cdiv(9 * (int64_t)in_ch, WG_BN), (unsigned)p.ksplit);
  hipLaunchKernelGGL(conv_wgrad_kernel, grid, dim3(256), 0, s, p);
  const int64_t n = (int64_t)out_ch * in_ch * 9;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rw_stream_grid(n, 256)), dim3(256), 0, s, (const float*)scratch, dw, n,
                     p.ksplit, scale);
  return RW_LAUNCH_RESULT();
}

// out[r] = sum_j a[r][j] b[r][j]: one workgroup per row, float32 products summed in a fixed order per thread,
// then a block tree (per-(image, channel) sums over a feature map: the demodulation term, bias-like gradients)
__global__ void __launch_bounds__(256) rowdot_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* __restrict__ out, int64_t n) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  const float* ar = a + r * n;
  const float* br = b + r * n;
  float acc = 0.f;
  for (int64_t j = threadIdx.x; j < n; j += 256) acc += ar[j] * br[j];
  acc = rw_block_sum_256(acc, red);
  if (threadIdx.x == 0) out[r] = acc;
}

extern "C" int rw_rowdot_f32(const float* a, const float* b, float* out, long long rows, long long n,
                             rw_stream_t stream) {
  RW_CHECK_ARG(a && b && out && rows > 0 && n > 0 && rows < (1LL << 31));
  hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)rows), dim3(256), 0, rw_s(stream), a, b, out, (int64_t)n);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// ToRGB backward (models.py:394-425 with demodulate=False, kernel 1; :639-655): y[b][c][p] = sum_i s W[c][i] style[b][i] x[b][i][p].
//
// d x: gx[b][i][p] = s style[b][i] sum_c W[c][i] g[b][c][p].  Streaming, the mirror of to_rgb_kernel (rw_ops.hip): a thread
// owns 4 consecutive pixels (16-byte accesses along W), reads the three gradient planes once and writes RGI_CG channel
// planes; the 3 x RGI_CG modulated weights of (image, channel group) sit in LDS.  Channel groups are a grid dimension so
// that the 4x4 .. 32x32 maps with 512 channels still fill the chip (g is re-read once per group: 3 planes against 64).
// ---------------------------------------------------------------------------------------
#define RGI_CG 64

template <bool V4>
__global__ void __launch_bounds__(256) to_rgb_input_grad_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                                const float* __restrict__ style, float* __restrict__ gx,
                                                                int in_ch, int64_t hw, float w_scale) {
  __shared__ float wm[3][RGI_CG];
  const int b = blockIdx.y, i0 = blockIdx.z * RGI_CG;
  const int ni = min(RGI_CG, in_ch - i0);
  for (int t = threadIdx.x; t < 3 * RGI_CG; t += 256) {
    const int c = t / RGI_CG, ii = t - c * RGI_CG;
    wm[c][ii] = ii < ni ? w_scale * w[c * in_ch + i0 + ii] * style[(int64_t)b * in_ch + i0 + ii] : 0.f;
  }
  __syncthreads();
  const float* gb = g + (int64_t)b * 3 * hw;
  float* xb = gx + ((int64_t)b * in_ch + i0) * hw;
  if (V4) {
    const int64_t hw4 = hw >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < hw4; q += (int64_t)gridDim.x * 256) {
      const float4 g0 = reinterpret_cast<const float4*>(gb)[q];
      const float4 g1 = reinterpret_cast<const float4*>(gb + hw)[q];
      const float4 g2 = reinterpret_cast<const float4*>(gb + 2 * hw)[q];
#pragma unroll 4
      for (int ii = 0; ii < ni; ++ii) {
        const float w0 = wm[0][ii], w1 = wm[1][ii], w2 = wm[2][ii];
        float4 o;
        o.x = w0 * g0.x + w1 * g1.x + w2 * g2.x;
        o.y = w0 * g0.y + w1 * g1.y + w2 * g2.y;
        o.z = w0 * g0.z + w1 * g1.z + w2 * g2.z;
        o.w = w0 * g0.w + w1 * g1.w + w2 * g2.w;
        reinterpret_cast<float4*>(xb + (int64_t)ii * hw)[q] = o;
      }
    }
  } else {
    // maps whose pixel count is no multiple of four (cropped goal maps: rows of 5 x 7, ...): one pixel per thread
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < hw; q += (int64_t)gridDim.x * 256) {
      const float g0 = gb[q], g1 = gb[hw + q], g2 = gb[2 * hw + q];
      for (int ii = 0; ii < ni; ++ii) xb[(int64_t)ii * hw + q] = wm[0][ii] * g0 + wm[1][ii] * g1 + wm[2][ii] * g2;
    }
  }
}

extern "C" int rw_to_rgb_input_grad_f32(const float* g, const float* w, const float* style, float* gx, int batch,
                                        int in_ch, int64_t hw, float w_scale, rw_stream_t stream) {
  RW_CHECK_ARG(g && w && style && gx && batch > 0 && batch <= 65535 && in_ch > 0 && hw > 0);
  const int groups = (int)rw_cdiv(in_ch, RGI_CG);
  RW_CHECK_ARG(groups <= 65535);
  const bool v4 = hw % 4 == 0;
  int64_t gxn = rw_cdiv(v4 ? hw / 4 : hw, 256);
  const int64_t cap = rw_cdiv(256 * 8, (int64_t)batch * groups);
  if (gxn > cap) gxn = cap;
  if (gxn < 1) gxn = 1;
  const dim3 grid((unsigned)gxn, (unsigned)batch, (unsigned)groups);
  if (v4)
    hipLaunchKernelGGL(to_rgb_input_grad_kernel<true>, grid, dim3(256), 0, rw_s(stream), g, w, style, gx, in_ch, hw, w_scale);
  else
    hipLaunchKernelGGL(to_rgb_input_grad_kernel<false>, grid, dim3(256), 0, rw_s(stream), g, w, style, gx, in_ch, hw, w_scale);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// t[b][c][i] = sum_p g[b][c][p] x[b][i][p]: what d W and d style of ToRGB are made of.  ONE pass over x: a workgroup takes
// (a chunk of RGS_CHUNK pixels, a group of RGS_CG channels, an image), keeps its 3 x 16 gradient values per thread in
// registers and walks the group's channel planes; per channel three sums over the thread's 16 products, a 64-lane
// butterfly, then the four waves' results through LDS -- summed in wave order -- to scratch[chunk][b][c][i].  A second
// small launch adds the chunks in order.  No atomics, nothing zeroed beforehand: two runs are bit-identical.
// ---------------------------------------------------------------------------------------
#define RGS_CG 32
#define RGS_PER_THREAD 16
#define RGS_CHUNK (256 * RGS_PER_THREAD)

template <bool V4>
__device__ __forceinline__ void rgs_load(float (&v)[RGS_PER_THREAD], const float* __restrict__ plane, int64_t p0, int64_t hw) {
  if (V4) {           // hw % 4 == 0 and p0 % 4 == 0: whole float4s are inside the plane or outside it
#pragma unroll
    for (int r = 0; r < RGS_PER_THREAD / 4; ++r) {
      const int64_t p = p0 + 4 * ((int64_t)threadIdx.x + 256 * r);
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < hw) f = *reinterpret_cast<const float4*>(plane + p);
      v[4 * r] = f.x; v[4 * r + 1] = f.y; v[4 * r + 2] = f.z; v[4 * r + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int r = 0; r < RGS_PER_THREAD; ++r) {
      const int64_t p = p0 + threadIdx.x + 256 * r;
      v[r] = p < hw ? plane[p] : 0.f;
    }
  }
}

template <bool V4>
__global__ void __launch_bounds__(256) to_rgb_weight_sums_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                 float* __restrict__ part, int batch, int in_ch, int64_t hw) {
  __shared__ float red[4][3][RGS_CG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = blockIdx.x, p0 = chunk * RGS_CHUNK;
  const int i0 = blockIdx.y * RGS_CG, b = blockIdx.z;
  const int ni = min(RGS_CG, in_ch - i0);
  float gr[3][RGS_PER_THREAD];
#pragma unroll
  for (int c = 0; c < 3; ++c) rgs_load<V4>(gr[c], g + ((int64_t)b * 3 + c) * hw, p0, hw);
  for (int ii = 0; ii < ni; ++ii) {
    float xv[RGS_PER_THREAD];
    rgs_load<V4>(xv, x + ((int64_t)b * in_ch + i0 + ii) * hw, p0, hw);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int e = 0; e < RGS_PER_THREAD; ++e) {
      a0 += gr[0][e] * xv[e]; a1 += gr[1][e] * xv[e]; a2 += gr[2][e] * xv[e];
    }
    a0 = rw_wave_sum(a0); a1 = rw_wave_sum(a1); a2 = rw_wave_sum(a2);
    if (lane == 0) { red[wave][0][ii] = a0; red[wave][1][ii] = a1; red[wave][2][ii] = a2; }
  }
  __syncthreads();
  if (threadIdx.x < 3 * RGS_CG) {
    const int c = threadIdx.x / RGS_CG, ii = threadIdx.x - c * RGS_CG;
    if (ii < ni)
      part[((chunk * batch + b) * 3 + c) * in_ch + i0 + ii] = red[0][c][ii] + red[1][c][ii] + red[2][c][ii] + red[3][c][ii];
  }
}

extern "C" long long rw_to_rgb_weight_sums_scratch_elems(int batch, int in_ch, int64_t hw) {
  if (batch <= 0 || in_ch <= 0 || hw <= 0) return 0;
  return (long long)(rw_cdiv(hw, RGS_CHUNK) * batch * 3 * in_ch);
}

extern "C" int rw_to_rgb_weight_sums_f32(const float* g, const float* x, float* scratch, float* t, int batch, int in_ch,
                                         int64_t hw, rw_stream_t stream) {
  RW_CHECK_ARG(g && x && scratch && t && batch > 0 && batch <= 65535 && in_ch > 0 && hw > 0);
  const int64_t chunks = rw_cdiv(hw, RGS_CHUNK), groups = rw_cdiv(in_ch, RGS_CG);
  RW_CHECK_ARG(chunks < (1LL << 31) && groups <= 65535);
  hipStream_t s = rw_s(stream);
  const dim3 grid((unsigned)chunks, (unsigned)groups, (unsigned)batch);
  if (hw % 4 == 0)
    hipLaunchKernelGGL(to_rgb_weight_sums_kernel<true>, grid, dim3(256), 0, s, g, x, scratch, batch, in_ch, hw);
  else
    hipLaunchKernelGGL(to_rgb_weight_sums_kernel<false>, grid, dim3(256), 0, s, g, x, scratch, batch, in_ch, hw);
  const int64_t n = (int64_t)batch * 3 * in_ch;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rw_stream_grid(n, 256)), dim3(256), 0, s, (const float*)scratch, t, n,
                     (int)chunks, 1.f);
  return RW_LAUNCH_RESULT();
}
