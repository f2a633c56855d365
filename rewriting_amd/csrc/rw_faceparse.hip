// The face-parsing BiSeNet of the edit-distance rows for faces (metrics/load_seg.py:11-35; metrics/face-parsing.PyTorch/
// model.py, resnet.py) and the "pixels correctly modified" count (metrics/seg_correct_mod.py:40-65): what a residual
// segmentation network has and the Inception graph does not.  Its convolutions are rw_conv2d_f32 / rw_conv2d_add_f32 and its
// global averages rw_global_avgpool_f32 (rw_inception.hip); here are
//   * the padded 3 x 3 stride-2 max pooling of the ResNet stem (resnet.py:64,74);
//   * one streaming kernel for every element-wise step of the context path and the fusion module -- the sigmoid channel gate,
//     the broadcast or map that is added, the nearest-neighbour step to the next size (model.py:76-83,111-122,203-209) -- and
//     for the image's nearest-neighbour resize to the working size (load_seg.py:27);
//   * the align_corners=True bilinear up-sampling of the class scores (model.py:251) and the label map: the arg-max over
//     the classes of that sample, picked at the pixel a nearest-neighbour resize reads (load_seg.py:30-34);
//   * the integer counts of the metric (seg_correct_mod.py:51-62).
// float32, NCHW, contiguous, on the caller's stream.  No atomics, no memsets, every sum in a fixed order: two runs give the
// same bits.  The index tables come from the host (rewriting_amd/faceparse.py: nearest_table, align_corners_table); a kernel
// clamps what it reads from one into the map, so that a wrong table gives a wrong picture and never a read outside it.
#include <math.h>
#include "rw_common.h"

#define FP_MAX_CLASSES 64
#define FP_MAX_SET 16
#define FP_MAX_SIDE (1 << 20)

__device__ __forceinline__ int fp_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// ---------------------------------------------------------------------------------------
// F.max_pool2d(x, 3, 2, 1) (resnet.py:64): one thread per output element, the taps in ascending (row, column) order
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) maxpool3x3s2p1_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total,
                                                             int h, int w, int oh, int ow) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % ow);
    const int64_t t = i / ow;
    const int oy = (int)(t % oh);
    const float* xp = x + (t / oh) * h * w;
    float m = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= h) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= w) continue;
        const float v = xp[(int64_t)iy * w + ix];
        if (v > m || v != v) m = v;              // a padded tap is never looked at; a NaN wins, as in max_pool2d
      }
    }
    y[i] = m;
  }
}

extern "C" int rw_maxpool3x3s2p1_f32(const float* x, float* y, int batch, int ch, int h, int w, rw_stream_t stream) {
  RW_CHECK_ARG(x && y && batch >= 1 && ch >= 1 && h >= 1 && w >= 1);
  if (h > FP_MAX_SIDE || w > FP_MAX_SIDE) return RW_ERR_UNSUPPORTED;
  const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
  const int64_t total = (int64_t)batch * ch * oh * ow;
  maxpool3x3s2p1_kernel<<<rw_stream_grid(total, 256), 256, 0, rw_s(stream)>>>(x, y, total, h, w, oh, ow);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// y[b, c, oy, ox] = x[b, c, r, q] s + a,  r = row[oy], q = col[ox] (a null table: that axis keeps its size and its index),
// s = 1 / (1 + expf(-gate[b, c])) or no multiply at all, a = add_map[b, c, r, q] or add_vec[b, c] or nothing.  The product
// is rounded, then the sum: torch's mul followed by add, no fused multiply-add.
// A workgroup works inside one (b, c) map (blockIdx.x), so the gate's exponential is taken once per thread, not per element.
// VEC: the columns keep their index and w is a multiple of 4 -- a thread moves four neighbours with 16-byte accesses.
// ---------------------------------------------------------------------------------------
#define FP_GATE_MAX_BLOCKS_PER_MAP 64

template <bool VEC>
__global__ void __launch_bounds__(256) gate_resample_kernel(const float* x, const float* __restrict__ gate, const float* add_map,
                                                            const float* __restrict__ add_vec, const int* __restrict__ row,
                                                            const int* __restrict__ col, float* __restrict__ y, int h, int w,
                                                            int oh, int ow) {
  const int64_t map = blockIdx.x;
  const float* xp = x + map * h * w;
  const float* ap = add_map ? add_map + map * h * w : nullptr;
  float* yp = y + map * oh * ow;
  const bool gated = gate != nullptr;
  const float s = gated ? 1.f / (1.f + expf(-gate[map])) : 1.f;
  const bool plus = ap != nullptr || add_vec != nullptr;
  const float av = add_vec ? add_vec[map] : 0.f;
  auto value = [&](float v, float a) -> float {
    if (gated) v = __fmul_rn(v, s);
    if (plus) v = __fadd_rn(v, a);
    return v;
  };
  if (VEC) {
    const int w4 = ow >> 2, items = oh * w4;
    for (int i = (int)blockIdx.y * 256 + threadIdx.x; i < items; i += (int)gridDim.y * 256) {
      const int oy = i / w4, q = (i - oy * w4) * 4;
      const int r = row ? fp_clamp(row[oy], h) : oy;
      const rw_f32x4 v = *(const rw_f32x4*)(xp + (int64_t)r * w + q);
      rw_f32x4 a = {av, av, av, av};
      if (ap) a = *(const rw_f32x4*)(ap + (int64_t)r * w + q);
      rw_f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = value(v[e], a[e]);
      *(rw_f32x4*)(yp + (int64_t)oy * ow + q) = o;
    }
  } else {
    const int items = oh * ow;
    for (int i = (int)blockIdx.y * 256 + threadIdx.x; i < items; i += (int)gridDim.y * 256) {
      const int oy = i / ow, ox = i - oy * ow;
      const int r = row ? fp_clamp(row[oy], h) : oy;
      const int q = col ? fp_clamp(col[ox], w) : ox;
      const int64_t at = (int64_t)r * w + q;
      yp[i] = value(xp[at], ap ? ap[at] : av);
    }
  }
}

extern "C" int rw_gate_resample_f32(const float* x, const float* gate, const float* add_map, const float* add_vec,
                                    const int* row, const int* col, float* y, int batch, int ch, int h, int w, int oh, int ow,
                                    rw_stream_t stream) {
  RW_CHECK_ARG(x && y && batch >= 1 && ch >= 1 && h >= 1 && w >= 1 && oh >= 1 && ow >= 1);
  RW_CHECK_ARG(!(add_map && add_vec));
  RW_CHECK_ARG((row || oh == h) && (col || ow == w));           // an axis without a table keeps its size
  if (h > FP_MAX_SIDE || w > FP_MAX_SIDE || oh > FP_MAX_SIDE || ow > FP_MAX_SIDE) return RW_ERR_UNSUPPORTED;
  if ((int64_t)h * w > (1 << 30) || (int64_t)oh * ow > (1 << 30)) return RW_ERR_UNSUPPORTED;       // a map in 31 bits
  const int64_t maps = (int64_t)batch * ch;
  if (maps > 0x7fffffff) return RW_ERR_UNSUPPORTED;
  const bool vec = !col && (w & 3) == 0 && rw_aligned16(x) && rw_aligned16(y) && (!add_map || rw_aligned16(add_map));
  const int64_t items = vec ? (int64_t)oh * (ow >> 2) : (int64_t)oh * ow;
  int64_t per_map = rw_cdiv(items, 256);
  if (per_map > FP_GATE_MAX_BLOCKS_PER_MAP) per_map = FP_GATE_MAX_BLOCKS_PER_MAP;
  const dim3 grid((unsigned)maps, (unsigned)per_map);
  if (vec)
    gate_resample_kernel<true><<<grid, 256, 0, rw_s(stream)>>>(x, gate, add_map, add_vec, row, col, y, h, w, oh, ow);
  else
    gate_resample_kernel<false><<<grid, 256, 0, rw_s(stream)>>>(x, gate, add_map, add_vec, row, col, y, h, w, oh, ow);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// F.interpolate(mode='bilinear', align_corners=True) (model.py:251).  idx: the rows' i0 (oh), the rows' i1 (oh), the
// columns' i0 (ow), the columns' i1 (ow); lam: the rows' (oh), the columns' (ow) -- the layout of lpips.device_tables.
// One sample, in torch's order, every product and sum rounded on its own:
//   (1 - lr) ((1 - lc) v00 + lc v01) + lr ((1 - lc) v10 + lc v11)
// ---------------------------------------------------------------------------------------
struct fp_taps {
  int y0, y1, x0, x1;
  float lr, lc;
};

__device__ __forceinline__ fp_taps fp_taps_at(const int* __restrict__ idx, const float* __restrict__ lam, int py, int px, int h,
                                              int w, int oh, int ow) {
  fp_taps t;
  t.y0 = fp_clamp(idx[py], h);
  t.y1 = fp_clamp(idx[oh + py], h);
  t.x0 = fp_clamp(idx[2 * oh + px], w);
  t.x1 = fp_clamp(idx[2 * oh + ow + px], w);
  t.lr = lam[py];
  t.lc = lam[oh + px];
  return t;
}

__device__ __forceinline__ float fp_bilinear_sample(const float* __restrict__ map, int w, const fp_taps& t) {
  const float* r0 = map + (int64_t)t.y0 * w;
  const float* r1 = map + (int64_t)t.y1 * w;
  const float c0 = __fsub_rn(1.f, t.lc), h0 = __fsub_rn(1.f, t.lr);
  const float top = __fadd_rn(__fmul_rn(c0, r0[t.x0]), __fmul_rn(t.lc, r0[t.x1]));
  const float bottom = __fadd_rn(__fmul_rn(c0, r1[t.x0]), __fmul_rn(t.lc, r1[t.x1]));
  return __fadd_rn(__fmul_rn(h0, top), __fmul_rn(t.lr, bottom));
}

__global__ void __launch_bounds__(256) bilinear_ac_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total,
                                                          int h, int w, int oh, int ow, const int* __restrict__ idx,
                                                          const float* __restrict__ lam) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % ow);
    const int64_t t = i / ow;
    const int oy = (int)(t % oh);
    y[i] = fp_bilinear_sample(x + (t / oh) * h * w, w, fp_taps_at(idx, lam, oy, ox, h, w, oh, ow));
  }
}

static inline bool fp_sides_ok(int h, int w, int oh, int ow) {
  return h <= FP_MAX_SIDE && w <= FP_MAX_SIDE && oh <= FP_MAX_SIDE && ow <= FP_MAX_SIDE && (int64_t)h * w <= (1 << 30);
}

extern "C" int rw_bilinear_ac_f32(const float* x, float* y, int batch, int ch, int h, int w, int oh, int ow, const int* idx,
                                  const float* lam, rw_stream_t stream) {
  RW_CHECK_ARG(x && y && idx && lam && batch >= 1 && ch >= 1 && h >= 1 && w >= 1 && oh >= 1 && ow >= 1);
  if (!fp_sides_ok(h, w, oh, ow)) return RW_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)batch * ch * oh * ow;
  bilinear_ac_kernel<<<rw_stream_grid(total, 256), 256, 0, rw_s(stream)>>>(x, y, total, h, w, oh, ow, idx, lam);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// labels[b, 0, oy, ox] = the lowest class that attains the maximum of the n samples fp_bilinear_sample takes of logits[b]
// at the working-size pixel (pick_row[oy], pick_col[ox]): numpy's argmax(0) of the up-sampled scores (load_seg.py:30-31)
// read through the nearest-neighbour resize of the label map (:33-34), without the (n, H, W) scores in memory.  A NaN
// wins, the first one first, as in numpy.argmax.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) seg_labels_kernel(const float* __restrict__ logits, long long* __restrict__ labels,
                                                         int64_t total, int n, int h, int w, int H, int W,
                                                         const int* __restrict__ idx, const float* __restrict__ lam,
                                                         const int* __restrict__ pick_row, const int* __restrict__ pick_col,
                                                         int OH, int OW) {
  const int64_t plane = (int64_t)h * w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    const int64_t t = i / OW;
    const int oy = (int)(t % OH);
    const int py = pick_row ? fp_clamp(pick_row[oy], H) : oy;
    const int px = pick_col ? fp_clamp(pick_col[ox], W) : ox;
    const fp_taps taps = fp_taps_at(idx, lam, py, px, h, w, H, W);
    const float* lp = logits + (t / OH) * n * plane;
    float best = fp_bilinear_sample(lp, w, taps);
    int arg = 0;
    for (int c = 1; c < n; ++c) {
      const float v = fp_bilinear_sample(lp + c * plane, w, taps);
      if (best == best && (v > best || v != v)) { best = v; arg = c; }
    }
    labels[i] = arg;
  }
}

extern "C" int rw_seg_labels_i64(const float* logits, long long* labels, int batch, int n, int h, int w, int H, int W,
                                 const int* idx, const float* lam, const int* pick_row, const int* pick_col, int OH, int OW,
                                 rw_stream_t stream) {
  RW_CHECK_ARG(logits && labels && idx && lam && batch >= 1 && n >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && OH >= 1 &&
               OW >= 1);
  RW_CHECK_ARG((pick_row || OH == H) && (pick_col || OW == W));
  if (n > FP_MAX_CLASSES) return RW_ERR_UNSUPPORTED;
  if (!fp_sides_ok(h, w, H, W) || OH > FP_MAX_SIDE || OW > FP_MAX_SIDE) return RW_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)batch * OH * OW;
  seg_labels_kernel<<<rw_stream_grid(total, 256), 256, 0, rw_s(stream)>>>(logits, labels, total, n, h, w, H, W, idx, lam,
                                                                          pick_row, pick_col, OH, OW);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// out[b] = (total, count) of seg_correct_mod.py:51-62 for image b: count = the pixels whose `before` label is one of src,
// total = those of them whose `after` label is one of tgt.  One workgroup per image; integer sums: lanes by a butterfly,
// the four waves through LDS.  The label sets travel by value with the launch.
// ---------------------------------------------------------------------------------------
struct fp_label_set {
  long long v[FP_MAX_SET];
  int n;
};

__device__ __forceinline__ bool fp_in_set(long long label, const fp_label_set& set) {
  bool hit = false;
  for (int i = 0; i < set.n; ++i) hit = hit || label == set.v[i];
  return hit;
}

__global__ void __launch_bounds__(256) seg_correct_counts_kernel(const long long* __restrict__ before,
                                                                 const long long* __restrict__ after, int64_t hw,
                                                                 int64_t before_stride, int64_t after_stride, fp_label_set src,
                                                                 fp_label_set tgt, long long* __restrict__ out) {
  __shared__ long long sums[4][2];
  const int64_t b = blockIdx.x;
  const long long* bp = before + b * before_stride;
  const long long* ap = after + b * after_stride;
  long long total = 0, count = 0;
  for (int64_t i = threadIdx.x; i < hw; i += 256) {
    if (!fp_in_set(bp[i], src)) continue;
    ++count;
    total += fp_in_set(ap[i], tgt) ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {           // (two sums per step, not rw_wave_sum twice: the code differs)
    total += __shfl_xor(total, off, 64);
    count += __shfl_xor(count, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { sums[threadIdx.x >> 6][0] = total; sums[threadIdx.x >> 6][1] = count; }
  __syncthreads();
  if (threadIdx.x < 2) out[b * 2 + threadIdx.x] = sums[0][threadIdx.x] + sums[1][threadIdx.x] + sums[2][threadIdx.x] + sums[3][threadIdx.x];
}

extern "C" int rw_seg_correct_counts_i64(const long long* before, const long long* after, int batch, long long hw,
                                         long long before_stride, long long after_stride, const long long* src, int n_src,
                                         const long long* tgt, int n_tgt, long long* out, rw_stream_t stream) {
  RW_CHECK_ARG(before && after && out && src && tgt && batch >= 1 && hw >= 1);
  RW_CHECK_ARG(n_src >= 1 && n_tgt >= 1 && before_stride >= hw && after_stride >= hw);
  if (n_src > FP_MAX_SET || n_tgt > FP_MAX_SET) return RW_ERR_UNSUPPORTED;
  fp_label_set s, t;
  for (int i = 0; i < FP_MAX_SET; ++i) { s.v[i] = i < n_src ? src[i] : 0; t.v[i] = i < n_tgt ? tgt[i] : 0; }
  s.n = n_src;
  t.n = n_tgt;
  seg_correct_counts_kernel<<<(unsigned)batch, 256, 0, rw_s(stream)>>>(before, after, hw, before_stride, after_stride, s, t, out);
  return RW_LAUNCH_RESULT();
}
