// PIL-exact bilinear resize on gfx950: the bytes of renormalize.as_url(img, size=...)'s PIL.Image.resize(size,
// resample=BILINEAR) (utils/renormalize.py:22-32) for a batch of (H, W, 3) uint8 pictures, as what rw_render_bytes_f32
// writes and rw_png_filter_u8 reads.  Pillow's 8-bit resampler is integer work over fixed-point tables that the host
// computes in double (rewriting_amd/resample.py; the definition stands in include/rewriting_hip.h); the kernels apply the
// tables:
//     out[o] = clamp((2^21 + sum_{j < count[o]} k[o][j] * in[first[o] + j]) >> 22, 0, 255)      int32, arithmetic shift
// along x into the scratch, rounded to bytes, then along y into out -- two plain launches, each skipped when its axis keeps
// its length.  No allocation, memset, atomic or stream drain; every byte written has one writer.
//
// A workgroup is four waves, one per row: lane l of a wave owns item 64 t + l of its row.
//   x pass: the rows of all pictures are one list of images * H rows.  An item is V output pixels (V = 4: twelve bytes,
//           three dword stores, where OW % 4 == 0 and the destination is 4-byte aligned; else V = 1, three byte stores).
//           Neighbouring lanes read neighbouring source pixels.
//   y pass: an item is R consecutive bytes of an output row (R = 4: one dword load per source row and one dword store,
//           where 3 OW % 4 == 0 and both pointers are 4-byte aligned; else R = 1).  The row's first, count and
//           coefficients are wave-uniform: scalar loads.
// Whatever the tables hold, nothing outside the picture is read: count is clamped to 0 .. K, first to the axis, and
// source index first + j to its last sample.  The sum is kept unsigned (wraps, never traps) and shifted as int32: a wrong
// table gives a wrong picture, never a fault.  The tables are signed and the shift arithmetic, so that Pillow's other
// separable filters fit the same kernels.
#include "rw_common.h"

#define RS_ROWS 4                                          // waves (rows) per workgroup
#define RS_BLOCK (RS_ROWS * RW_WAVE)
#define RS_SHIFT 22                                        // Pillow's PRECISION_BITS = 32 - 8 - 2

struct rs_pass {
  const uint8_t* src;      // x pass: (rows, n, 3); y pass: (images, n, row_bytes)
  uint8_t* dst;            // x pass: (rows, m, 3); y pass: (images, m, row_bytes)
  const int32_t* k;        // (m, K)
  const int32_t* bounds;   // (m, 2) = first, count
  int K, n, m;             // the axis: n samples in, m out
  int row_bytes;           // y pass: bytes of a row
  int64_t rows;            // x pass: images * H; y pass: images * m
  unsigned tiles_x;        // workgroups along a row
};

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned rs_byte(unsigned acc) { return (unsigned)rs_clamp((int)acc >> RS_SHIFT, 0, 255); }

template <int V>
__global__ void __launch_bounds__(RS_BLOCK) resize_x_kernel(const rs_pass p) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
  const int64_t row = (int64_t)tile_y * RS_ROWS + wave;
  const int o0 = (int)(tile_x * RW_WAVE + lane) * V;       // < m + 64 V: the entry keeps 3 m in 31 bits
  if (row >= p.rows || o0 >= p.m) return;                  // V == 4: m % 4 == 0, the four pixels are in or out together
  const uint8_t* src = p.src + row * p.n * 3;
  uint8_t* dst = p.dst + (row * p.m + o0) * 3;
  unsigned b[3 * V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int o = o0 + v;
    const int first = rs_clamp(p.bounds[2 * o], 0, p.n - 1), count = rs_clamp(p.bounds[2 * o + 1], 0, p.K);
    const int room = p.n - 1 - first;
    const int32_t* k = p.k + (int64_t)o * p.K;
    unsigned acc0 = 1u << (RS_SHIFT - 1), acc1 = acc0, acc2 = acc0;
    for (int j = 0; j < count; ++j) {
      const uint8_t* s = src + 3 * (first + (j < room ? j : room));
      const unsigned kj = (unsigned)k[j];
      acc0 += kj * s[0]; acc1 += kj * s[1]; acc2 += kj * s[2];
    }
    b[3 * v] = rs_byte(acc0); b[3 * v + 1] = rs_byte(acc1); b[3 * v + 2] = rs_byte(acc2);
  }
  if constexpr (V == 4) {
    unsigned* d32 = reinterpret_cast<unsigned*>(dst);      // 12-byte items past a 4-byte aligned base
#pragma unroll
    for (int q = 0; q < 3; ++q) d32[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
  } else {
    dst[0] = (uint8_t)b[0]; dst[1] = (uint8_t)b[1]; dst[2] = (uint8_t)b[2];
  }
}

template <int R>
__global__ void __launch_bounds__(RS_BLOCK) resize_y_kernel(const rs_pass p) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
  const int64_t row = (int64_t)tile_y * RS_ROWS + wave;    // (image, output row), wave-uniform
  const int x0 = (int)(tile_x * RW_WAVE + lane) * R;
  if (row >= p.rows || x0 >= p.row_bytes) return;          // R == 4: row_bytes % 4 == 0
  const int64_t img = row / p.m;
  const int o = (int)(row - img * p.m);
  const int first = rs_clamp(p.bounds[2 * o], 0, p.n - 1), count = rs_clamp(p.bounds[2 * o + 1], 0, p.K);
  const int room = p.n - 1 - first;
  const int32_t* k = p.k + (int64_t)o * p.K;
  const uint8_t* src = p.src + (img * p.n + first) * p.row_bytes + x0;
  unsigned acc[R];
#pragma unroll
  for (int c = 0; c < R; ++c) acc[c] = 1u << (RS_SHIFT - 1);
  for (int j = 0; j < count; ++j) {
    const uint8_t* s = src + (int64_t)(j < room ? j : room) * p.row_bytes;
    const unsigned kj = (unsigned)k[j];
    if constexpr (R == 4) {
      const unsigned w = *reinterpret_cast<const unsigned*>(s);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += kj * ((w >> (8 * c)) & 0xffu);
    } else {
      acc[0] += kj * s[0];
    }
  }
  uint8_t* dst = p.dst + row * p.row_bytes + x0;
  if constexpr (R == 4)
    *reinterpret_cast<unsigned*>(dst) = rs_byte(acc[0]) | (rs_byte(acc[1]) << 8) | (rs_byte(acc[2]) << 16) | (rs_byte(acc[3]) << 24);
  else
    dst[0] = (uint8_t)rs_byte(acc[0]);
}

// the grid of a pass: ceil(items / 64) workgroups along a row times ceil(rows / 4); false where it passes 31 bits
static bool rs_grid(rs_pass& p, int64_t items, unsigned& blocks) {
  const int64_t tiles_x = rw_cdiv(items, RW_WAVE), total = tiles_x * rw_cdiv(p.rows, RS_ROWS);
  if (total > INT32_MAX) return false;
  p.tiles_x = (unsigned)tiles_x;
  blocks = (unsigned)total;
  return true;
}

extern "C" int rw_resize_bilinear_u8(const uint8_t* image, const int32_t* kx, const int32_t* bounds_x, const int32_t* ky,
                                     const int32_t* bounds_y, uint8_t* scratch, uint8_t* out, int64_t images, int height,
                                     int width, int out_height, int out_width, int kx_width, int ky_width,
                                     rw_stream_t stream) {
  const bool along_x = out_width != width, along_y = out_height != height;
  RW_CHECK_ARG(image && out && images >= 1);
  RW_CHECK_ARG(along_x || along_y);                        // neither axis changes: the picture is the caller's own
  RW_CHECK_ARG(!along_x || (kx && bounds_x && kx_width >= 1));
  RW_CHECK_ARG(!along_y || (ky && bounds_y && ky_width >= 1));
  RW_CHECK_ARG(!(along_x && along_y) || scratch);
  if (height < 1 || width < 1 || out_height < 1 || out_width < 1) return RW_ERR_UNSUPPORTED;
  // offsets inside a row and a picture's size are 32-bit; picture and row bases are 64-bit
  if (3 * (int64_t)height * width > INT32_MAX || 3 * (int64_t)height * out_width > INT32_MAX ||
      3 * (int64_t)out_height * out_width > INT32_MAX)
    return RW_ERR_UNSUPPORTED;
  RW_CHECK_ARG(images <= INT64_MAX / INT32_MAX);           // images * rows stays in 64 bits

  rs_pass px = {}, py = {};
  unsigned blocks_x = 0, blocks_y = 0;
  bool vx = false, vy = false;
  if (along_x) {
    px.src = image; px.dst = along_y ? scratch : out;
    px.k = kx; px.bounds = bounds_x; px.K = kx_width; px.n = width; px.m = out_width;
    px.rows = images * height;
    vx = out_width % 4 == 0 && ((uintptr_t)px.dst % 4) == 0;
    RW_CHECK_ARG(rs_grid(px, vx ? out_width / 4 : out_width, blocks_x));
  }
  if (along_y) {
    py.src = along_x ? scratch : image; py.dst = out;
    py.k = ky; py.bounds = bounds_y; py.K = ky_width; py.n = height; py.m = out_height;
    py.row_bytes = 3 * out_width;
    py.rows = images * out_height;
    vy = py.row_bytes % 4 == 0 && ((uintptr_t)py.src % 4) == 0 && ((uintptr_t)py.dst % 4) == 0;
    RW_CHECK_ARG(rs_grid(py, vy ? py.row_bytes / 4 : py.row_bytes, blocks_y));
  }
  hipStream_t s = rw_s(stream);
  if (along_x) {
    if (vx) hipLaunchKernelGGL(resize_x_kernel<4>, dim3(blocks_x), dim3(RS_BLOCK), 0, s, px);
    else hipLaunchKernelGGL(resize_x_kernel<1>, dim3(blocks_x), dim3(RS_BLOCK), 0, s, px);
  }
  if (along_y) {
    if (vy) hipLaunchKernelGGL(resize_y_kernel<4>, dim3(blocks_y), dim3(RS_BLOCK), 0, s, py);
    else hipLaunchKernelGGL(resize_y_kernel<1>, dim3(blocks_y), dim3(RS_BLOCK), 0, s, py);
  }
  return RW_LAUNCH_RESULT();
}
