// Overlays on gfx950: the bytes of ImageVisualizer.masked_image / renormalize.as_image (utils/imgviz.py:56-122,309-330,
// utils/upsample.py:124-156, utils/renormalize.py:15-19) for a batch of images, in ONE launch: byte conversion, the
// heat map > level (or a byte mask), its outline `thickness` wide, and the blend, written (B, H, W, 3) uint8 as
// PIL.Image.fromarray takes it.
//
// One workgroup of 256 threads per tile of RD_TH rows x 64 columns, (image, tile) flattened over the grid.
//   1. inside bits of the tile's rows and of `thickness` rows above and below, as 64-bit row words in LDS: a wave
//      evaluates 64 consecutive pixels of a row and its __ballot IS the word.  The 8 columns left and right of the tile
//      (thickness <= 8) come as 8 rows x 8 columns per wave, one byte per row.  The heat map is a few KiB and stays in
//      cache.
//   2. one thread per row ORs the row word with its shifts by 1 .. thickness (taking the side bytes in).
//   3. a lane owns four consecutive pixels of a row: it ORs the 2 thickness + 1 dilated row words around its row (one
//      ds_read_b64 each, the same address in 16 lanes), loads one float4 per channel and stores three dwords of 12 packed
//      bytes.  V = 1 (one pixel, three byte stores, per lane and step) where W % 4 != 0 or a pointer is not aligned.
//
// The inside bit of a pixel comes from rd_inside() alone, which sees (y, x), the sizes, the selector and the level --
// not the tile, the wave, the batch or V: a halo pixel of one tile and the same pixel inside the next tile agree, and an
// image's bytes are the same alone or in a batch, aligned or not.  Every out byte has one writer; nothing is zeroed
// first, no atomics, no partial slots.  Products and sums are rounded one by one (no contraction into fused
// multiply-adds): `data * mul + add` of renormalize.py rounds twice, and so must this.
#include "rw_common.h"

#include <math.h>

// HIP's rd_mul / rd_add are plain operators that the compiler may still contract; these, compiled with contraction
// off, are not.
#pragma clang fp contract(off)
__device__ __forceinline__ float rd_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rd_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rd_sub(float a, float b) { return a - b; }

#define RD_BLOCK 256
#define RD_TW 64                                           // one row word
#define RD_TH 16
#define RD_ROWS (RD_TH + 2 * RW_RENDER_MAX_THICKNESS)      // rows of inside bits a tile can need
#define RD_SIDE 8                                          // columns kept left and right of the tile

struct rd_problem {
  const float* image;      // (B, 3, H, W)
  const void* sel;         // mode 1: float (B, h, w); mode 2: bytes (B, H, W)
  uint8_t* out;            // (B, H, W, 3)
  int H, W, h, w;
  int tiles_x, tiles_per_image;
  int thickness;
  float level, inv2H, inv2W, outside_bright;
  unsigned border_rgb;     // r | g << 8 | b << 16
  int inside_rgb;          // the same, or < 0: an inside pixel keeps the image's bytes
};

// Is pixel (y, x) of the image inside?  Pixels beyond the image's edge are not.  sel: this image's selector.
//   mode 2: its mask byte is non-zero.
//   mode 1: up(y, x) > level with up bilinear over the heat map's pixel centres, zeros outside the map:
//           fy = ((2y + 1) h - H) / 2H = (y + 1/2) h / H - 1/2, rows floor(fy) and floor(fy) + 1 weighted 1 - t and t.
//           NaN compares false.
__device__ __forceinline__ bool rd_inside(int mode, const void* __restrict__ sel, int y, int x, int H, int W, int h, int w,
                                          float inv2H, float inv2W, float level) {
  if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return false;
  if (mode == 2) return static_cast<const uint8_t*>(sel)[y * W + x] != 0;
  const float* heat = static_cast<const float*>(sel);
  const float fy = rd_mul((float)((2 * y + 1) * h - H), inv2H);
  const float fx = rd_mul((float)((2 * x + 1) * w - W), inv2W);
  const float y0f = floorf(fy), x0f = floorf(fx);
  const float ty = rd_sub(fy, y0f), tx = rd_sub(fx, x0f);
  const float sy = rd_sub(1.f, ty), sx = rd_sub(1.f, tx);
  const int y0 = (int)y0f, x0 = (int)x0f;                  // -1 .. h - 1, -1 .. w - 1
  const bool r0 = y0 >= 0, r1 = y0 + 1 < h, c0 = x0 >= 0, c1 = x0 + 1 < w;
  const float v00 = (r0 && c0) ? heat[y0 * w + x0] : 0.f;
  const float v01 = (r0 && c1) ? heat[y0 * w + x0 + 1] : 0.f;
  const float v10 = (r1 && c0) ? heat[(y0 + 1) * w + x0] : 0.f;
  const float v11 = (r1 && c1) ? heat[(y0 + 1) * w + x0 + 1] : 0.f;
  const float top = rd_add(rd_mul(v00, sx), rd_mul(v01, tx));
  const float bot = rd_add(rd_mul(v10, sx), rd_mul(v11, tx));
  const float up = rd_add(rd_mul(top, sy), rd_mul(bot, ty));
  return up > level;
}

// trunc(clamp(v, 0, 255)) as .clamp(0, 255).byte() gives it; NaN -> 0
__device__ __forceinline__ unsigned rd_byte(float v) { return (unsigned)fminf(fmaxf(v, 0.f), 255.f); }

// one channel of one pixel: s = the image's byte; border / inside / outside decide what is shown
__device__ __forceinline__ unsigned rd_blend(float x, bool inside, bool border, unsigned border_c, int inside_c,
                                             float outside_bright) {
  const unsigned s = rd_byte(rd_add(rd_mul(x, 127.5f), 127.5f));
  if (border) return border_c;
  if (inside) return inside_c >= 0 ? (unsigned)inside_c : s;
  return rd_byte(rd_mul(outside_bright, (float)s));
}

template <int MODE, int V>
__global__ void __launch_bounds__(RD_BLOCK) render_bytes_kernel(const rd_problem p) {
  __shared__ unsigned long long centre[RD_ROWS];           // inside bits of columns tx0 .. tx0 + 63, rows ty0 - T ..
  __shared__ unsigned long long grown[RD_ROWS];            // the same, dilated along x by T
  __shared__ unsigned side[2][RD_ROWS];                    // 8 bits: columns tx0 - 8 .. tx0 - 1 / tx0 + 64 .. tx0 + 71

  const int img = blockIdx.x / p.tiles_per_image;
  const int tile = blockIdx.x - img * p.tiles_per_image;
  const int ty0 = (tile / p.tiles_x) * RD_TH, tx0 = (tile % p.tiles_x) * RD_TW;
  const int H = p.H, W = p.W, T = p.thickness;
  const int hw = H * W;                                    // 3 * hw fits 31 bits (checked by the entry)
  const float* src = p.image + (int64_t)img * 3 * hw;
  uint8_t* dst = p.out + (int64_t)img * 3 * hw;

  if constexpr (MODE != 0) {
    const void* sel = MODE == 1 ? static_cast<const void*>(static_cast<const float*>(p.sel) + (int64_t)img * p.h * p.w)
                                : static_cast<const void*>(static_cast<const uint8_t*>(p.sel) + (int64_t)img * hw);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = RD_TH + 2 * T;
    const int side_groups = T > 0 ? (rows + 7) >> 3 : 0;   // per side, 8 rows each
    const int items = rows + 2 * side_groups;              // wave-uniform loop: every lane reaches every __ballot
    for (int i = wave; i < items; i += RD_BLOCK / RW_WAVE) {
      if (i < rows) {
        const bool in = rd_inside(MODE, sel, ty0 - T + i, tx0 + lane, H, W, p.h, p.w, p.inv2H, p.inv2W, p.level);
        const unsigned long long word = __ballot(in);
        if (lane == 0) centre[i] = word;
      } else {
        const int j = i - rows, right = j >= side_groups, g = right ? j - side_groups : j;
        const int row = g * 8 + (lane >> 3);
        const int x = (right ? tx0 + RD_TW : tx0 - RD_SIDE) + (lane & 7);
        const bool in = rd_inside(MODE, sel, ty0 - T + row, x, H, W, p.h, p.w, p.inv2H, p.inv2W, p.level);
        const unsigned long long word = __ballot(in);
        if (lane < 8 && g * 8 + lane < rows) side[right][g * 8 + lane] = (unsigned)(word >> (8 * lane)) & 0xffu;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      const unsigned long long c = centre[threadIdx.x];
      unsigned long long g = c;
      if (T > 0) {
        const unsigned long long l = side[0][threadIdx.x], r = side[1][threadIdx.x];
        for (int d = 1; d <= T; ++d) g |= (c << d) | (l >> (RD_SIDE - d)) | (c >> d) | (r << (RD_TW - d));
      }
      grown[threadIdx.x] = g;
    }
    __syncthreads();
  }

  const unsigned bc = p.border_rgb;
  const int ic = p.inside_rgb;
  if constexpr (V == 4) {
    const int r = threadIdx.x >> 4, q = (threadIdx.x & 15) * 4;
    const int y = ty0 + r, x = tx0 + q;
    if (y >= H || x >= W) return;                          // W % 4 == 0: the four pixels are in or out together
    unsigned in4 = 0, border4 = 0;
    if constexpr (MODE != 0) {
      unsigned long long nb = 0;
      for (int j = 0; j <= 2 * T; ++j) nb |= grown[r + j];
      const unsigned long long c = centre[r + T];
      in4 = (unsigned)(c >> q) & 0xfu;
      border4 = (unsigned)(nb >> q) & ~in4 & 0xfu;
    } else {
      in4 = 0xfu;
    }
    const int o = y * W + x;
    const rw_f32x4 c0 = *reinterpret_cast<const rw_f32x4*>(src + o);
    const rw_f32x4 c1 = *reinterpret_cast<const rw_f32x4*>(src + hw + o);
    const rw_f32x4 c2 = *reinterpret_cast<const rw_f32x4*>(src + 2 * hw + o);
    unsigned b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = (in4 >> j) & 1u, border = (border4 >> j) & 1u;
      b[3 * j + 0] = rd_blend(c0[j], in, border, bc & 0xffu, ic < 0 ? -1 : ic & 0xff, p.outside_bright);
      b[3 * j + 1] = rd_blend(c1[j], in, border, (bc >> 8) & 0xffu, ic < 0 ? -1 : (ic >> 8) & 0xff, p.outside_bright);
      b[3 * j + 2] = rd_blend(c2[j], in, border, (bc >> 16) & 0xffu, ic < 0 ? -1 : (ic >> 16) & 0xff, p.outside_bright);
    }
    unsigned* d32 = reinterpret_cast<unsigned*>(dst + 3 * o);       // 12 o bytes past a 4-byte aligned base
#pragma unroll
    for (int k = 0; k < 3; ++k) d32[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int step = 0; step < RD_TH * RD_TW / RD_BLOCK; ++step) {
      const int i = step * RD_BLOCK + threadIdx.x;
      const int r = i >> 6, q = i & 63;
      const int y = ty0 + r, x = tx0 + q;
      if (y >= H || x >= W) continue;
      bool in = true, border = false;
      if constexpr (MODE != 0) {
        unsigned long long nb = 0;
        for (int j = 0; j <= 2 * T; ++j) nb |= grown[r + j];
        in = (centre[r + T] >> q) & 1u;
        border = !in && ((nb >> q) & 1u);
      }
      const int o = y * W + x;
      dst[3 * o + 0] = (uint8_t)rd_blend(src[o], in, border, bc & 0xffu, ic < 0 ? -1 : ic & 0xff, p.outside_bright);
      dst[3 * o + 1] = (uint8_t)rd_blend(src[hw + o], in, border, (bc >> 8) & 0xffu, ic < 0 ? -1 : (ic >> 8) & 0xff,
                                         p.outside_bright);
      dst[3 * o + 2] = (uint8_t)rd_blend(src[2 * hw + o], in, border, (bc >> 16) & 0xffu, ic < 0 ? -1 : (ic >> 16) & 0xff,
                                         p.outside_bright);
    }
  }
}

template <int MODE>
static void rd_launch(bool vec4, unsigned blocks, hipStream_t s, const rd_problem& p) {
  if (vec4) hipLaunchKernelGGL((render_bytes_kernel<MODE, 4>), dim3(blocks), dim3(RD_BLOCK), 0, s, p);
  else hipLaunchKernelGGL((render_bytes_kernel<MODE, 1>), dim3(blocks), dim3(RD_BLOCK), 0, s, p);
}

extern "C" int rw_render_bytes_f32(const float* image, const void* selector, uint8_t* out, int64_t images, int height,
                                   int width, int mode, int sel_height, int sel_width, float level, int thickness,
                                   uint32_t border_rgb, int32_t inside_rgb, float outside_bright, rw_stream_t stream) {
  RW_CHECK_ARG(image && out && images >= 1 && height >= 1 && width >= 1);
  RW_CHECK_ARG(3 * (int64_t)height * width <= INT32_MAX);  // offsets inside an image are 32-bit; image bases are 64-bit
  RW_CHECK_ARG(mode >= 0 && mode <= 2 && (mode == 0 || selector));
  RW_CHECK_ARG(mode != 2 || (sel_height == height && sel_width == width));
  RW_CHECK_ARG(thickness >= 0 && thickness <= RW_RENDER_MAX_THICKNESS);
  RW_CHECK_ARG(isfinite(outside_bright));
  if (mode == 1) {
    if (sel_height < 2 || sel_width < 2) return RW_ERR_UNSUPPORTED;   // the host grid degenerates to a constant there
    // (2y + 1) h - H and the offsets inside a heat map are 32-bit
    RW_CHECK_ARG((int64_t)sel_height * sel_width <= INT32_MAX && (2 * (int64_t)height + 1) * sel_height <= INT32_MAX &&
                 (2 * (int64_t)width + 1) * sel_width <= INT32_MAX);
  }
  rd_problem p;
  p.image = image; p.sel = selector; p.out = out;
  p.H = height; p.W = width; p.h = mode == 1 ? sel_height : 0; p.w = mode == 1 ? sel_width : 0;
  p.tiles_x = (int)rw_cdiv(width, RD_TW);
  const int64_t tiles = (int64_t)p.tiles_x * rw_cdiv(height, RD_TH);
  RW_CHECK_ARG(tiles <= INT32_MAX && images * tiles <= INT32_MAX);     // the grid's x extent
  p.tiles_per_image = (int)tiles;
  p.thickness = thickness;
  p.level = level;
  p.inv2H = (float)(1.0 / (2.0 * height)); p.inv2W = (float)(1.0 / (2.0 * width));
  p.outside_bright = outside_bright;
  p.border_rgb = border_rgb & 0xffffffu;
  p.inside_rgb = inside_rgb < 0 ? -1 : (inside_rgb & 0xffffff);
  const bool vec4 = width % 4 == 0 && ((uintptr_t)image % 16) == 0 && ((uintptr_t)out % 4) == 0;
  const unsigned blocks = (unsigned)(images * tiles);
  hipStream_t s = rw_s(stream);
  switch (mode) {
    case 0: rd_launch<0>(vec4, blocks, s, p); break;
    case 1: rd_launch<1>(vec4, blocks, s, p); break;
    default: rd_launch<2>(vec4, blocks, s, p); break;
  }
  return RW_LAUNCH_RESULT();
}
