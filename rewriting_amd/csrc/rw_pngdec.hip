// PNG decoding on gfx950: the way back from rw_png.hip -- what PIL.Image.open(...).convert('RGB') does per file on the
// host (metrics/distances.py:67-70) for a batch of files of one shape, whose raw deflate streams lie in one device
// buffer.  The format, the status codes and what the host does (chunks, CRC-32, the zlib header and trailer) are in
// include/rewriting_hip.h.
//
//   rw_png_inflate_u8: ONE WAVE PER STREAM (a workgroup is one wave, so its barriers cannot wait on anyone).  Every lane
//     runs the inflate of rw_inflate_core.h on the same state: the symbol decode is wave-uniform, branch by branch.  The
//     lanes share out what is wide:
//       * the coded bytes come through a 2 KiB ring in LDS that the wave fills 1 KiB at a time (16 bytes a lane, dword
//         loads where a dword lies inside the span, guarded byte loads at its two ends: nothing outside the span is read);
//       * the fast decode tables are filled 64 symbols at a time;
//       * a match of length n at distance d is out[p + i] = out[p - d + (i mod d)], i < n: all sources lie before p, so
//         the 64 lanes copy it in ceil(n / 64) rounds, overlapping or not;
//       * the last 32 KiB of output live in LDS as a ring (every index masked); each finished KiB leaves it as one
//         dword x4 store per lane, and its Adler sums are taken from those registers;
//       * stored blocks are copied from the coded buffer 64 bytes at a time.
//     Nothing the kernel writes to global memory is read by it: `coded` and `span` are read only, `stream` and `status`
//     written only.  Every store is a plain vector store below `expect` (the core refuses output beyond it before the
//     sink sees it).  LDS: 32 KiB window + 2 KiB ring + 2 x 2 KiB fast tables + 1.2 KiB of counts, symbols and
//     lengths = 40 064 bytes, four streams per CU.
//   rw_png_unfilter_u8: one wave per image, a diagonal wavefront over bands of 64 rows: lane r works on row band + r, one
//     pixel behind lane r - 1, so the pixel above comes from the neighbour lane by a shuffle, the pixel above left is
//     last step's shuffle, the pixel to the left is the lane's own last result.  The last row of a band waits in LDS
//     (4 W bytes) for lane 0 of the next band.  A band takes W + 63 steps.  The filtered rows are read straight from
//     `stream` (one step ahead of their use), not staged.
#include "rw_common.h"
#include "rw_inflate_core.h"

#define PD_WINDOW 32768u
#define PD_RING 2048u
#define PD_CHUNK 1024u                                     // ring fill and window flush: 64 lanes x 16 bytes
#define PD_ADLER 65521u
#define PD_MAX_WIDTH 16384                                 // the band's last row in LDS: 4 W bytes <= 64 KiB

static_assert(PD_CHUNK == RW_WAVE * 16 && PD_RING == 2 * PD_CHUNK, "a chunk is one dword x4 per lane");

struct pd_lanes {
  int lane;
  __device__ __forceinline__ int first() const { return lane; }
  __device__ __forceinline__ int step() const { return RW_WAVE; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }      // the workgroup is this wave
  __device__ __forceinline__ uint32_t uniform(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
};

// The coded bytes of one stream.  Positions relative to the dword below `begin`: rel = pos + skew; the ring holds
// rel in [loaded - PD_RING, loaded) (after a jump: [loaded - PD_CHUNK, loaded)); the core reads forwards, and goes back at
// most 8 bytes, never across a jump.
struct pd_source {
  const uint8_t* begin;
  uint64_t n;
  uint8_t* ring;
  uint32_t skew;
  uint64_t loaded;
  int lane;

  __device__ __forceinline__ uint64_t size() const { return n; }
  __device__ __forceinline__ const uint8_t* data() const { return begin; }

  __device__ __forceinline__ void fill() {                 // rel in [loaded, loaded + PD_CHUNK)
    const uint8_t* base = begin - skew;                    // dword aligned
    const uint64_t lo = skew, hi = skew + n;               // the rel positions that exist
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t rel = loaded + (uint64_t)lane * 16 + 4 * j;
      unsigned v = 0;
      if (rel >= lo && rel + 4 <= hi) {
        v = *reinterpret_cast<const unsigned*>(base + rel);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (rel + k >= lo && rel + k < hi) v |= (unsigned)base[rel + k] << (8 * k);
      }
      w[j] = v;
    }
    __syncthreads();
    *reinterpret_cast<rw_u32x4*>(ring + ((loaded + (uint64_t)lane * 16) & (PD_RING - 1))) = rw_u32x4{w[0], w[1], w[2], w[3]};
    __syncthreads();
    loaded += PD_CHUNK;
  }

  __device__ __forceinline__ uint32_t bytes(uint64_t pos, uint32_t take) {         // take in 1 .. 4, pos + take <= n
    const uint64_t rel = pos + skew;
    while (rel + take > loaded) {                          // twice at most
      if (rel >= loaded + PD_CHUNK) loaded = rel & ~(uint64_t)(PD_CHUNK - 1);
      fill();
    }
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
      if (k < take) word |= (uint32_t)ring[(rel + k) & (PD_RING - 1)] << (8 * k);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
  }
};

// The output of one stream: the window ring in LDS, the global stream behind it.  pos <= expect always (the core asks
// produced() first), so everything below `pos` may be stored.
struct pd_sink {
  uint8_t* win;
  uint8_t* out;            // 16-byte aligned
  uint32_t pos, flushed;   // flushed: a multiple of PD_CHUNK
  uint32_t s1, s2;         // sum d_k and sum (pos - k) d_k mod 65521 over what was flushed: the fold of pngcode.adler_fold
  int lane;

  __device__ __forceinline__ uint64_t produced() const { return pos; }

  __device__ __forceinline__ void fold(unsigned n, unsigned c1, unsigned c2) {      // c2 < 2^28, n <= 1024
    s2 = (s2 + n * s1 + c2 % PD_ADLER) % PD_ADLER;
    s1 = (s1 + c1) % PD_ADLER;
  }
  __device__ __forceinline__ void flush() {                // whole chunks that are complete
    while (pos - flushed >= PD_CHUNK) {
      __syncthreads();
      const unsigned at = flushed + (unsigned)lane * 16;
      const rw_u32x4 v = *reinterpret_cast<const rw_u32x4*>(win + (at & (PD_WINDOW - 1)));
      *reinterpret_cast<rw_u32x4*>(out + at) = v;
      unsigned c1 = 0, c2 = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned d = (v[e >> 2] >> (8 * (e & 3))) & 0xffu;
        c1 += d;
        c2 += (PD_CHUNK - ((unsigned)lane * 16 + e)) * d;
      }
      fold(PD_CHUNK, rw_wave_sum(c1), rw_wave_sum(c2));
      flushed += PD_CHUNK;
    }
  }
  __device__ __forceinline__ void finish() {               // the rest, byte by byte: fewer than PD_CHUNK
    __syncthreads();
    const unsigned m = pos - flushed;
    unsigned c1 = 0, c2 = 0;
    for (unsigned i = lane; i < m; i += RW_WAVE) {
      const unsigned d = win[(flushed + i) & (PD_WINDOW - 1)];
      out[flushed + i] = (uint8_t)d;
      c1 += d;
      c2 += (m - i) * d;
    }
    fold(m, rw_wave_sum(c1), rw_wave_sum(c2));
    flushed = pos;
  }

  __device__ __forceinline__ void literal(uint8_t byte) {
    if (lane == 0) win[pos & (PD_WINDOW - 1)] = byte;
    ++pos;
    flush();
  }
  __device__ __forceinline__ void copy(uint32_t distance, uint32_t length) {        // 1 <= distance <= pos, length <= 258
    __syncthreads();                                       // lane 0's literals are in the window
    for (uint32_t i = lane; i < length; i += RW_WAVE) {
      const uint32_t from = pos - distance + (distance >= length ? i : i % distance);
      const uint8_t v = win[from & (PD_WINDOW - 1)];       // a lane reads before it writes; no write of this copy is a source
      win[(pos + i) & (PD_WINDOW - 1)] = v;
    }
    pos += length;
    flush();
  }
  __device__ __forceinline__ void stored(const uint8_t* src, uint32_t n) {          // src: n bytes inside the span
    while (n) {
      const uint32_t m = n < PD_CHUNK ? n : PD_CHUNK;
      for (uint32_t i = lane; i < m; i += RW_WAVE) win[(pos + i) & (PD_WINDOW - 1)] = src[i];
      pos += m;
      src += m;
      n -= m;
      flush();
    }
  }
};

struct pd_inflate_problem {
  const uint8_t* coded;
  const uint64_t* span;    // (images, 2): offset, length
  uint8_t* stream;         // (images, stride)
  uint32_t* status;        // (images, 4)
  int64_t stride;
  uint32_t expect;
};

__global__ void __launch_bounds__(RW_WAVE) png_inflate_kernel(const pd_inflate_problem p) {
  __shared__ __attribute__((aligned(16))) uint8_t win[PD_WINDOW];
  __shared__ __attribute__((aligned(16))) uint8_t ring[PD_RING];
  __shared__ uint16_t fast[2][1 << RW_INF_FAST_BITS];
  __shared__ uint16_t small[2][3][RW_INF_MAX_BITS + 1];
  __shared__ uint16_t lit_symbol[RW_INF_MAX_LIT], dist_symbol[RW_INF_MAX_DIST];
  __shared__ uint8_t lengths[RW_INF_MAX_LENGTHS];

  const int lane = threadIdx.x;
  const int64_t img = blockIdx.x;
  rw_inflate::Work work;
  work.lit = rw_inflate::Table{fast[0], small[0][0], small[0][1], small[0][2], lit_symbol};
  work.dist = rw_inflate::Table{fast[1], small[1][0], small[1][1], small[1][2], dist_symbol};
  work.lengths = lengths;

  pd_source source;
  source.begin = p.coded + p.span[2 * img];
  source.n = p.span[2 * img + 1];
  source.ring = ring;
  source.skew = (uint32_t)((uintptr_t)source.begin & 3u);
  source.loaded = 0;
  source.lane = lane;
  pd_sink sink;
  sink.win = win;
  sink.out = p.stream + img * p.stride;
  sink.pos = sink.flushed = sink.s1 = sink.s2 = 0;
  sink.lane = lane;
  pd_lanes lanes{lane};

  const int code = rw_inflate::inflate(source, sink, work, lanes, (uint64_t)p.expect);
  sink.finish();
  if (lane < 4) {
    const uint32_t v = lane == 0 ? (uint32_t)code : lane == 1 ? sink.pos : lane == 2 ? sink.s1 : sink.s2;
    p.status[4 * img + lane] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pd_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (unsigned)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

struct pd_unfilter_problem {
  const uint8_t* stream;   // (images, stride): H rows of a type byte and BPP W bytes
  uint32_t* status;        // (images, 4): [0] read here; RW_PNG_BAD_FILTER written
  uint8_t* out;            // (images, H, W, 3)
  int64_t stride;
  int H, W;
};

template <int BPP>
__device__ __forceinline__ unsigned pd_load_pixel(const uint8_t* at) {
  unsigned v = 0;
#pragma unroll
  for (int c = 0; c < BPP; ++c) v |= (unsigned)at[c] << (8 * c);
  return v;
}

template <int BPP>
__global__ void __launch_bounds__(RW_WAVE) png_unfilter_kernel(const pd_unfilter_problem p) {
  extern __shared__ unsigned pd_above[];                   // W pixels: the last row of the band before this one
  const int lane = threadIdx.x;
  const int64_t img = blockIdx.x;
  uint8_t* dst = p.out + img * p.H * p.W * 3;
  if (p.status[4 * img] != RW_PNG_OK) {                    // wave-uniform: the stream is not the image's; zeros
    const int64_t n = (int64_t)p.H * p.W * 3;
    for (int64_t i = lane; i < n; i += RW_WAVE) dst[i] = 0;
    return;
  }
  const uint8_t* src = p.stream + img * p.stride;
  const int64_t row_len = 1 + (int64_t)BPP * p.W;
  bool bad = false;
  for (int band = 0; band < p.H; band += RW_WAVE) {
    const int y = band + lane;
    const bool active = y < p.H;
    const uint8_t* row = src + (active ? y : 0) * row_len;
    int type = active ? row[0] : 0;
    if (type > 4) { bad = true; type = 0; }
    unsigned mine = 0, left = 0, up = 0, upleft = 0;
    unsigned raw = (active && lane == 0) ? pd_load_pixel<BPP>(row + 1) : 0u;        // pixel 0 of lane 0: step 0
    const int steps = p.W + min(RW_WAVE, p.H - band) - 1;
    for (int t = 0; t < steps; ++t) {
      const int x = t - lane;
      unsigned above = __shfl_up(mine, 1, 64);             // lane - 1 finished pixel x of the row above in step t - 1
      if (lane == 0) above = (band > 0 && x < p.W) ? pd_above[x] : 0u;
      upleft = up;
      up = above;
      const bool work = active && x >= 0 && x < p.W;
      const unsigned cur = raw;
      // the bytes of the next step's pixel, ahead of their use
      const int xn = x + 1;
      if (active && xn >= 0 && xn < p.W) raw = pd_load_pixel<BPP>(row + 1 + (int64_t)xn * BPP);
      if (work) {
        if (x == 0) { left = 0; upleft = 0; }
        unsigned v = 0;
#pragma unroll
        for (int c = 0; c < BPP; ++c) {
          const unsigned a = (left >> (8 * c)) & 0xffu, b = (up >> (8 * c)) & 0xffu, cc = (upleft >> (8 * c)) & 0xffu;
          unsigned pred = 0;
          if (type == 1) pred = a;
          else if (type == 2) pred = b;
          else if (type == 3) pred = (a + b) >> 1;
          else if (type == 4) pred = pd_paeth((int)a, (int)b, (int)cc);
          v |= ((((cur >> (8 * c)) & 0xffu) + pred) & 0xffu) << (8 * c);
        }
        mine = left = v;
        uint8_t* px = dst + ((int64_t)y * p.W + x) * 3;
        if (BPP == 1) { px[0] = px[1] = px[2] = (uint8_t)v; }                       // grey to three channels
        else { px[0] = (uint8_t)v; px[1] = (uint8_t)(v >> 8); px[2] = (uint8_t)(v >> 16); }   // alpha, if any, is dropped
        if (lane == RW_WAVE - 1) pd_above[x] = v;
      }
    }
    __syncthreads();                                       // the band's last row is whole before lane 0 reads it
  }
  if (bad) p.status[4 * img] = RW_PNG_BAD_FILTER;
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int rw_png_inflate_u8(const uint8_t* coded, const uint64_t* span, uint8_t* stream, int64_t stride, int64_t expect,
                                 uint32_t* status, int64_t images, rw_stream_t stream_) {
  RW_CHECK_ARG(coded && span && stream && status);
  RW_CHECK_ARG(images >= 1 && images <= INT32_MAX);
  if (expect < 1 || expect > INT32_MAX) return RW_ERR_UNSUPPORTED;
  RW_CHECK_ARG(stride >= expect && stride % 16 == 0 && rw_aligned16(stream));
  pd_inflate_problem p;
  p.coded = coded; p.span = span; p.stream = stream; p.status = status; p.stride = stride; p.expect = (uint32_t)expect;
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)images), dim3(RW_WAVE), 0, rw_s(stream_), p);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_png_unfilter_u8(const uint8_t* stream, int64_t stride, uint32_t* status, uint8_t* out, int64_t images,
                                  int height, int width, int channels, rw_stream_t stream_) {
  RW_CHECK_ARG(stream && status && out);
  RW_CHECK_ARG(images >= 1 && images <= INT32_MAX);
  if (channels != 1 && channels != 3 && channels != 4) return RW_ERR_UNSUPPORTED;
  if (height < 1 || width < 1 || width > PD_MAX_WIDTH) return RW_ERR_UNSUPPORTED;
  const int64_t len = (int64_t)height * (1 + (int64_t)channels * width);
  if (len > INT32_MAX) return RW_ERR_UNSUPPORTED;
  RW_CHECK_ARG(stride >= len);
  pd_unfilter_problem p;
  p.stream = stream; p.status = status; p.out = out; p.stride = stride; p.H = height; p.W = width;
  const dim3 grid((unsigned)images), block(RW_WAVE);
  const size_t lds = 4 * (size_t)width;
  hipStream_t s = rw_s(stream_);
  if (channels == 1) hipLaunchKernelGGL(png_unfilter_kernel<1>, grid, block, lds, s, p);
  else if (channels == 3) hipLaunchKernelGGL(png_unfilter_kernel<3>, grid, block, lds, s, p);
  else hipLaunchKernelGGL(png_unfilter_kernel<4>, grid, block, lds, s, p);
  return RW_LAUNCH_RESULT();
}
