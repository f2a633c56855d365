// PNG encoding on gfx950: the per-byte work of renormalize.as_url's img.save(format='png') (utils/renormalize.py:22-32)
// and of SaveImageWorker.work (utils/imgsave.py:58-66) for a batch of (B, H, W, 3) uint8 images that are already on the
// device -- what rw_render_bytes_f32 leaves.  The format and what the host adds are in include/rewriting_hip.h.
//
// The filtered scanline stream of an image (H rows of 1 + 3 W bytes) is cut into segments of PG_SEG bytes; an image's
// stream is kept padded to whole segments, so every segment starts 16-byte aligned.
//   rw_png_filter_u8, three launches:
//     1. one WAVE per row: the five sums of |residual as a signed byte| (libpng's heuristic), the smallest wins, ties to
//        the lowest type -> row_type (B, H).  The prior row is zero for row 0.
//     2. one workgroup per segment: a thread filters 16 consecutive stream bytes per step and stores them as one dword x4;
//        the byte counts go to one LDS histogram per wave (LDS atomics), the Adler-32 sums of the segment are reduced in
//        the workgroup.  It stores its 256 counts and its (s1, s2) plainly, into its own slots.
//     3. one workgroup per image adds the segments' counts in order.
//   rw_png_encode_u8: one workgroup per segment writes the whole byte-aligned deflate block of the segment.  A thread
//     codes PG_RUN consecutive bytes; its bit offset comes from a workgroup scan of the bit counts; the bits are ORed into
//     a zeroed LDS image of the block (words that two threads share: LDS atomics; words inside a thread's run: plain
//     stores) and the image is stored with dword x4 stores into the segment's own slot of PG_CAP bytes.
//   rw_png_compact_u8: a scan of the segment lengths (one workgroup, 64-bit offsets) and a gather of every slot to its
//     offset in one contiguous buffer, behind a head of (length, s1, s2) per segment.
// No global atomics, nothing zeroed first, every global byte has one writer.  All of it is integer work:
// the same bytes on every run, alone or in a batch.
#include "rw_common.h"

#define PG_BLOCK 256
#define PG_SEG 16384                                       // stream bytes per deflate block
#define PG_RUN (PG_SEG / PG_BLOCK)                         // consecutive bytes a thread codes: 64 = four dword x4
#define PG_HDR_BYTES 256                                   // room for the dynamic block header: at most 1880 bits
#define PG_CAP (PG_SEG * 15 / 8 + PG_HDR_BYTES + 16)       // a coded segment: header, 15 bits a byte, the 7-byte tail
#define PG_TABLE_WORDS (1 + 257 + PG_HDR_BYTES / 4)        // header bits; code | length << 16 of 0 .. 256; the header
#define PG_ADLER 65521u

static_assert(PG_CAP % 16 == 0 && PG_RUN == 64, "the slots are stored as dword x4, a run is four of them");

// ---------------------------------------------------------------------------------------------------------------------
// the filters of the PNG specification (section 9): x the byte, a the byte three to the left, b above, c above left
__device__ __forceinline__ unsigned pg_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (unsigned)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}
__device__ __forceinline__ unsigned pg_residual(int type, unsigned x, unsigned a, unsigned b, unsigned c) {
  unsigned pred = 0;
  if (type == 1) pred = a;
  else if (type == 2) pred = b;
  else if (type == 3) pred = (a + b) >> 1;
  else if (type == 4) pred = pg_paeth((int)a, (int)b, (int)c);
  return (x - pred) & 0xffu;
}
__device__ __forceinline__ unsigned pg_abs8(unsigned r) { return r < 128u ? r : 256u - r; }

// the neighbours of byte i of a row; prev == nullptr: row 0
__device__ __forceinline__ void pg_neighbours(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int i,
                                              unsigned& x, unsigned& a, unsigned& b, unsigned& c) {
  x = cur[i];
  a = i >= 3 ? cur[i - 3] : 0u;
  b = prev ? prev[i] : 0u;
  c = (prev && i >= 3) ? prev[i - 3] : 0u;
}

struct pg_problem {
  const uint8_t* image;    // (B, H, W, 3)
  uint8_t* row_type;       // (B, H)
  uint8_t* stream;         // (B, nseg * PG_SEG)
  unsigned* hist_part;     // (B, nseg, 256)
  unsigned* hist;          // (B, 256)
  unsigned* adler;         // (B, nseg, 2)
  int64_t rows;            // B * H
  int H, row_bytes;        // 3 W
  int stream_len, nseg;    // H (1 + 3 W) < 2^31
};

__global__ void __launch_bounds__(PG_BLOCK) png_row_type_kernel(const pg_problem p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (PG_BLOCK / RW_WAVE) + (threadIdx.x >> 6);
  if (r >= p.rows) return;                                 // wave-uniform
  const int y = (int)(r % p.H);
  const uint8_t* cur = p.image + r * p.row_bytes;          // rows of all images lie back to back
  const uint8_t* prev = y > 0 ? cur - p.row_bytes : nullptr;
  unsigned long long sum[5] = {0, 0, 0, 0, 0};
  for (int i = lane; i < p.row_bytes; i += RW_WAVE) {
    unsigned x, a, b, c;
    pg_neighbours(cur, prev, i, x, a, b, c);
#pragma unroll
    for (int t = 0; t < 5; ++t) sum[t] += pg_abs8(pg_residual(t, x, a, b, c));
  }
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum[t] += __shfl_xor(sum[t], off, 64);
  int best = 0;
#pragma unroll
  for (int t = 1; t < 5; ++t)
    if (sum[t] < sum[best]) best = t;
  if (lane == 0) p.row_type[r] = (uint8_t)best;
}

__global__ void __launch_bounds__(PG_BLOCK) png_filter_kernel(const pg_problem p) {
  __shared__ unsigned counts[PG_BLOCK / RW_WAVE][256];
  __shared__ unsigned red[2][PG_BLOCK / RW_WAVE];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int img = blockIdx.x / p.nseg, seg = blockIdx.x - img * p.nseg;
  const int p0 = seg * PG_SEG;                             // < stream_len < 2^31
  const int n = min(PG_SEG, p.stream_len - p0);
  const int row_len = 1 + p.row_bytes;
  const uint8_t* image = p.image + (int64_t)img * p.H * p.row_bytes;
  const uint8_t* types = p.row_type + (int64_t)img * p.H;
  uint8_t* dst = p.stream + (int64_t)blockIdx.x * PG_SEG;

#pragma unroll
  for (int k = 0; k < PG_BLOCK / RW_WAVE; ++k) counts[k][tid] = 0;
  __syncthreads();

  unsigned s1 = 0, s2 = 0;                                 // s2 <= 64 * 16384 * 255 < 2^32
  for (int q = tid * 16; q < n; q += PG_BLOCK * 16) {
    int y = (p0 + q) / row_len;
    int j = (p0 + q) - y * row_len;                        // 0: the type byte, else byte j - 1 of the row
    int type = types[y];
    unsigned word[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (q + e < n) {
        unsigned v;
        if (j == 0) {
          v = (unsigned)type;
        } else {
          const uint8_t* cur = image + (int64_t)y * p.row_bytes;
          unsigned x, a, b, c;
          pg_neighbours(cur, y > 0 ? cur - p.row_bytes : nullptr, j - 1, x, a, b, c);
          v = pg_residual(type, x, a, b, c);
        }
        word[e >> 2] |= v << (8 * (e & 3));
        atomicAdd(&counts[wave][v], 1u);
        s1 += v;
        s2 += (unsigned)(n - (q + e)) * v;
        if (++j == row_len) {
          j = 0;
          ++y;
          if (y < p.H) type = types[y];
        }
      }
    }
    *reinterpret_cast<rw_u32x4*>(dst + q) = rw_u32x4{word[0], word[1], word[2], word[3]};
  }
  s2 %= PG_ADLER;                                          // 256 of them sum below 2^24
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  if ((tid & 63) == 0) { red[0][wave] = s1; red[1][wave] = s2; }
  __syncthreads();                                         // the counts are complete as well
  unsigned total = 0;
#pragma unroll
  for (int k = 0; k < PG_BLOCK / RW_WAVE; ++k) total += counts[k][tid];
  p.hist_part[(int64_t)blockIdx.x * 256 + tid] = total;
  if (tid < 2) {
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < PG_BLOCK / RW_WAVE; ++k) v += red[tid][k];
    p.adler[(int64_t)blockIdx.x * 2 + tid] = v % PG_ADLER;
  }
}

__global__ void __launch_bounds__(PG_BLOCK) png_hist_sum_kernel(const pg_problem p) {
  const unsigned* part = p.hist_part + (int64_t)blockIdx.x * p.nseg * 256 + threadIdx.x;
  unsigned total = 0;                                      // the stream has fewer than 2^31 bytes
  for (int s = 0; s < p.nseg; ++s) total += part[(int64_t)s * 256];
  p.hist[(int64_t)blockIdx.x * 256 + threadIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------------------------------
struct pg_encode_problem {
  const uint8_t* stream;   // (B, nseg * PG_SEG)
  const unsigned* table;   // (B, PG_TABLE_WORDS)
  uint8_t* coded;          // (B, nseg, PG_CAP)
  unsigned* lengths;       // (B, nseg)
  int stream_len, nseg;
};

// OR `bits` (at most 32 of them) into the LDS image at bit position pos; the words may be shared with other threads
__device__ __forceinline__ void pg_or_bits(unsigned* image, unsigned pos, unsigned bits) {
  const unsigned long long v = (unsigned long long)bits << (pos & 31);
  atomicOr(&image[pos >> 5], (unsigned)v);
  if (v >> 32) atomicOr(&image[(pos >> 5) + 1], (unsigned)(v >> 32));
}

// Dynamic LDS only (its base stays 16-byte aligned): the block's image, PG_CAP bytes; the code table; the wave totals.
#define PG_LDS_TABLE PG_CAP
#define PG_LDS_RED (PG_LDS_TABLE + 272 * 4)
#define PG_LDS_BYTES (PG_LDS_RED + 16 * 4)
static_assert(PG_LDS_TABLE % 16 == 0 && PG_LDS_RED % 16 == 0 && PG_LDS_BYTES % 16 == 0, "every carve at 16 bytes");

__global__ void __launch_bounds__(PG_BLOCK) png_encode_kernel(const pg_encode_problem p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pg_smem[];
  unsigned* image = reinterpret_cast<unsigned*>(pg_smem);
  unsigned* table = reinterpret_cast<unsigned*>(pg_smem + PG_LDS_TABLE);
  unsigned* red = reinterpret_cast<unsigned*>(pg_smem + PG_LDS_RED);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x / p.nseg, seg = blockIdx.x - img * p.nseg;
  const int n = min(PG_SEG, p.stream_len - seg * PG_SEG);
  const unsigned* tab = p.table + (int64_t)img * PG_TABLE_WORDS;
  const unsigned hdr_bits = min(tab[0], (unsigned)(PG_HDR_BYTES * 8));
  for (int i = tid; i < 257; i += PG_BLOCK) table[i] = tab[1 + i];

  // this thread's run: bytes tid * 64 .. of the segment, m of them
  const int first = tid * PG_RUN;
  const int m = min(max(n - first, 0), PG_RUN);
  const uint8_t* src = p.stream + (int64_t)blockIdx.x * PG_SEG + first;
  unsigned w[PG_RUN / 4];
#pragma unroll
  for (int k = 0; k < PG_RUN / 16; ++k) {
    rw_u32x4 v = {0, 0, 0, 0};
    if (16 * k < m) v = *reinterpret_cast<const rw_u32x4*>(src + 16 * k);   // the filter pass wrote the whole 16 bytes
    w[4 * k] = v[0]; w[4 * k + 1] = v[1]; w[4 * k + 2] = v[2]; w[4 * k + 3] = v[3];
  }
  __syncthreads();

  unsigned bits = 0;
#pragma unroll
  for (int e = 0; e < PG_RUN; ++e)
    if (e < m) bits += (table[(w[e >> 2] >> (8 * (e & 3))) & 0xffu] >> 16) & 15u;

  // exclusive scan of the bit counts over the workgroup (a thread has at most 960 bits, the workgroup 245 760)
  unsigned incl = bits;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < PG_BLOCK / RW_WAVE; ++k) {
    if (k < wave) before += red[k];
    total += red[k];
  }
  const unsigned start = hdr_bits + before + incl - bits;

  // the block: header, literals, end-of-block, then the empty stored block `000`, pad, 00 00 FF FF
  const unsigned eob = table[256];
  const unsigned end_bits = hdr_bits + total + ((eob >> 16) & 15u) + 3;
  const unsigned tail = (end_bits + 7) >> 3;               // byte offset of 00 00 FF FF
  const unsigned seg_len = tail + 4;                       // <= PG_CAP - 9
  const unsigned chunks = (seg_len + 15) >> 4;
  for (unsigned c = tid; c < chunks; c += PG_BLOCK) reinterpret_cast<rw_u32x4*>(image)[c] = rw_u32x4{0, 0, 0, 0};
  __syncthreads();

  const unsigned hdr_words = (hdr_bits + 31) >> 5;
  for (unsigned i = tid; i < hdr_words; i += PG_BLOCK) {
    unsigned v = tab[258 + i];
    if (i == hdr_words - 1 && (hdr_bits & 31)) v &= (1u << (hdr_bits & 31)) - 1u;
    atomicOr(&image[i], v);
  }
  {
    unsigned long long acc = 0;
    unsigned fill = start & 31, word = start >> 5;
    bool shared = true;                                    // the first word may hold a neighbour's bits below `fill`
#pragma unroll
    for (int e = 0; e < PG_RUN; ++e) {
      if (e < m) {
        const unsigned entry = table[(w[e >> 2] >> (8 * (e & 3))) & 0xffu];
        acc |= (unsigned long long)(entry & 0xffffu) << fill;
        fill += (entry >> 16) & 15u;
        if (fill >= 32) {
          if (shared) atomicOr(&image[word], (unsigned)acc);
          else image[word] = (unsigned)acc;                // bits 0 .. 31 of this word are all this thread's
          shared = false;
          ++word;
          acc >>= 32;
          fill -= 32;
        }
      }
    }
    if (acc) atomicOr(&image[word], (unsigned)acc);
  }
  if (tid == 0) {
    pg_or_bits(image, hdr_bits + total, eob & 0xffffu);
    atomicOr(&image[(tail + 2) >> 2], 0xffu << (8 * ((tail + 2) & 3)));
    atomicOr(&image[(tail + 3) >> 2], 0xffu << (8 * ((tail + 3) & 3)));
    p.lengths[blockIdx.x] = seg_len;
  }
  __syncthreads();
  rw_u32x4* dst = reinterpret_cast<rw_u32x4*>(p.coded + (int64_t)blockIdx.x * PG_CAP);
  for (unsigned c = tid; c < chunks; c += PG_BLOCK) dst[c] = reinterpret_cast<const rw_u32x4*>(image)[c];
}

// ---------------------------------------------------------------------------------------------------------------------
// offsets[i] = lengths[0] + ... + lengths[i - 1], by one workgroup: a thread sums a run, thread 0 scans the 256 sums
__global__ void __launch_bounds__(PG_BLOCK) png_scan_kernel(const unsigned* __restrict__ lengths,
                                                            unsigned long long* __restrict__ offsets, int64_t n) {
  __shared__ unsigned long long sums[PG_BLOCK];
  const int64_t per = (n + PG_BLOCK - 1) / PG_BLOCK;
  const int64_t lo = min((int64_t)threadIdx.x * per, n), hi = min(lo + per, n);
  unsigned long long s = 0;
  for (int64_t i = lo; i < hi; ++i) s += lengths[i];
  sums[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int k = 0; k < PG_BLOCK; ++k) { const unsigned long long v = sums[k]; sums[k] = run; run += v; }
  }
  __syncthreads();
  s = sums[threadIdx.x];
  for (int64_t i = lo; i < hi; ++i) { offsets[i] = s; s += lengths[i]; }
}

// one workgroup per segment: its bytes to packed_bytes + offset, its (length, s1, s2) to the head.  A segment that
// would pass `capacity` is not copied (the host sees that from the lengths).
__global__ void __launch_bounds__(PG_BLOCK) png_gather_kernel(const uint8_t* __restrict__ coded,
                                                              const unsigned* __restrict__ lengths,
                                                              const unsigned* __restrict__ adler,
                                                              const unsigned long long* __restrict__ offsets,
                                                              unsigned* __restrict__ head, uint8_t* __restrict__ bytes,
                                                              int64_t capacity) {
  const int tid = threadIdx.x;
  const unsigned len = min(lengths[blockIdx.x], (unsigned)PG_CAP);
  const unsigned long long off = offsets[blockIdx.x];
  if (tid == 0) head[3 * (int64_t)blockIdx.x] = len;
  if (tid == 1) head[3 * (int64_t)blockIdx.x + 1] = adler[2 * (int64_t)blockIdx.x];
  if (tid == 2) head[3 * (int64_t)blockIdx.x + 2] = adler[2 * (int64_t)blockIdx.x + 1];
  if (off + len > (unsigned long long)capacity) return;
  const uint8_t* src = coded + (int64_t)blockIdx.x * PG_CAP;
  uint8_t* dst = bytes + off;
  const unsigned lead = min((unsigned)((4 - ((uintptr_t)dst & 3)) & 3), len);       // bytes up to dst's next dword
  const unsigned words = (len - lead) >> 2;
  if ((unsigned)tid < lead) dst[tid] = src[tid];
  for (unsigned i = tid; i < words; i += PG_BLOCK) {
    const uint8_t* s = src + lead + 4 * i;
    *reinterpret_cast<unsigned*>(dst + lead + 4 * i) = s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16 | (unsigned)s[3] << 24;
  }
  const unsigned done = lead + 4 * words;
  if (done + tid < len) dst[done + tid] = src[done + tid];                          // at most 3 bytes
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t rw_png_segment_bytes(void) { return PG_SEG; }
extern "C" int64_t rw_png_segment_capacity(void) { return PG_CAP; }
extern "C" int64_t rw_png_table_words(void) { return PG_TABLE_WORDS; }

// the checks the three entries share; nseg of one image
static int pg_shape(int64_t images, int height, int width, int64_t* stream_len, int64_t* nseg) {
  RW_CHECK_ARG(images >= 1);
  if (height < 1 || width < 1) return RW_ERR_UNSUPPORTED;
  const int64_t len = (int64_t)height * (1 + 3 * (int64_t)width);
  if (len > INT32_MAX) return RW_ERR_UNSUPPORTED;          // offsets inside a stream are 32-bit; image bases are 64-bit
  *stream_len = len;
  *nseg = rw_cdiv(len, PG_SEG);
  RW_CHECK_ARG(images * *nseg <= INT32_MAX && rw_cdiv(images * height, PG_BLOCK / RW_WAVE) <= INT32_MAX);   // the grids
  return 0;
}

extern "C" int rw_png_filter_u8(const uint8_t* image, uint8_t* row_type, uint8_t* stream, uint32_t* hist_part, uint32_t* hist,
                                uint32_t* adler, int64_t images, int height, int width, rw_stream_t stream_) {
  RW_CHECK_ARG(image && row_type && stream && hist_part && hist && adler);
  int64_t len, nseg;
  const int rc = pg_shape(images, height, width, &len, &nseg);
  if (rc) return rc;
  RW_CHECK_ARG(((uintptr_t)stream % 16) == 0);
  pg_problem p;
  p.image = image; p.row_type = row_type; p.stream = stream; p.hist_part = hist_part; p.hist = hist; p.adler = adler;
  p.rows = images * height; p.H = height; p.row_bytes = 3 * width; p.stream_len = (int)len; p.nseg = (int)nseg;
  hipStream_t s = rw_s(stream_);
  hipLaunchKernelGGL(png_row_type_kernel, dim3((unsigned)rw_cdiv(p.rows, PG_BLOCK / RW_WAVE)), dim3(PG_BLOCK), 0, s, p);
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)(images * nseg)), dim3(PG_BLOCK), 0, s, p);
  hipLaunchKernelGGL(png_hist_sum_kernel, dim3((unsigned)images), dim3(PG_BLOCK), 0, s, p);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_png_encode_u8(const uint8_t* stream, const uint32_t* table, uint8_t* coded, uint32_t* lengths,
                                int64_t images, int height, int width, rw_stream_t stream_) {
  RW_CHECK_ARG(stream && table && coded && lengths);
  int64_t len, nseg;
  const int rc = pg_shape(images, height, width, &len, &nseg);
  if (rc) return rc;
  RW_CHECK_ARG(((uintptr_t)stream % 16) == 0 && ((uintptr_t)coded % 16) == 0);
  pg_encode_problem p;
  p.stream = stream; p.table = table; p.coded = coded; p.lengths = lengths; p.stream_len = (int)len; p.nseg = (int)nseg;
  hipLaunchKernelGGL(png_encode_kernel, dim3((unsigned)(images * nseg)), dim3(PG_BLOCK), PG_LDS_BYTES, rw_s(stream_), p);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_png_compact_u8(const uint8_t* coded, const uint32_t* lengths, const uint32_t* adler, uint64_t* offsets,
                                 uint32_t* head, uint8_t* bytes, int64_t capacity, int64_t segments, rw_stream_t stream_) {
  RW_CHECK_ARG(coded && lengths && adler && offsets && head && bytes);
  RW_CHECK_ARG(segments >= 1 && segments <= INT32_MAX && capacity >= 0);
  hipStream_t s = rw_s(stream_);
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(PG_BLOCK), 0, s, lengths,
                     reinterpret_cast<unsigned long long*>(offsets), segments);
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)segments), dim3(PG_BLOCK), 0, s, coded, lengths, adler,
                     reinterpret_cast<const unsigned long long*>(offsets), head, bytes, capacity);
  return RW_LAUNCH_RESULT();
}
