// The inflate of RFC 1951, written once for the device kernel (rw_pngdec.hip: one wave per stream) and for the host
// program that carries the sanitizers (rw_pngdec_host.cpp).  Plain C++: no LDS, no lane index, no HIP type.  What the
// two sides differ in comes in through three small policies:
//   Source  size(), bytes(pos, take): up to four bytes of the coded stream from pos, and data() for a stored block's bytes
//           (host: a pointer; device: a staging ring in LDS that the lanes fill together);
//   Sink    literal(byte), copy(distance, length), stored(src, n) and produced().  The core asks produced() before every
//           one of them and hands over nothing that would pass the expected length or reach before the first byte: a
//           sink never has to refuse, and the core never touches output itself;
//   Lanes   first() / step() of a loop that may be shared out (host: 0, 1; device: lane, 64), sync() after such a loop and
//           uniform(v), which tells the compiler that v is the same in every lane.
// Every lane of a wave runs this code on the same state, so every branch here is wave-uniform.
//
// What is accepted is what zlib's inflate accepts (inftrees.c: inflate_table; inflate.c):
//   * an over-subscribed set of code lengths is an error, for all three alphabets;
//   * an incomplete set is an error, except a literal/length or distance set whose only code has length 1 (the other
//     1-bit pattern is then an invalid symbol where it occurs), and a distance set with no code at all (any match is then
//     an invalid symbol); the code-length code has no exception;
//   * the literal/length set must give the end-of-block symbol a code;
//   * HLIT above 286 symbols and HDIST above 30 are errors; repeat symbol 16 with no length before it and a repeat
//     that runs past HLIT + HDIST are errors; a repeat may run from the literal lengths into the distance lengths;
//   * literal/length symbols 286, 287 and distance symbols 30, 31 (fixed blocks can code them) are invalid symbols.
// Termination: every pass of the symbol loop and of the block loop consumes at least one bit of input or ends the stream
// (a code has at least one bit; a code that cannot be decoded ends it), and both loops count against 8 * coded bytes + 4
// passes all the same, so that a table this code got wrong could still not spin.
#ifndef RW_INFLATE_CORE_H
#define RW_INFLATE_CORE_H

#include <stdint.h>

#ifndef RW_HD
#if defined(__HIPCC__)
#define RW_HD __host__ __device__ __forceinline__
#else
#define RW_HD inline
#endif
#endif

// the first defect of a stream or of an image: the codes of include/rewriting_hip.h, for a build without that header
#ifndef RW_PNG_OK
#define RW_PNG_OK 0
#define RW_PNG_TRUNCATED 1
#define RW_PNG_BAD_BLOCK_TYPE 2
#define RW_PNG_STORED_LENGTH 3
#define RW_PNG_BAD_CODELEN_SET 4
#define RW_PNG_BAD_LITLEN_SET 5
#define RW_PNG_BAD_DIST_SET 6
#define RW_PNG_NO_END_OF_BLOCK 7
#define RW_PNG_BAD_SYMBOL 8
#define RW_PNG_DISTANCE_TOO_FAR 9
#define RW_PNG_OUTPUT_OVER 10
#define RW_PNG_OUTPUT_UNDER 11
#define RW_PNG_BAD_FILTER 12
#endif

#define RW_INF_FAST_BITS 10                       // codes up to this length decode in one table read
#define RW_INF_MAX_BITS 15
#define RW_INF_MAX_LIT 288
#define RW_INF_MAX_DIST 32
#define RW_INF_MAX_LENGTHS 320                    // HLIT + HDIST <= 286 + 30

namespace rw_inflate {

// One alphabet's decoder.  fast[v] for the next RW_INF_FAST_BITS bits v of the stream: symbol | length << 9, or 0 (no code
// that short starts so); count[l] codes of length l; symbol[] the symbols by (length, symbol) -- zlib's puff.c layout.
struct Table {
  uint16_t* fast;      // 1 << RW_INF_FAST_BITS
  uint16_t* count;     // RW_INF_MAX_BITS + 1
  uint16_t* first;     // RW_INF_MAX_BITS + 1: the first code of a length (RFC 1951 3.2.2)
  uint16_t* end;       // RW_INF_MAX_BITS + 1: one past the last place, in symbol[], of a length
  uint16_t* symbol;    // as many as the alphabet has
};

struct Host {          // the Lanes policy of a single thread
  RW_HD int first() const { return 0; }
  RW_HD int step() const { return 1; }
  RW_HD void sync() const {}
  RW_HD uint32_t uniform(uint32_t v) const { return v; }
};

// A guarded bit reader over the n bytes of a Source.  A read past the end yields zero bits and latches `truncated`; no
// byte outside 0 .. n - 1 is asked of the source.
template <class Source>
struct BitReader {
  Source& src;
  uint64_t hold;       // the next bits, lowest first
  uint32_t nbits;      // of them: <= 64
  uint64_t pos, n;     // the next byte to take; the bytes there are
  bool truncated;

  RW_HD BitReader(Source& s) : src(s), hold(0), nbits(0), pos(0), n(s.size()), truncated(false) {}

  RW_HD void refill() {                           // to more than 32 bits, while there are bytes
    if (nbits > 32) return;
    uint32_t take = n - pos < 4 ? (uint32_t)(n - pos) : 4u;
    uint32_t word = take ? src.bytes(pos, take) : 0u;       // `take` bytes from pos, little endian, zeros above them
    hold |= (uint64_t)word << nbits;
    nbits += 8 * take;
    pos += take;
  }
  RW_HD uint32_t peek(uint32_t bits) {            // bits <= 16; zeros where the stream has ended
    refill();
    return (uint32_t)hold & ((1u << bits) - 1u);
  }
  RW_HD void drop(uint32_t bits) {                // after a peek of at least as many
    if (bits > nbits) { truncated = true; hold = 0; nbits = 0; return; }
    hold >>= bits;
    nbits -= bits;
  }
  RW_HD uint32_t take(uint32_t bits) { const uint32_t v = peek(bits); drop(bits); return v; }
  RW_HD uint32_t left() { refill(); return nbits; }
  // to the next byte boundary; the offset of that byte in the source
  RW_HD uint64_t align() { drop(nbits & 7u); return pos - nbits / 8; }
  RW_HD void seek(uint64_t byte) { pos = byte < n ? byte : n; hold = 0; nbits = 0; }
};

RW_HD uint32_t reverse_bits(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t k = 0; k < len; ++k) r |= ((code >> k) & 1u) << (len - 1 - k);
  return r;
}

// Builds t from lengths[0 .. n).  Returns 0 for a complete set, 1 for an incomplete one (zlib's `left` > 0: the caller
// says whether that is allowed; `longest` tells it how), -1 for an over-subscribed one.  With no code at all: 1, longest 0.
template <class Lanes>
RW_HD int build_table(const Table& t, const uint8_t* lengths, int n, Lanes& lanes, int* longest) {
  lanes.sync();                                   // whoever still decodes with the table that was here has finished
  if (lanes.first() == 0) {
    for (int l = 0; l <= RW_INF_MAX_BITS; ++l) t.count[l] = 0;
    for (int s = 0; s < n; ++s) t.count[lengths[s]] = (uint16_t)(t.count[lengths[s]] + 1);
  }
  for (int k = lanes.first(); k < (1 << RW_INF_FAST_BITS); k += lanes.step()) t.fast[k] = 0;
  lanes.sync();
  int left = 1, top = 0, place = 0;
  uint32_t code = 0;
  for (int l = 1; l <= RW_INF_MAX_BITS; ++l) {
    const int c = (int)lanes.uniform(t.count[l]);
    left = (left << 1) - c;
    if (left < 0) return -1;
    if (c) top = l;
    if (lanes.first() == 0) {
      t.first[l] = (uint16_t)code;
      t.end[l] = (uint16_t)place;                 // where the length's symbols start: the fill below moves it to their end
    }
    place += c;
    code = (code + (uint32_t)c) << 1;
  }
  *longest = top;
  lanes.sync();
  if (lanes.first() == 0) {                       // the symbols in order of (length, symbol)
    for (int s = 0; s < n; ++s) {
      const uint32_t l = lengths[s];
      if (l) { const uint16_t at = t.end[l]; t.symbol[at] = (uint16_t)s; t.end[l] = (uint16_t)(at + 1); }
    }
  }
  lanes.sync();
  for (int j = lanes.first(); j < place; j += lanes.step()) {         // place j of that order: the lanes share them out
    const uint32_t s = t.symbol[j], l = lengths[s];
    if (l > RW_INF_FAST_BITS) continue;
    const uint32_t entry = s | l << 9, start = (uint32_t)t.end[l] - (uint32_t)t.count[l];
    for (uint32_t v = reverse_bits(t.first[l] + ((uint32_t)j - start), l); v < (1u << RW_INF_FAST_BITS); v += 1u << l)
      t.fast[v] = (uint16_t)entry;
  }
  lanes.sync();
  return left > 0 ? 1 : 0;
}

// The next symbol, or -1: no code of the table starts with the bits that come (or the stream ended inside it: the
// reader has latched that).
template <class Source, class Lanes>
RW_HD int decode(BitReader<Source>& in, const Table& t, Lanes& lanes) {
  const uint32_t bits = in.peek(RW_INF_MAX_BITS);
  const uint32_t e = lanes.uniform(t.fast[bits & ((1u << RW_INF_FAST_BITS) - 1u)]);
  if (e) {
    in.drop(e >> 9);
    return in.truncated ? -1 : (int)(e & 511u);
  }
  int code = 0, first = 0, index = 0;             // puff.c: the code read bit by bit against the counts
  for (int l = 1; l <= RW_INF_MAX_BITS; ++l) {
    code |= (int)((bits >> (l - 1)) & 1u);
    const int c = (int)lanes.uniform(t.count[l]);
    if (code - c < first) {
      in.drop((uint32_t)l);
      return in.truncated ? -1 : (int)lanes.uniform(t.symbol[index + (code - first)]);
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  if (in.left() < RW_INF_MAX_BITS) in.truncated = true;   // the stream ended inside what might have been a code
  return -1;
}

// the work areas of one stream: LDS on the device, plain arrays on the host
struct Work {
  Table lit, dist;
  uint8_t* lengths;    // RW_INF_MAX_LENGTHS
};

RW_HD uint32_t length_base(int s) {               // s = symbol - 257: RFC 1951 3.2.5
  return s < 8 ? 3u + (uint32_t)s : s == 28 ? 258u : 3u + ((4u + ((uint32_t)s & 3u)) << ((uint32_t)s / 4u - 1u));
}
RW_HD uint32_t length_extra(int s) { return s < 8 || s == 28 ? 0u : (uint32_t)s / 4u - 1u; }
RW_HD uint32_t dist_base(int s) { return s < 4 ? 1u + (uint32_t)s : 1u + ((2u + ((uint32_t)s & 1u)) << ((uint32_t)s / 2u - 1u)); }
RW_HD uint32_t dist_extra(int s) { return s < 4 ? 0u : (uint32_t)s / 2u - 1u; }

template <class Lanes>
RW_HD int fixed_tables(const Work& w, Lanes& lanes) {
  for (int s = lanes.first(); s < 288; s += lanes.step()) w.lengths[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  lanes.sync();
  int top;
  build_table(w.lit, w.lengths, 288, lanes, &top);
  for (int s = lanes.first(); s < 32; s += lanes.step()) w.lengths[s] = 5;
  lanes.sync();
  build_table(w.dist, w.lengths, 32, lanes, &top);
  return RW_PNG_OK;
}

template <class Source, class Lanes>
RW_HD int dynamic_tables(BitReader<Source>& in, const Work& w, Lanes& lanes) {
  const int nlen = (int)in.take(5) + 257, ndist = (int)in.take(5) + 1, ncode = (int)in.take(4) + 4;
  if (in.truncated) return RW_PNG_TRUNCATED;
  if (nlen > 286) return RW_PNG_BAD_LITLEN_SET;
  if (ndist > 30) return RW_PNG_BAD_DIST_SET;
  // the code-length code: 3 bits each, in the order of RFC 1951 3.2.7 (packed here five bits a symbol)
  const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                            10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  uint64_t cl = 0;                                // 19 lengths of 3 bits
  for (int k = 0; k < ncode; ++k) {
    const uint32_t s = (uint32_t)((k < 12 ? order_lo >> (5 * k) : order_hi >> (5 * (k - 12))) & 31u);
    cl |= (uint64_t)in.take(3) << (3 * s);
  }
  if (in.truncated) return RW_PNG_TRUNCATED;
  lanes.sync();                                   // the lengths area may still be read by a table fill before this block
  for (int s = lanes.first(); s < 19; s += lanes.step()) w.lengths[s] = (uint8_t)((cl >> (3 * s)) & 7u);
  lanes.sync();
  int top;
  if (build_table(w.lit, w.lengths, 19, lanes, &top) != 0) return RW_PNG_BAD_CODELEN_SET;   // borrowed until the real one

  int have = 0, prev = -1;
  lanes.sync();
  while (have < nlen + ndist) {                   // every pass drops at least one bit or returns
    const int s = decode(in, w.lit, lanes);
    if (in.truncated) return RW_PNG_TRUNCATED;
    if (s < 0) return RW_PNG_BAD_CODELEN_SET;     // cannot happen: the code is complete
    if (s < 16) {
      if (lanes.first() == 0) w.lengths[have] = (uint8_t)s;
      ++have;
      prev = s;
      continue;
    }
    int value = 0, repeat;
    if (s == 16) {
      if (prev < 0) return RW_PNG_BAD_CODELEN_SET;
      value = prev;
      repeat = 3 + (int)in.take(2);
    } else if (s == 17) {
      repeat = 3 + (int)in.take(3);
    } else {
      repeat = 11 + (int)in.take(7);
    }
    if (in.truncated) return RW_PNG_TRUNCATED;
    if (have + repeat > nlen + ndist) return RW_PNG_BAD_CODELEN_SET;
    for (int k = lanes.first(); k < repeat; k += lanes.step()) w.lengths[have + k] = (uint8_t)value;
    have += repeat;
    prev = value;
  }
  lanes.sync();
  if (lanes.uniform(w.lengths[256]) == 0) return RW_PNG_NO_END_OF_BLOCK;
  // the distance lengths first: the literal table replaces the code-length code, which is done with
  int rc = build_table(w.dist, w.lengths + nlen, ndist, lanes, &top);
  if (rc < 0 || (rc > 0 && top > 1)) return RW_PNG_BAD_DIST_SET;
  rc = build_table(w.lit, w.lengths, nlen, lanes, &top);
  if (rc < 0 || (rc > 0 && top != 1)) return RW_PNG_BAD_LITLEN_SET;
  return RW_PNG_OK;
}

// The whole stream into the sink.  Returns the first defect; the sink has what came before it.
template <class Source, class Sink, class Lanes>
RW_HD int inflate(Source& src, Sink& sink, const Work& w, Lanes& lanes, uint64_t expect) {
  BitReader<Source> in(src);
  const uint64_t bound = 8 * in.n + 4;
  uint64_t passes = 0;
  for (;;) {
    if (++passes > bound) return RW_PNG_TRUNCATED;
    const uint32_t last = in.take(1), type = in.take(2);
    if (in.truncated) return RW_PNG_TRUNCATED;
    if (type == 3) return RW_PNG_BAD_BLOCK_TYPE;
    if (type == 0) {
      const uint64_t at = in.align();
      in.seek(at);
      const uint32_t len = in.take(16), nlen = in.take(16);
      if (in.truncated) return RW_PNG_TRUNCATED;
      if ((len ^ 0xffffu) != nlen) return RW_PNG_STORED_LENGTH;
      if (at + 4 + len > in.n) return RW_PNG_TRUNCATED;
      if (sink.produced() + len > expect) return RW_PNG_OUTPUT_OVER;
      if (len) sink.stored(src.data() + at + 4, len);
      in.seek(at + 4 + len);
    } else {
      const int rc = type == 1 ? fixed_tables(w, lanes) : dynamic_tables(in, w, lanes);
      if (rc) return rc;
      for (;;) {
        if (++passes > bound) return RW_PNG_TRUNCATED;
        int s = decode(in, w.lit, lanes);
        if (in.truncated) return RW_PNG_TRUNCATED;
        if (s < 0 || s > 285) return RW_PNG_BAD_SYMBOL;
        if (s < 256) {
          if (sink.produced() >= expect) return RW_PNG_OUTPUT_OVER;
          sink.literal((uint8_t)s);
          continue;
        }
        if (s == 256) break;
        s -= 257;
        const uint32_t length = length_base(s) + in.take(length_extra(s));
        if (in.truncated) return RW_PNG_TRUNCATED;
        const int d = decode(in, w.dist, lanes);
        if (in.truncated) return RW_PNG_TRUNCATED;
        if (d < 0 || d > 29) return RW_PNG_BAD_SYMBOL;
        const uint32_t distance = dist_base(d) + in.take(dist_extra(d));
        if (in.truncated) return RW_PNG_TRUNCATED;
        if (distance > sink.produced()) return RW_PNG_DISTANCE_TOO_FAR;
        if (sink.produced() + length > expect) return RW_PNG_OUTPUT_OVER;
        sink.copy(distance, length);
      }
    }
    if (last) break;
  }
  return sink.produced() < expect ? RW_PNG_OUTPUT_UNDER : RW_PNG_OK;
}

}  // namespace rw_inflate

#endif
