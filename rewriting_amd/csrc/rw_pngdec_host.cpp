// The inflate core (rw_inflate_core.h) on the host, alone: a program with its own main, never part of the library.  It
// is what the address and undefined-behaviour sanitizers run on (tests/test_pngdec_core_host.py builds it with them): the
// same core the kernel of rw_pngdec.hip runs, with a plain-vector sink and one thread as the lanes.
//
//   rw_pngdec_host CASES
// CASES: uint32 count, then per case uint32 coded bytes n, uint32 expected length, n bytes -- a raw deflate stream
// (little endian).  Prints per case: status, bytes produced, Adler-32 of them (decimal).
// Every stream is copied into a heap block of exactly its size, so that a read past its end is a report, not luck.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "rw_inflate_core.h"

namespace {

struct PointerSource {
  const uint8_t* begin;
  uint64_t n;
  uint64_t size() const { return n; }
  const uint8_t* data() const { return begin; }
  uint32_t bytes(uint64_t pos, uint32_t take) const {
    uint32_t word = 0;
    for (uint32_t k = 0; k < take; ++k) word |= (uint32_t)begin[pos + k] << (8 * k);
    return word;
  }
};

struct VectorSink {
  std::vector<uint8_t> out;
  uint64_t produced() const { return out.size(); }
  void literal(uint8_t byte) { out.push_back(byte); }
  void copy(uint32_t distance, uint32_t length) {
    for (uint32_t i = 0; i < length; ++i) out.push_back(out[out.size() - distance]);
  }
  void stored(const uint8_t* src, uint32_t n) { out.insert(out.end(), src, src + n); }
};

uint32_t adler32(const std::vector<uint8_t>& data) {
  uint32_t a = 1, b = 0;
  for (uint8_t v : data) {
    a = (a + v) % 65521u;
    b = (b + a) % 65521u;
  }
  return b << 16 | a;
}

bool read_u32(FILE* f, uint32_t* v) {
  uint8_t raw[4];
  if (fread(raw, 1, 4, f) != 4) return false;
  *v = raw[0] | (uint32_t)raw[1] << 8 | (uint32_t)raw[2] << 16 | (uint32_t)raw[3] << 24;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CASES\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  uint32_t cases = 0;
  if (!f || !read_u32(f, &cases)) {
    fprintf(stderr, "%s: cannot read %s\n", argv[0], argv[1]);
    return 2;
  }
  // the work areas: one allocation each, of exactly the size the core is promised
  using namespace rw_inflate;
  std::vector<uint16_t> lit_fast(1 << RW_INF_FAST_BITS), dist_fast(1 << RW_INF_FAST_BITS);
  std::vector<uint16_t> lit_count(RW_INF_MAX_BITS + 1), dist_count(RW_INF_MAX_BITS + 1);
  std::vector<uint16_t> lit_first(RW_INF_MAX_BITS + 1), dist_first(RW_INF_MAX_BITS + 1);
  std::vector<uint16_t> lit_end(RW_INF_MAX_BITS + 1), dist_end(RW_INF_MAX_BITS + 1);
  std::vector<uint16_t> lit_symbol(RW_INF_MAX_LIT), dist_symbol(RW_INF_MAX_DIST);
  std::vector<uint8_t> lengths(RW_INF_MAX_LENGTHS);
  Work work;
  work.lit = Table{lit_fast.data(), lit_count.data(), lit_first.data(), lit_end.data(), lit_symbol.data()};
  work.dist = Table{dist_fast.data(), dist_count.data(), dist_first.data(), dist_end.data(), dist_symbol.data()};
  work.lengths = lengths.data();

  for (uint32_t c = 0; c < cases; ++c) {
    uint32_t n = 0, expect = 0;
    if (!read_u32(f, &n) || !read_u32(f, &expect)) {
      fprintf(stderr, "%s: case %u is cut short\n", argv[0], c);
      return 2;
    }
    std::unique_ptr<uint8_t[]> coded(new uint8_t[n]);
    if (n && fread(coded.get(), 1, n, f) != n) {
      fprintf(stderr, "%s: case %u is cut short\n", argv[0], c);
      return 2;
    }
    PointerSource source{coded.get(), n};
    VectorSink sink;
    Host lanes;
    const int status = inflate(source, sink, work, lanes, (uint64_t)expect);
    printf("%d %llu %u\n", status, (unsigned long long)sink.produced(), adler32(sink.out));
  }
  fclose(f);
  return 0;
}
