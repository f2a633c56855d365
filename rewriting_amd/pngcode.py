"""The host side of the device PNG encoder (include/rewriting_hip.h, "PNG encoding"): what is O(256) per image.

From the byte histogram of an image's filtered stream: a complete, length-limited prefix code for the literals
(``limited_lengths``: package-merge, so the Kraft sum is exactly 1 and no length passes the limit -- zlib refuses
incomplete and over-subscribed sets alike), the code-length code, the bits of the dynamic block header and the table
the encode kernel reads (``code_table``).  After the kernels: the Adler-32 of the stream from the segments' sums
(``adler_fold``) and the chunk framing (``frame``).  Everything here is deterministic: the same histogram gives the
same table.  numpy and zlib only -- tests/png_checks.py builds its twin of the encoder on these functions.
"""
import struct
import zlib

import numpy

MAX_LITERAL_BITS = 15
MAX_CODELEN_BITS = 7
END_OF_BLOCK = 256
HEADER_BYTES = 256           # PG_HDR_BYTES of rw_png.hip: the room a table has for the block header
TABLE_WORDS = 1 + 257 + HEADER_BYTES // 4
ADLER = 65521
CODELEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)      # RFC 1951 3.2.7
ZLIB_HEADER = b'\x78\x01'
STREAM_END = b'\x01\x00\x00\xff\xff'         # the final, empty, stored block
SIGNATURE = b'\x89PNG\r\n\x1a\n'


def limited_lengths(counts, max_bits):
    """Code lengths (int array like counts) of an optimal prefix code with no length above max_bits, by package-merge.
    Symbols with count 0 get length 0.  With two or more used symbols the code is complete (Kraft sum exactly 1); a
    lone used symbol is given a partner (the next symbol, or the one before the last) so that it is complete as well.
    Ties are broken by symbol number: the result depends on counts alone."""
    counts = numpy.asarray(counts, dtype=numpy.int64)
    lengths = numpy.zeros(len(counts), dtype=numpy.int64)
    used = numpy.flatnonzero(counts > 0)
    if len(used) == 0:
        return lengths
    if len(used) == 1:
        s = int(used[0])
        lengths[s] = lengths[s + 1 if s + 1 < len(counts) else s - 1] = 1
        return lengths
    n = len(used)
    assert n <= 1 << max_bits, 'no prefix code of %d symbols within %d bits' % (n, max_bits)
    order = used[numpy.argsort(counts[used], kind='stable')]         # by count, then by symbol
    leaf_w = counts[order]
    # level by level: the leaves and the packages of the level before, by weight (equal weights: leaves first, then in
    # order); neighbours pair up into the next level's packages.  Only which items are packages is kept.
    pack_w, levels = leaf_w[:0], []
    for _ in range(max_bits):
        w = numpy.concatenate([leaf_w, pack_w])
        pick = numpy.argsort(w, kind='stable')
        levels.append(numpy.cumsum(pick >= n))                       # packages among the first k + 1 items
        pairs = len(pick) // 2
        w = w[pick][:2 * pairs]
        pack_w = w[0::2] + w[1::2]
    # back from the last level: of its first 2 n - 2 items the leaves (a prefix of the leaves: they are sorted) gain a
    # bit, and the packages are the first 2 p items of the level before
    gained = numpy.zeros(n + 1, dtype=numpy.int64)
    take = 2 * n - 2
    for packages_among in reversed(levels):
        if take == 0:
            break
        p = int(packages_among[take - 1])
        gained[take - p] += 1                                        # leaves 0 .. take - p - 1
        take = 2 * p
    lengths[order] = numpy.cumsum(gained[::-1])[::-1][1:]
    return lengths


def kraft_sum_times(lengths, max_bits):
    """sum 2^(max_bits - length) over the used symbols: 2^max_bits for a complete code"""
    return sum(1 << (max_bits - int(v)) for v in lengths if v > 0)


def canonical_codes(lengths):
    """The codes of RFC 1951 3.2.2 for these lengths (0 where the length is 0), as an int array"""
    lengths = numpy.asarray(lengths, dtype=numpy.int64)
    top = int(lengths.max())
    per_length = numpy.bincount(lengths, minlength=top + 1)
    per_length[0] = 0
    code, first = 0, numpy.zeros(top + 1, dtype=numpy.int64)
    for bits in range(1, top + 1):
        code = (code + int(per_length[bits - 1])) << 1
        first[bits] = code
    order = numpy.argsort(lengths, kind='stable')                    # by length, then by symbol
    by_length = lengths[order]
    rank = numpy.empty(len(lengths), dtype=numpy.int64)              # of a symbol among those of its length
    rank[order] = numpy.arange(len(lengths)) - numpy.searchsorted(by_length, by_length, side='left')
    return numpy.where(lengths > 0, first[lengths] + rank, 0)


def _bit_reversal_table(bits):
    table = numpy.zeros(1 << bits, dtype=numpy.int64)
    values = numpy.arange(1 << bits)
    for k in range(bits):
        table |= ((values >> k) & 1) << (bits - 1 - k)
    return table


_REVERSED_15 = _bit_reversal_table(MAX_LITERAL_BITS)


def reversed_codes(codes, lengths):
    """Every code with its bits in stream order: the highest bit of the code in bit 0"""
    codes, lengths = numpy.asarray(codes, dtype=numpy.int64), numpy.asarray(lengths, dtype=numpy.int64)
    return _REVERSED_15[codes] >> (MAX_LITERAL_BITS - lengths)


def run_lengths(lengths):
    """The sequence of code lengths in the code-length alphabet: [(symbol, extra bits, value of the extra bits)].
    Greedy: a run of zeros as 18 (11 .. 138) or 17 (3 .. 10), a run of one length as the length, then 16 (3 .. 6)."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                take = min(run, 138)
                out.append((18, 7, take - 11))
                run -= take
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out.extend([(0, 0, 0)] * run)
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                take = min(run, 6)
                out.append((16, 2, take - 3))
                run -= take
            out.extend([(v, 0, 0)] * run)
        i = j
    return out


class _Bits:
    """A deflate bit string: values go in from their lowest bit (Huffman codes bit-reversed first: RFC 1951 3.1.1)"""

    def __init__(self):
        self.value, self.count = 0, 0

    def put(self, value, bits):
        self.value |= value << self.count
        self.count += bits

    def tobytes(self):
        return self.value.to_bytes((self.count + 7) // 8, 'little')


def block_header(literal_lengths):
    """(bits, count) of a dynamic block's header, BFINAL = 0, for the lengths of literals 0 .. 256 and no distance code,
    and the lengths of the code-length code it uses (for the tests)."""
    literal_lengths = [int(v) for v in literal_lengths]
    assert len(literal_lengths) == 257 and literal_lengths[END_OF_BLOCK] > 0
    sequence = run_lengths(literal_lengths + [0])            # HLIT = 0: 257 codes; HDIST = 0: one distance code, unused
    counts = numpy.zeros(19, dtype=numpy.int64)
    for symbol, _, _ in sequence:
        counts[symbol] += 1
    cl_lengths = limited_lengths(counts, MAX_CODELEN_BITS)
    cl_bits = [int(v) for v in cl_lengths]
    cl_codes = [int(v) for v in reversed_codes(canonical_codes(cl_lengths), cl_lengths)]      # in stream order
    hclen = 19
    while hclen > 4 and cl_lengths[CODELEN_ORDER[hclen - 1]] == 0:
        hclen -= 1
    bits = _Bits()
    bits.put(0, 1)               # BFINAL
    bits.put(2, 2)               # BTYPE = 10
    bits.put(0, 5)               # HLIT
    bits.put(0, 5)               # HDIST
    bits.put(hclen - 4, 4)
    for symbol in CODELEN_ORDER[:hclen]:
        bits.put(cl_bits[symbol], 3)
    for symbol, extra, value in sequence:
        bits.put(cl_codes[symbol], cl_bits[symbol])
        if extra:
            bits.put(value, extra)
    assert bits.count <= 8 * HEADER_BYTES
    return bits, cl_lengths


def code_table(histogram, segments):
    """The uint32 row of rw_png_encode_u8's table for one image, from the 256 counts of its stream and the number of its
    segments (an end-of-block each), and the literal lengths (257)."""
    counts = numpy.zeros(257, dtype=numpy.int64)
    counts[:256] = numpy.asarray(histogram, dtype=numpy.int64)
    counts[END_OF_BLOCK] = segments
    lengths = limited_lengths(counts, MAX_LITERAL_BITS)
    codes = canonical_codes(lengths)
    header, _ = block_header(lengths)
    row = numpy.zeros(TABLE_WORDS, dtype=numpy.uint32)
    row[0] = header.count
    row[1:258] = reversed_codes(codes, lengths) | lengths << 16
    packed = header.tobytes().ljust(HEADER_BYTES, b'\0')
    row[258:] = numpy.frombuffer(packed, dtype='<u4')
    return row, lengths


def coded_bytes_bound(histogram, lengths, header_bits, segments):
    """No more bytes than this come out of an image's segments together: the literals' bits, and per segment the header,
    the end-of-block, the three bits of the stored block, the padding and 00 00 FF FF."""
    literal_bits = int((numpy.asarray(histogram, dtype=numpy.int64) * lengths[:256]).sum())
    per_segment = header_bits + int(lengths[END_OF_BLOCK]) + 3 + 7 + 32
    return (literal_bits + segments * per_segment + 7) // 8 + segments


def adler_fold(parts):
    """The Adler-32 of a stream from (n, s1, s2) of its segments in order (see rw_png_filter_u8)"""
    a, b = 1, 0
    for n, s1, s2 in parts:
        b = (b + int(n) * a + int(s2)) % ADLER
        a = (a + int(s1)) % ADLER
    return b << 16 | a


def chunk(kind, data):
    crc = zlib.crc32(data, zlib.crc32(kind)) & 0xffffffff
    return b''.join([struct.pack('>I', len(data)), kind, data, struct.pack('>I', crc)])


def frame(width, height, segments, adler):
    """The PNG file: signature, IHDR (8-bit truecolour, no interlace), one IDAT of the coded segments, IEND"""
    idat = b''.join([ZLIB_HEADER] + list(segments) + [STREAM_END, struct.pack('>I', adler)])
    return b''.join([SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, 2, 0, 0, 0)),
                     chunk(b'IDAT', idat), chunk(b'IEND', b'')])
