"""A numpy twin of the device PNG encoder (include/rewriting_hip.h, "PNG encoding"), parameterised by the segment size S:
the filter rule, the histogram, the package's host builder (rewriting_amd/pngcode.py) for the code lengths and the
block header, the bit layout of a segment and the framing.  The format is fully specified, so hip.png_encode has to
give these bytes exactly.  Independent of the kernels where it can be: the codes are written out bit by bit from the
canonical code (highest bit first), and the Adler-32 is zlib's over the whole stream, not a fold of partial sums.
"""
import heapq
import io
import struct
import zlib

import numpy

from rewriting_amd import pngcode


# ---- the filter pass
def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return numpy.where((pa <= pb) & (pa <= pc), a, numpy.where(pb <= pc, b, c))


def filter_rows(image):
    """(stream bytes, row types) of image (H, W, 3) uint8: per row the type, of 0 .. 4, with the smallest sum of
    |residual as a signed byte|, ties to the lowest type; the row above row 0 is zero."""
    h, w, _ = image.shape
    rows = image.reshape(h, 3 * w).astype(numpy.int64)
    stream = numpy.zeros((h, 1 + 3 * w), dtype=numpy.uint8)
    types = numpy.zeros(h, dtype=numpy.int64)
    for y in range(h):
        x = rows[y]
        b = rows[y - 1] if y else numpy.zeros_like(x)
        a = numpy.concatenate([numpy.zeros(3, dtype=numpy.int64), x[:-3]])[:len(x)]
        c = numpy.concatenate([numpy.zeros(3, dtype=numpy.int64), b[:-3]])[:len(x)]
        residuals = [(x - pred) & 0xff for pred in (0 * x, a, b, (a + b) >> 1, _paeth(a, b, c))]
        cost = [int(numpy.where(r < 128, r, 256 - r).sum()) for r in residuals]
        types[y] = cost.index(min(cost))
        stream[y, 0] = types[y]
        stream[y, 1:] = residuals[types[y]]
    return stream.reshape(-1), types


# ---- the bit layout
def _code_bits(codes, lengths, symbols):
    """The bits of the symbols' codes in stream order: every code from its highest bit down"""
    codes = numpy.asarray(codes, dtype=numpy.int64)[symbols]
    lens = numpy.asarray(lengths, dtype=numpy.int64)[symbols]
    assert (lens > 0).all(), 'a symbol of the stream has no code'
    k = numpy.arange(pngcode.MAX_LITERAL_BITS)
    bits = (codes[:, None] >> numpy.maximum(lens[:, None] - 1 - k[None, :], 0)) & 1
    return bits[k[None, :] < lens[:, None]].astype(numpy.uint8)


def coded_segment(data, header, codes, lengths):
    """The bytes of one segment: the dynamic header, the literals, end-of-block, `000`, padding, 00 00 FF FF"""
    head = numpy.array([(header.value >> i) & 1 for i in range(header.count)], dtype=numpy.uint8)
    symbols = numpy.concatenate([numpy.asarray(data, dtype=numpy.int64), [pngcode.END_OF_BLOCK]])
    bits = numpy.concatenate([head, _code_bits(codes, lengths, symbols), numpy.zeros(3, dtype=numpy.uint8)])
    return numpy.packbits(bits, bitorder='little').tobytes() + b'\x00\x00\xff\xff'


def encode(image, segment_bytes):
    """(png file, filtered stream, details) for image (H, W, 3) uint8"""
    image = numpy.ascontiguousarray(image, dtype=numpy.uint8)
    h, w, _ = image.shape
    stream, types = filter_rows(image)
    nseg = -(-len(stream) // segment_bytes)
    histogram = numpy.bincount(stream, minlength=256)
    counts = numpy.concatenate([histogram, [nseg]])
    lengths = pngcode.limited_lengths(counts, pngcode.MAX_LITERAL_BITS)
    codes = pngcode.canonical_codes(lengths)
    header, cl_lengths = pngcode.block_header(lengths)
    segments = [coded_segment(stream[s:s + segment_bytes], header, codes, lengths)
                for s in range(0, len(stream), segment_bytes)]
    idat = b''.join([b'\x78\x01'] + segments + [b'\x01\x00\x00\xff\xff',
                                               struct.pack('>I', zlib.adler32(stream.tobytes()) & 0xffffffff)])

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)

    png = b''.join([b'\x89PNG\r\n\x1a\n', chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)),
                    chunk(b'IDAT', idat), chunk(b'IEND', b'')])
    details = dict(types=types, counts=counts, lengths=lengths, cl_lengths=cl_lengths, header_bits=header.count,
                   segments=segments, idat=idat)
    return png, stream.tobytes(), details


# ---- reading a file back
def idat_of(png):
    """The payload of the (one) IDAT chunk, with the chunk CRCs checked"""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    at, found = 8, []
    while at < len(png):
        size, kind = struct.unpack('>I', png[at:at + 4])[0], png[at + 4:at + 8]
        data = png[at + 8:at + 8 + size]
        assert struct.unpack('>I', png[at + 8 + size:at + 12 + size])[0] == zlib.crc32(kind + data) & 0xffffffff, kind
        if kind == b'IDAT':
            found.append(data)
        at += 12 + size
    assert at == len(png) and len(found) == 1
    return found[0]


def decode(png):
    """The pixels (H, W, 3) uint8 as PIL reads them"""
    import PIL.Image
    return numpy.asarray(PIL.Image.open(io.BytesIO(png)).convert('RGB'))


def pil_png_size(image):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(image).save(buf, format='png')
    return len(buf.getvalue())


# ---- codes
def unlimited_depth(counts):
    """The longest code of a plain Huffman tree over the used symbols"""
    heap = [(int(c), i, 0) for i, c in enumerate(counts) if c > 0]
    heapq.heapify(heap)
    tick = len(counts)
    while len(heap) > 1:
        (wa, _, da), (wb, _, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (wa + wb, tick, max(da, db) + 1))
        tick += 1
    return heap[0][2]


def kraft_is_one(lengths, max_bits):
    return pngcode.kraft_sum_times(lengths, max_bits) == 1 << max_bits


# ---- pictures
def lowpass_noise(size, seed, channels=3):
    """A smooth random picture plus a little noise: what a generator's output codes like"""
    rng = numpy.random.RandomState(seed)
    field = rng.randn(size + 24, size + 24, channels)
    for axis in (0, 1):
        for _ in range(3):                               # three box blurs of 8 (each takes 8 off): close to a Gaussian
            cs, n = numpy.cumsum(field, axis=axis), field.shape[axis]
            field = numpy.take(cs, range(8, n), axis=axis) - numpy.take(cs, range(0, n - 8), axis=axis)
    field = (field - field.mean()) / field.std()
    return numpy.clip(128 + 48 * field + 2.0 * rng.randn(size, size, channels), 0, 255).astype(numpy.uint8)


def skewed_literal_lengths():
    """257 literal code lengths, a complete code (Kraft sum 1), whose sequence uses nine symbols of the code-length
    alphabet with the counts 1 1 2 3 5 8 13 21 67 -- every count above the sum of all counts two places below it, so a
    plain Huffman tree over them is a chain, 8 deep.  The 1s are the run of 138 unused literals (one symbol 18) and the
    distance code's 0; the lengths are interleaved so that none comes more than twice in a row (no repeat codes)."""
    left = {7: 67, 6: 21, 10: 13, 8: 8, 9: 5, 5: 3, 11: 2}
    assert sum(n << (15 - bits) for bits, n in left.items()) == 1 << 15 and sum(left.values()) == 257 - 138
    tail = []
    while any(left.values()):
        bits = max((b for b in left if left[b] and tail[-2:] != [b, b]), key=lambda b: (left[b], b))
        tail.append(bits)
        left[bits] -= 1
    return [0] * 138 + tail


def fibonacci_row(symbols=16, seed=0):
    """A 1-row image whose Sub residuals take `symbols` values with the Fibonacci counts 1, 2, 3, 5, ... (4 178 bytes for
    16); the one end-of-block is the other 1 of the series, so a plain Huffman tree over the block's symbols is
    `symbols` deep"""
    fib = [1, 2]
    while len(fib) < symbols:
        fib.append(fib[-1] + fib[-2])
    values = [((k + 1) // 2) * (1 if k % 2 else -1) for k in range(symbols)]           # 0, 1, -1, 2, -2, ...
    residuals = numpy.concatenate([numpy.full(n, v) for v, n in zip(values[::-1], fib)])
    residuals = numpy.concatenate([residuals, numpy.zeros(-len(residuals) % 3, dtype=residuals.dtype)])
    numpy.random.RandomState(seed).shuffle(residuals)
    pixels = numpy.cumsum(residuals.reshape(-1, 3), axis=0)                            # x[i] = x[i - 3] + r[i]
    return (pixels & 0xff).astype(numpy.uint8)[None]
