"""A numpy / Python twin of the device PNG decoder (include/rewriting_hip.h, "PNG decoding") and the builders its tests
need.  Written from RFC 1951 and the PNG specification, not from the kernels: the codes are matched bit by bit against
a dictionary of canonical codes, the length and distance tables are the RFC's, spelled out.

* ``inflate(data, expect)``   (status, bytes): the status codes of the library, first defect first;
* ``unfilter(stream, h, w, channels)``   (status, pixels (h, w, 3));
* ``png_decode(...)``   the signature and the results of hip.png_decode, on the host (the pixels as a CPU tensor);
* ``Deflate``   a builder of raw deflate streams from explicit ops and explicit code lengths: stored, fixed and dynamic
  blocks, also ones no encoder would write and ones that are defective in exactly one way;
* ``png_file``   a PNG file with a chosen filter type per row, channels 1, 3, 4 (or any IHDR one asks for), any split
  of the IDAT.
"""
import struct
import zlib

import numpy

from rewriting_amd import pngcode

OK, TRUNCATED, BAD_BLOCK_TYPE, STORED_LENGTH, BAD_CODELEN_SET, BAD_LITLEN_SET, BAD_DIST_SET, NO_END_OF_BLOCK, BAD_SYMBOL, \
    DISTANCE_TOO_FAR, OUTPUT_OVER, OUTPUT_UNDER, BAD_FILTER = range(13)

# RFC 1951 3.2.5
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


# ---- inflate
class _Reader:
    def __init__(self, data):
        self.data, self.n, self.pos, self.truncated = bytes(data), 8 * len(data), 0, False

    def peek(self, bits):               # zeros past the end
        at = self.pos >> 3
        return (int.from_bytes(self.data[at:at + 4], 'little') >> (self.pos & 7)) & ((1 << bits) - 1)

    def drop(self, bits):
        if self.pos + bits > self.n:
            self.truncated, self.pos = True, self.n
        else:
            self.pos += bits

    def take(self, bits):
        v = self.peek(bits)
        self.drop(bits)
        return 0 if self.truncated else v

    def left(self):
        return self.n - self.pos


def _code_set(lengths):
    """(kind, longest, codes): kind 0 complete, 1 incomplete, -1 over-subscribed; codes {(length, bits in stream order
    as an integer, first bit lowest): symbol}"""
    lengths = [int(v) for v in lengths]
    longest = max(lengths) if lengths else 0
    kraft = sum(1 << (15 - v) for v in lengths if v)
    if kraft > 1 << 15:
        return -1, longest, {}
    codes, code = {}, 0
    for bits in range(1, 16):
        for symbol, v in enumerate(lengths):
            if v == bits:
                codes[(bits, int(format(code, '0%db' % bits)[::-1], 2))] = symbol
                code += 1
        code <<= 1
    return (0 if kraft == 1 << 15 else 1), longest, codes


def _decode(reader, codes):
    """The next symbol, or -1 (the reader says whether the stream ended inside it)"""
    window = reader.peek(15)
    for bits in range(1, 16):
        symbol = codes.get((bits, window & ((1 << bits) - 1)))
        if symbol is not None:
            reader.drop(bits)
            return -1 if reader.truncated else symbol
    if reader.left() < 15:
        reader.truncated = True
    return -1


def _dynamic(reader):
    nlen, ndist, ncode = reader.take(5) + 257, reader.take(5) + 1, reader.take(4) + 4
    if reader.truncated:
        return TRUNCATED, None, None
    if nlen > 286:
        return BAD_LITLEN_SET, None, None
    if ndist > 30:
        return BAD_DIST_SET, None, None
    cl = [0] * 19
    for k in range(ncode):
        cl[pngcode.CODELEN_ORDER[k]] = reader.take(3)
    if reader.truncated:
        return TRUNCATED, None, None
    kind, _, cl_codes = _code_set(cl)
    if kind != 0:
        return BAD_CODELEN_SET, None, None
    lengths = []
    while len(lengths) < nlen + ndist:
        s = _decode(reader, cl_codes)
        if reader.truncated:
            return TRUNCATED, None, None
        if s < 16:
            lengths.append(s)
            continue
        if s == 16:
            if not lengths:
                return BAD_CODELEN_SET, None, None
            value, repeat = lengths[-1], 3 + reader.take(2)
        elif s == 17:
            value, repeat = 0, 3 + reader.take(3)
        else:
            value, repeat = 0, 11 + reader.take(7)
        if reader.truncated:
            return TRUNCATED, None, None
        if len(lengths) + repeat > nlen + ndist:
            return BAD_CODELEN_SET, None, None
        lengths.extend([value] * repeat)
    if lengths[256] == 0:
        return NO_END_OF_BLOCK, None, None
    kind, longest, dist = _code_set(lengths[nlen:])
    if kind < 0 or (kind > 0 and longest > 1):
        return BAD_DIST_SET, None, None
    kind, longest, lit = _code_set(lengths[:nlen])
    if kind < 0 or (kind > 0 and longest != 1):
        return BAD_LITLEN_SET, None, None
    return OK, lit, dist


_FIXED = None


def inflate(data, expect):
    """(status, output) of the raw deflate stream `data`, of which `expect` bytes are expected: zlib's acceptance rules,
    the first defect as the library's status code, the output up to it"""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_code_set(FIXED_LIT)[2], _code_set(FIXED_DIST)[2])
    reader, out = _Reader(data), bytearray()
    while True:
        last, kind = reader.take(1), reader.take(2)
        if reader.truncated:
            return TRUNCATED, bytes(out)
        if kind == 3:
            return BAD_BLOCK_TYPE, bytes(out)
        if kind == 0:
            reader.pos = (reader.pos + 7) & ~7
            at = reader.pos >> 3
            size, inverse = reader.take(16), reader.take(16)
            if reader.truncated:
                return TRUNCATED, bytes(out)
            if size ^ 0xffff != inverse:
                return STORED_LENGTH, bytes(out)
            if at + 4 + size > len(reader.data):
                return TRUNCATED, bytes(out)
            if len(out) + size > expect:
                return OUTPUT_OVER, bytes(out)
            out += reader.data[at + 4:at + 4 + size]
            reader.pos = 8 * (at + 4 + size)
        else:
            if kind == 1:
                lit, dist = _FIXED
            else:
                status, lit, dist = _dynamic(reader)
                if status:
                    return status, bytes(out)
            while True:
                s = _decode(reader, lit)
                if reader.truncated:
                    return TRUNCATED, bytes(out)
                if s < 0 or s > 285:
                    return BAD_SYMBOL, bytes(out)
                if s < 256:
                    if len(out) >= expect:
                        return OUTPUT_OVER, bytes(out)
                    out.append(s)
                    continue
                if s == 256:
                    break
                length = LENGTH_BASE[s - 257] + reader.take(LENGTH_EXTRA[s - 257])
                if reader.truncated:
                    return TRUNCATED, bytes(out)
                d = _decode(reader, dist)
                if reader.truncated:
                    return TRUNCATED, bytes(out)
                if d < 0 or d > 29:
                    return BAD_SYMBOL, bytes(out)
                distance = DIST_BASE[d] + reader.take(DIST_EXTRA[d])
                if reader.truncated:
                    return TRUNCATED, bytes(out)
                if distance > len(out):
                    return DISTANCE_TOO_FAR, bytes(out)
                if len(out) + length > expect:
                    return OUTPUT_OVER, bytes(out)
                if distance >= length:
                    out += out[len(out) - distance:len(out) - distance + length]
                else:
                    for _ in range(length):
                        out.append(out[-distance])
        if last:
            break
    return (OUTPUT_UNDER if len(out) < expect else OK), bytes(out)


def raw_sums(data):
    """(s1, s2) as rw_png_inflate_u8 reports them: sum d_k and sum (n - k) d_k mod 65521"""
    d = numpy.frombuffer(bytes(data), dtype=numpy.uint8).astype(numpy.int64)
    n = len(d)
    return int(d.sum() % 65521), int(((n - numpy.arange(n)) % 65521 * d).sum() % 65521)


# ---- the filters
def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(stream, h, w, channels):
    """(status, pixels (h, w, 3) uint8) of a filtered stream: h rows of a type byte and channels * w bytes"""
    rows = numpy.frombuffer(bytes(stream), dtype=numpy.uint8).reshape(h, 1 + channels * w)
    out = numpy.zeros((h, channels * w), dtype=numpy.int64)
    status, bpp = OK, channels
    for y in range(h):
        kind, x = int(rows[y, 0]), rows[y, 1:].astype(numpy.int64)
        above = out[y - 1] if y else numpy.zeros_like(x)
        if kind > 4:
            status, kind = BAD_FILTER, 0
        if kind == 0:
            out[y] = x
        elif kind == 1:
            out[y] = numpy.cumsum(x.reshape(w, bpp), axis=0).reshape(-1) & 0xff
        elif kind == 2:
            out[y] = (x + above) & 0xff
        else:
            row = [0] * len(x)
            xs, bs = x.tolist(), above.tolist()
            for i in range(len(xs)):
                a = row[i - bpp] if i >= bpp else 0
                c = bs[i - bpp] if i >= bpp else 0
                row[i] = (xs[i] + ((a + bs[i]) >> 1 if kind == 3 else _paeth(a, bs[i], c))) & 0xff
            out[y] = row
    pixels = out.astype(numpy.uint8).reshape(h, w, channels)
    return status, numpy.ascontiguousarray(numpy.repeat(pixels, 3, axis=2) if channels == 1 else pixels[:, :, :3])


def png_decode(files_or_spans, h, w, channels, device='cpu', timings=None):
    """hip.png_decode on the host: (pixels (B, h, w, 3) as a CPU tensor, status (B, 4) int64)"""
    import torch
    if isinstance(files_or_spans, tuple):
        coded, spans = files_or_spans
        coded = bytes(coded.cpu().numpy().tobytes()) if hasattr(coded, 'cpu') else bytes(coded)
        streams = [coded[int(o):int(o) + int(n)] for o, n in numpy.asarray(spans).reshape(-1, 2)]
    else:
        streams = [bytes(s) for s in files_or_spans]
    expect = h * (1 + channels * w)
    pixels = numpy.zeros((len(streams), h, w, 3), dtype=numpy.uint8)
    status = numpy.zeros((len(streams), 4), dtype=numpy.int64)
    for i, s in enumerate(streams):
        code, out = inflate(s, expect)
        if code == OK:
            code, pixels[i] = unfilter(out, h, w, channels)
        status[i] = (code, len(out)) + raw_sums(out)
    return torch.from_numpy(pixels), status


# ---- building deflate streams
class _Bits:
    def __init__(self):
        self.out, self.acc, self.fill = bytearray(), 0, 0

    def put(self, value, bits):
        self.acc |= value << self.fill
        self.fill += bits
        while self.fill >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.fill -= 8

    def align(self):
        if self.fill:
            self.put(0, 8 - self.fill)

    def tobytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.fill else b'')


def _stream_codes(lengths):
    """Per symbol (bits in stream order, length) of the canonical code; the bits are cut to the length where the set is
    over-subscribed (such a stream is refused before any of its symbols is read)"""
    lengths = numpy.asarray(lengths, dtype=numpy.int64)
    codes = pngcode.canonical_codes(lengths) & ((1 << lengths) - 1)
    return [(int(c), int(v)) for c, v in zip(pngcode.reversed_codes(codes, lengths), lengths)]


def _length_symbol(length):
    s = max(k for k in range(29) if LENGTH_BASE[k] <= length)
    if length == 258:
        s = 28
    return 257 + s, LENGTH_EXTRA[s], length - LENGTH_BASE[s]


def _distance_symbol(distance):
    s = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return s, DIST_EXTRA[s], distance - DIST_BASE[s]


class Deflate:
    """A raw deflate stream, block by block.  ops: an int is a literal; (length, distance) a match; ('symbol', s) the
    bare code of literal/length symbol s; ('match', length, distance symbol, extra value) a match whose distance is
    given as its symbol.  The end-of-block is written unless end=False."""

    def __init__(self):
        self.bits = _Bits()

    def stored(self, data, final=False, nlen=None):
        self.bits.put(int(final), 1)
        self.bits.put(0, 2)
        self.bits.align()
        self.bits.put(len(data), 16)
        self.bits.put(len(data) ^ 0xffff if nlen is None else nlen, 16)
        self.bits.out += bytes(data)
        return self

    def _ops(self, ops, lit, dist, end):
        for op in ops:
            if isinstance(op, tuple) and op[0] == 'symbol':
                self.bits.put(*lit[op[1]])
            elif isinstance(op, tuple) and op[0] == 'match':
                symbol, extra, value = _length_symbol(op[1])
                self.bits.put(*lit[symbol])
                self.bits.put(value, extra)
                self.bits.put(*dist[op[2]])
                self.bits.put(op[3], DIST_EXTRA[op[2]] if op[2] < 30 else 0)
            elif isinstance(op, tuple):
                symbol, extra, value = _length_symbol(op[0])
                self.bits.put(*lit[symbol])
                self.bits.put(value, extra)
                symbol, extra, value = _distance_symbol(op[1])
                self.bits.put(*dist[symbol])
                self.bits.put(value, extra)
            else:
                self.bits.put(*lit[int(op)])
        if end:
            self.bits.put(*lit[256])

    def fixed(self, ops, final=False, end=True):
        self.bits.put(int(final), 1)
        self.bits.put(1, 2)
        self._ops(ops, _stream_codes(FIXED_LIT), _stream_codes(FIXED_DIST), end)
        return self

    def dynamic(self, ops, lit_lengths, dist_lengths, final=False, end=True, sequence=None, cl_lengths=None, hlit=None,
                hdist=None):
        """lit_lengths (257 .. 286 of them), dist_lengths (1 .. 30).  sequence: the code-length symbols as
        pngcode.run_lengths gives them [(symbol, extra bits, value)] (default: run_lengths over both sets joined, so a
        run goes from the literal lengths into the distance lengths where they agree); cl_lengths: the 19 lengths of
        the code-length code (default: a complete code for the sequence's counts); hlit / hdist: the header fields, if
        they are to lie."""
        lit_lengths, dist_lengths = [int(v) for v in lit_lengths], [int(v) for v in dist_lengths]
        if sequence is None:
            sequence = pngcode.run_lengths(lit_lengths + dist_lengths)
        if cl_lengths is None:
            counts = numpy.zeros(19, dtype=numpy.int64)
            for symbol, _, _ in sequence:
                counts[symbol] += 1
            cl_lengths = pngcode.limited_lengths(counts, pngcode.MAX_CODELEN_BITS)
        cl = _stream_codes(cl_lengths)
        hclen = 19
        while hclen > 4 and cl_lengths[pngcode.CODELEN_ORDER[hclen - 1]] == 0:
            hclen -= 1
        self.bits.put(int(final), 1)
        self.bits.put(2, 2)
        self.bits.put(len(lit_lengths) - 257 if hlit is None else hlit, 5)
        self.bits.put(len(dist_lengths) - 1 if hdist is None else hdist, 5)
        self.bits.put(hclen - 4, 4)
        for symbol in pngcode.CODELEN_ORDER[:hclen]:
            self.bits.put(int(cl_lengths[symbol]), 3)
        for symbol, extra, value in sequence:
            self.bits.put(*cl[symbol])
            self.bits.put(value, extra)
        pad = [0] * 32
        self._ops(ops, _stream_codes(lit_lengths + pad)[:len(lit_lengths) + 32], _stream_codes(dist_lengths + pad), end)
        return self

    def tobytes(self):
        return self.bits.tobytes()


def flat_lengths(used, bits):
    """Code lengths of `bits` for the symbols of `used` (a complete code when there are 2 ** bits of them)"""
    lengths = [0] * (max(used) + 1)
    for s in used:
        lengths[s] = bits
    return lengths


# ---- building PNG files
def filter_stream(image, types):
    """The filtered stream of image (h, w, channels) uint8 with the filter type types[y] for row y (types above 4 are
    written as they are, the row unfiltered)"""
    h, w, channels = image.shape
    rows = image.reshape(h, w * channels).astype(numpy.int64)
    out = numpy.zeros((h, 1 + w * channels), dtype=numpy.uint8)
    zero = numpy.zeros(channels, dtype=numpy.int64)
    for y in range(h):
        x = rows[y]
        b = rows[y - 1] if y else numpy.zeros_like(x)
        a, c = numpy.concatenate([zero, x])[:len(x)], numpy.concatenate([zero, b])[:len(x)]
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        paeth = numpy.where((pa <= pb) & (pa <= pc), a, numpy.where(pb <= pc, b, c))
        pred = {0: 0 * x, 1: a, 2: b, 3: (a + b) >> 1, 4: paeth}.get(int(types[y]), 0 * x)
        out[y, 0] = types[y]
        out[y, 1:] = (x - pred) & 0xff
    return out.tobytes()


def chunk(kind, data, crc=None):
    crc = zlib.crc32(kind + data) & 0xffffffff if crc is None else crc
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', crc)


def png_container(w, h, idat, colour=2, depth=8, interlace=0, split=None, between=b'', before=b''):
    """The file around a zlib stream: IHDR, the IDAT (cut at the offsets of `split`, `between` put after every piece
    but the last), IEND.  `before`: chunks between IHDR and the first IDAT."""
    cuts = [0] + list(split or []) + [len(idat)]
    pieces = [chunk(b'IDAT', idat[a:b]) for a, b in zip(cuts, cuts[1:])]
    return b''.join([pngcode.SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, colour, 0, 0, interlace)), before,
                     between.join(pieces), chunk(b'IEND', b'')])


def zlib_wrap(deflate, stream, adler=None):
    adler = zlib.adler32(stream) & 0xffffffff if adler is None else adler
    return b'\x78\x01' + deflate + struct.pack('>I', adler)


def png_file(image, types=None, level=6, deflate=None, adler=None, **container):
    """A PNG file of image (h, w, channels) uint8, channels 1, 3 or 4, with filter type types[y] for row y (default:
    y % 5) -- compressed by zlib at `level`, or carrying the raw deflate stream `deflate` one built by hand"""
    image = numpy.ascontiguousarray(image, dtype=numpy.uint8)
    h, w, channels = image.shape
    types = [y % 5 for y in range(h)] if types is None else list(types)
    stream = filter_stream(image, types)
    if deflate is None:
        packer = zlib.compressobj(level, zlib.DEFLATED, -15)
        deflate = packer.compress(stream) + packer.flush()
    return png_container(w, h, zlib_wrap(deflate, stream, adler), colour={1: 0, 3: 2, 4: 6}[channels], **container)


# ---- the corpus the host tests and the device tests share
def random_image(h, w, channels=3, seed=0):
    return numpy.random.RandomState(seed).randint(0, 256, (h, w, channels)).astype(numpy.uint8)


def smooth_image(h, w, seed, period=128):
    """png_checks.lowpass_noise, tiled: smooth content with a seam every `period` pixels"""
    from tests import png_checks
    tile = png_checks.lowpass_noise(period, seed)
    return numpy.ascontiguousarray(numpy.tile(tile, (-(-h // period), -(-w // period), 1))[:h, :w])


def pil_file(image, **save):
    """What PIL writes for image (h, w, 1 | 3 | 4) uint8 with the options `save` of its PNG plugin"""
    import io
    import PIL.Image
    image = numpy.asarray(image)
    mode = {1: 'L', 3: 'RGB', 4: 'RGBA'}[image.shape[2]]
    buf = io.BytesIO()
    PIL.Image.fromarray(image[:, :, 0] if mode == 'L' else image, mode).save(buf, format='png', **save)
    return buf.getvalue()


def pil_pixels(file_bytes):
    import io
    import PIL.Image
    with PIL.Image.open(io.BytesIO(file_bytes)) as im:
        return numpy.asarray(im.convert('RGB'), dtype=numpy.uint8)


PIL_OPTIONS = (dict(compress_level=1), dict(compress_level=6), dict(compress_level=9), dict(optimize=True))
EDGE_SHAPES = ((31, 352, 32767), (32, 341, 32768), (99, 110, 32769))       # H (1 + 3 W) around the window's 32 768


def corpus():
    """[(name, file)]: the files whose decoding is compared with PIL's, on the host (the twin) and on the device"""
    files = []
    for h, w in ((1, 1), (1, 2), (2, 1), (3, 5), (7, 33)):
        for k, options in enumerate(PIL_OPTIONS):
            files.append(('random %dx%d %s' % (h, w, options), pil_file(random_image(h, w, seed=h * w + k), **options)))
    files.append(('random 160x160', pil_file(random_image(160, 160, seed=5))))          # > 64 KiB coded: several IDATs
    smooth = smooth_image(40, 300, seed=8)
    for options in PIL_OPTIONS:
        files.append(('smooth 40x300 %s' % options, pil_file(smooth, **options)))
    files.append(('flat 40x300', pil_file(numpy.full((40, 300, 3), 77, numpy.uint8), compress_level=1)))
    files.append(('smooth 90x364', pil_file(numpy.tile(smooth_image(30, 364, seed=9), (3, 1, 1)))))
    for h, w, length in EDGE_SHAPES:
        assert h * (1 + 3 * w) == length
        files.append(('random %dx%d' % (h, w), pil_file(random_image(h, w, seed=length))))
        files.append(('smooth %dx%d' % (h, w), pil_file(smooth_image(h, w, seed=length % 100))))
    picture = smooth_image(7, 33, seed=4, period=16)
    for kind in range(5):
        files.append(('filter %d 7x33' % kind, png_file(picture, types=[kind] * 7)))
    for channels in (1, 3, 4):
        files.append(('channels %d 7x33' % channels, pil_file(random_image(7, 33, channels, seed=channels))))
        files.append(('channels %d filters 7x33' % channels, png_file(smooth_image(7, 33, 3, 16)[:, :, [0, 1, 2, 0][:channels]])))
    return files


def hand_streams():
    """[(name, raw deflate stream, its output)]: streams no encoder writes, from the builder; zlib accepts each"""
    rng = numpy.random.RandomState(11)
    streams = []
    block = bytes(rng.randint(0, 256, 32768, dtype=numpy.uint8))
    out = bytearray(block)
    for length in (258, 3):
        out += out[len(out) - 32768:len(out) - 32768 + length]
    streams.append(('stored 32768 then matches at 32768',
                    Deflate().stored(block).fixed([(258, 32768), (3, 32768)], final=True).tobytes(), bytes(out)))
    for d in (1, 2, 3, 63, 64, 65):
        literals = [int(v) for v in rng.randint(0, 144, d)]
        out = bytearray(literals)
        for _ in range(258):
            out.append(out[-d])
        streams.append(('%d literals then (258, %d)' % (d, d), Deflate().fixed(literals + [(258, d)], final=True).tobytes(), bytes(out)))
    streams.append(('empty stored block between two', Deflate().fixed([1, 2, 3]).stored(b'').fixed([4, 5], final=True).tobytes(),
                    bytes([1, 2, 3, 4, 5])))
    streams.append(('empty final fixed block', Deflate().fixed([7, 8, 9]).fixed([], final=True).tobytes(), bytes([7, 8, 9])))
    four = flat_lengths([65, 66, 256, 257], 2)
    streams.append(('one distance code of length 1', Deflate().dynamic([65, 66, 65, (3, 1)], four, [1], final=True).tobytes(),
                    b'ABAAAA'))
    streams.append(('no distance code, literals only',
                    Deflate().dynamic([65, 66, 67, 67], flat_lengths([65, 66, 67, 256], 2), [0], final=True).tobytes(), b'ABCC'))
    assert (16, 2, 2) in pngcode.run_lengths(four + [2, 2, 2, 2])[-1:]       # 2, then 16 x 5: over [257] and the four distances
    streams.append(('repeat from the literal into the distance lengths',
                    Deflate().dynamic([65, 66, (3, 2), 65], four, [2, 2, 2, 2], final=True).tobytes(), b'ABABAA'))
    return streams


DEFECT_SHAPE = (7, 33, 3)        # every defect is sent as a stream of this shape: expect = 700


def defect_streams():
    """[(name, raw deflate stream)] with exactly one defect each, for expect = 700; zlib refuses each (or gives another
    length)"""
    expect = DEFECT_SHAPE[0] * (1 + DEFECT_SHAPE[2] * DEFECT_SHAPE[1])
    body = filter_stream(smooth_image(7, 33, 2, 16), [y % 5 for y in range(7)])
    assert len(body) == expect

    def packed(data, level=9):
        packer = zlib.compressobj(level, zlib.DEFLATED, -15)
        return packer.compress(data) + packer.flush()
    text = bytes(numpy.random.RandomState(3).randint(97, 105, 700, dtype=numpy.uint8))
    dynamic = packed(text)
    assert dynamic[0] & 6 == 4                                               # a dynamic block
    lits = [65, 66, 67, 68, 69]
    plain = flat_lengths([65, 66, 67, 256], 2)
    return [
        ('block type 3', b'\x07'),
        ('LEN / NLEN mismatch', Deflate().stored(body, final=True, nlen=0).tobytes()),
        ('cut in a dynamic header', dynamic[:3]),
        ('cut inside a symbol', Deflate().fixed(lits + [(20, 5)], final=True).tobytes()[:7]),
        ('cut inside the extra bits', Deflate().fixed(lits + [('match', 3, 29, 0)], final=True).tobytes()[:8]),
        ('over-subscribed literal set', Deflate().dynamic([], flat_lengths([65, 66, 67, 256], 1), [0], final=True).tobytes()),
        ('incomplete literal set', Deflate().dynamic([], flat_lengths([65, 66, 256], 2), [0], final=True).tobytes()),
        ('no end-of-block code', Deflate().dynamic([], flat_lengths([65, 66, 67, 68], 2) + [0] * 188, [0], final=True,
                                                   end=False).tobytes()),
        ('repeat 16 first', Deflate().dynamic([], plain, [0], final=True, end=False,
                                              sequence=[(16, 2, 0), (0, 0, 0)]).tobytes()),
        ('repeat past the count', Deflate().dynamic([], plain, [0], final=True, end=False,
                                                    sequence=[(18, 7, 127), (18, 7, 127)]).tobytes()),
        ('literal/length symbol 286', Deflate().fixed([65, ('symbol', 286)], final=True).tobytes()),
        ('distance symbol 30', Deflate().fixed([65, 66, 67, ('match', 3, 30, 0)], final=True).tobytes()),
        ('distance one past the start', Deflate().fixed([65, 66, 67, (3, 4)], final=True).tobytes()),
        ('one byte too many', packed(body + b'\x00')),
        ('one byte too few', packed(body[:-1])),
    ]


# ---- the host program (rewriting_amd/csrc/rw_pngdec_host.cpp)
def build_host_program(directory, compiler='c++', sanitize=False):
    """Builds the stand-alone program into `directory`; returns its path, or None if the sanitizer runtime will not link"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = os.path.join(root, 'rewriting_amd', 'csrc', 'rw_pngdec_host.cpp')
    target = os.path.join(str(directory), 'rw_pngdec_host')
    flags = ['-O1', '-g', '-std=c++17', '-I', os.path.dirname(source)]
    if sanitize:
        flags += ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    done = subprocess.run([compiler] + flags + [source, '-o', target], capture_output=True, text=True)
    if done.returncode != 0:
        if sanitize and ('asan' in done.stderr or 'ubsan' in done.stderr or 'sanitize' in done.stderr):
            return None
        raise RuntimeError('%s failed:\n%s' % (compiler, done.stderr))
    return target


def run_host_program(program, cases, directory):
    """[(status, produced, adler)] of the program over cases [(stream, expect)]; its exit code must be 0 and its stderr
    empty (a sanitizer report is neither)"""
    import os
    import subprocess
    path = os.path.join(str(directory), 'cases.bin')
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for stream, expect in cases:
            f.write(struct.pack('<II', len(stream), expect) + bytes(stream))
    done = subprocess.run([program, path], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == '', 'exit %d\n%s' % (done.returncode, done.stderr[-4000:])
    lines = done.stdout.split()
    assert len(lines) == 3 * len(cases)
    return [tuple(int(v) for v in lines[3 * i:3 * i + 3]) for i in range(len(cases))]


def twin_result(stream, expect):
    """(status, produced, adler) as the host program prints them"""
    status, out = inflate(stream, expect)
    return status, len(out), zlib.adler32(out) & 0xffffffff
