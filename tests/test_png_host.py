"""The PNG format of the device encoder, on the host: tests/png_checks.py's numpy twin of the whole encoder (built on the
package's host builder, rewriting_amd/pngcode.py) gives files that PIL and zlib read back exactly, its two prefix codes
are complete and length-limited, and its files are about the size of PIL's.  tests/test_gpu_png.py holds hip.png_encode
to these bytes."""
import zlib

import numpy
import pytest

from rewriting_amd import _lib, hip, pngcode
from tests import png_checks as C


def _random(h, w, seed=0):
    return numpy.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(numpy.uint8)


def _ramp(h, w):
    y, x = numpy.mgrid[0:h, 0:w]
    return numpy.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) % 256], axis=2).astype(numpy.uint8)


SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (7, 33)]
PICTURES = ([('random_%dx%d' % s, _random(*s)) for s in SHAPES]
            + [('zeros_%dx%d' % s, numpy.zeros(s + (3,), dtype=numpy.uint8)) for s in SHAPES]
            + [('ones_%dx%d' % s, numpy.full(s + (3,), 255, dtype=numpy.uint8)) for s in SHAPES]
            + [('ramp_7x33', _ramp(7, 33)), ('ramp_40x300', _ramp(40, 300)),
               ('lowpass_noise_64', C.lowpass_noise(64, seed=1)), ('fibonacci_row', C.fibonacci_row())])


def _check_codes(details):
    assert C.kraft_is_one(details['lengths'], pngcode.MAX_LITERAL_BITS)
    assert C.kraft_is_one(details['cl_lengths'], pngcode.MAX_CODELEN_BITS)
    assert max(details['lengths']) <= pngcode.MAX_LITERAL_BITS and max(details['cl_lengths']) <= pngcode.MAX_CODELEN_BITS
    assert details['lengths'][pngcode.END_OF_BLOCK] > 0 and (details['lengths'][details['counts'] > 0] > 0).all()


@pytest.mark.parametrize('segment_bytes', [64, 1000, 16384])
@pytest.mark.parametrize('name,image', PICTURES, ids=[n for n, _ in PICTURES])
def test_twin_files_read_back_exactly(name, image, segment_bytes):
    png, stream, details = C.encode(image, segment_bytes)
    assert len(stream) == image.shape[0] * (1 + 3 * image.shape[1])
    assert len(details['segments']) == -(-len(stream) // segment_bytes)
    assert zlib.decompress(C.idat_of(png)) == stream
    assert numpy.array_equal(C.decode(png), image)
    _check_codes(details)


def test_filter_types_follow_the_minimum_sum_rule():
    # a picture that is constant along x codes with Sub (1), one constant along y with Up (2); row 0 has no row above:
    # there None / Up and Sub / Paeth tie in pairs and the lower type wins
    y, x = numpy.mgrid[0:6, 0:40]
    along_x = numpy.repeat(((37 * y + 5) % 251)[:, :, None], 3, axis=2).astype(numpy.uint8)
    along_y = numpy.repeat((37 * x % 251)[:, :, None], 3, axis=2).astype(numpy.uint8)
    assert C.filter_rows(along_x)[1][0] == 1
    assert list(C.filter_rows(along_y)[1][1:]) == [2] * 5
    assert C.filter_rows(numpy.zeros((3, 4, 3), dtype=numpy.uint8))[1].tolist() == [0, 0, 0]
    # byte by byte, as the PNG specification words it, on a picture with every kind of row
    image = numpy.concatenate([_random(3, 9, seed=5), along_x[:3, :9], along_y[:3, :9], C.lowpass_noise(9, seed=6)])
    stream, types = C.filter_rows(image)
    rows = image.reshape(len(image), -1).astype(int)
    for r in range(len(rows)):
        costs, coded = [], []
        for kind in range(5):
            out = []
            for i in range(rows.shape[1]):
                a = rows[r, i - 3] if i >= 3 else 0
                b = rows[r - 1, i] if r else 0
                c = rows[r - 1, i - 3] if r and i >= 3 else 0
                p = a + b - c
                paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
                out.append((rows[r, i] - [0, a, b, (a + b) // 2, paeth][kind]) % 256)
            coded.append(out)
            costs.append(sum(v if v < 128 else 256 - v for v in out))
        assert types[r] == costs.index(min(costs)), (r, costs)
        assert stream.reshape(len(rows), -1)[r].tolist() == [types[r]] + coded[types[r]]
    # the stream is what PIL undoes: the types written are the types used
    image = C.lowpass_noise(64, seed=2)
    stream, types = C.filter_rows(image)
    assert (numpy.frombuffer(stream, dtype=numpy.uint8).reshape(64, -1)[:, 0] == types).all()
    assert len(set(types.tolist())) > 1


def test_literal_code_is_limited_to_15_bits():
    """Fibonacci counts: a plain Huffman tree over the block's symbols is 16 deep; the built code stops at 15 and stays
    complete -- zlib takes the file."""
    image = C.fibonacci_row()
    png, stream, details = C.encode(image, 16384)
    assert 4000 < len(stream) < 5000
    assert C.unlimited_depth(details['counts']) > pngcode.MAX_LITERAL_BITS
    _check_codes(details)
    assert max(details['lengths']) == pngcode.MAX_LITERAL_BITS
    assert zlib.decompress(C.idat_of(png)) == stream and numpy.array_equal(C.decode(png), image)


def test_code_length_code_is_limited_to_7_bits():
    """A complete literal code whose length sequence has chain-like counts in the 19-symbol alphabet: a plain Huffman
    tree there is 8 deep; the built one stops at 7, stays complete, and zlib inflates a block under this header."""
    lengths = C.skewed_literal_lengths()
    assert len(lengths) == 257 and C.kraft_is_one(lengths, pngcode.MAX_LITERAL_BITS)
    counts = numpy.bincount([s for s, _, _ in pngcode.run_lengths(lengths + [0])], minlength=19)
    assert C.unlimited_depth(counts) > pngcode.MAX_CODELEN_BITS
    header, cl_lengths = pngcode.block_header(lengths)
    assert C.kraft_is_one(cl_lengths, pngcode.MAX_CODELEN_BITS)
    assert max(cl_lengths) == pngcode.MAX_CODELEN_BITS and (cl_lengths[counts > 0] > 0).all()
    data = [s for s in range(256) if lengths[s]] * 3
    block = C.coded_segment(data, header, pngcode.canonical_codes(lengths), lengths) + b'\x01\x00\x00\xff\xff'
    assert zlib.decompressobj(-15).decompress(block) == bytes(data)


def test_limited_lengths_properties():
    rng = numpy.random.RandomState(3)
    for trial in range(40):
        n = int(rng.randint(2, 258))
        counts = numpy.zeros(257, dtype=numpy.int64)
        counts[rng.choice(257, n, replace=False)] = (rng.pareto(0.4, n) * 3 + 1).astype(numpy.int64)
        for limit in (15, 12, 9):
            lengths = pngcode.limited_lengths(counts, limit)
            assert C.kraft_is_one(lengths, limit) and max(lengths) <= limit
            assert ((lengths > 0) == (counts > 0)).all()
            assert (pngcode.limited_lengths(counts.copy(), limit) == lengths).all()           # deterministic
        # where the plain tree fits the limit, the limited code costs the same
        if C.unlimited_depth(counts) <= 15:
            cost = int((pngcode.limited_lengths(counts, 15) * counts).sum())
            assert cost == _huffman_cost(counts)
    one = numpy.zeros(19, dtype=numpy.int64)
    one[18] = 5
    assert C.kraft_is_one(pngcode.limited_lengths(one, 7), 7)                                 # a lone symbol gets a partner


def _huffman_cost(counts):
    import heapq
    heap = [int(c) for c in counts if c > 0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        merged = heapq.heappop(heap) + heapq.heappop(heap)
        cost += merged
        heapq.heappush(heap, merged)
    return cost


def test_table_and_adler_fold():
    image = C.lowpass_noise(64, seed=4)
    _, stream, details = C.encode(image, 1000)
    row, lengths = pngcode.code_table(details['counts'][:256], int(details['counts'][256]))
    assert row.dtype == numpy.uint32 and len(row) == pngcode.TABLE_WORDS and row[0] == details['header_bits']
    assert (lengths == details['lengths']).all() and ((row[1:258] >> 16) == lengths).all()
    codes = pngcode.canonical_codes(lengths)
    for s in (0, 1, 255, 256):
        assert format(int(row[1 + s]) & 0xffff, '0%db' % lengths[s])[::-1] == format(codes[s], '0%db' % lengths[s])
    # the segments' sums fold to zlib's Adler-32, and the bound holds
    data = numpy.frombuffer(stream, dtype=numpy.uint8).astype(numpy.int64)
    parts = []
    for s in range(0, len(data), 1000):
        d = data[s:s + 1000]
        parts.append((len(d), int(d.sum()) % 65521, int((d * (len(d) - numpy.arange(len(d)))).sum()) % 65521))
    assert pngcode.adler_fold(parts) == zlib.adler32(stream) & 0xffffffff
    bound = pngcode.coded_bytes_bound(details['counts'][:256], lengths, int(row[0]), len(parts))
    total = sum(len(s) for s in details['segments'])
    assert total <= bound <= total + 8 * len(parts)
    assert pngcode.frame(64, 64, details['segments'], zlib.adler32(stream) & 0xffffffff) == C.encode(image, 1000)[0]


# Measured here (PIL 's default PNG, zlib level 6): the twin's file is 1.003 x PIL's on each of the three pictures
# (111 874 / 111 567, 111 843 / 111 434, 111 920 / 111 574 bytes).  The bar is that ratio plus 5 % for PIL / zlib
# version drift, nothing else.
SIZE_RATIO_MEASURED = 1.004
SIZE_RATIO_BAR = SIZE_RATIO_MEASURED * 1.05


def test_library_constants_match_the_host_builder():
    lib = _lib.load()
    assert hip.png_segment_bytes() == lib.rw_png_segment_bytes() == 16384
    assert lib.rw_png_table_words() == pngcode.TABLE_WORDS
    # a coded segment fits its slot: the header, 15 bits a byte, end-of-block, `000`, padding, 00 00 FF FF
    worst = (8 * pngcode.HEADER_BYTES + 15 * hip.png_segment_bytes() + 15 + 3 + 7) // 8 + 4
    assert worst <= lib.rw_png_segment_capacity() and lib.rw_png_segment_capacity() % 16 == 0


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_size_against_pil_on_lowpass_noise_256(seed):
    image = C.lowpass_noise(256, seed)
    png, _, _ = C.encode(image, hip.png_segment_bytes())
    ratio = len(png) / C.pil_png_size(image)
    print('twin %d bytes, PIL %d bytes, ratio %.4f (bar %.4f)' % (len(png), C.pil_png_size(image), ratio, SIZE_RATIO_BAR))
    assert ratio <= SIZE_RATIO_BAR


def test_routes_without_a_device_refuse():
    """Nothing falls back to a host encoder: bytes and images on the CPU are refused"""
    import torch
    from rewriting_amd import pngwriter
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.png_encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pngwriter.as_urls(torch.zeros(1, 3, 4, 4))
    assert pngwriter.as_url(b'abc') == 'data:image/png;base64,YWJj' and pngwriter.MAX_WRITERS == 16


# ---- what the C entries refuse (nothing is launched: the placeholder pointers are never dereferenced)
P = 0x10000
ENTRIES = {
    'rw_png_filter_u8': ['image', 'row_type', 'stream', 'hist_part', 'hist', 'adler', 'images', 'height', 'width', 'queue'],
    'rw_png_encode_u8': ['stream', 'table', 'coded', 'lengths', 'images', 'height', 'width', 'queue'],
    'rw_png_compact_u8': ['coded', 'lengths', 'adler', 'offsets', 'head', 'bytes', 'capacity', 'segments', 'queue'],
}
GOOD = dict(images=2, height=40, width=300, capacity=1 << 20, segments=6, queue=None)
BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
REFUSED = [
    ('rw_png_filter_u8', dict(image=None), BAD_ARGUMENT), ('rw_png_filter_u8', dict(adler=None), BAD_ARGUMENT),
    ('rw_png_filter_u8', dict(images=0), BAD_ARGUMENT), ('rw_png_filter_u8', dict(stream=P + 8), BAD_ARGUMENT),
    ('rw_png_filter_u8', dict(height=0), UNSUPPORTED), ('rw_png_filter_u8', dict(width=0), UNSUPPORTED),
    ('rw_png_filter_u8', dict(height=1, width=715827883), UNSUPPORTED),              # 1 + 3 W = 2^31 + 2
    ('rw_png_filter_u8', dict(height=1 << 15, width=21846), UNSUPPORTED),             # H (1 + 3 W) = 2^31 + 2^15
    ('rw_png_filter_u8', dict(image=None, height=0), BAD_ARGUMENT),                   # a bad argument is reported first
    ('rw_png_encode_u8', dict(table=None), BAD_ARGUMENT), ('rw_png_encode_u8', dict(images=-1), BAD_ARGUMENT),
    ('rw_png_encode_u8', dict(coded=P + 4), BAD_ARGUMENT), ('rw_png_encode_u8', dict(width=0), UNSUPPORTED),
    ('rw_png_encode_u8', dict(height=1, width=715827883), UNSUPPORTED),
    ('rw_png_compact_u8', dict(head=None), BAD_ARGUMENT), ('rw_png_compact_u8', dict(segments=0), BAD_ARGUMENT),
    ('rw_png_compact_u8', dict(capacity=-1), BAD_ARGUMENT), ('rw_png_compact_u8', dict(segments=1 << 31), BAD_ARGUMENT),
]


@pytest.mark.parametrize('entry,change,want', REFUSED, ids=['%s-%s' % (e[7:], '-'.join(sorted(c))) + str(i)
                                                           for i, (e, c, _) in enumerate(REFUSED)])
def test_entries_refuse(entry, change, want):
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    args = dict(GOOD, **change)
    status = int(getattr(_lib.load(), entry)(*[args.get(name, P) for name in ENTRIES[entry]]))
    assert status == want, (entry, change, status)
