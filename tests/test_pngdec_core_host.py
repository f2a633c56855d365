"""The inflate core (rewriting_amd/csrc/rw_inflate_core.h) on the CPU, outside Python: the stand-alone program
rw_pngdec_host.cpp, built here with the address and undefined-behaviour sanitizers, gives the twin's statuses, lengths and
Adler sums on the hand-made streams, the defects and the corpus, and survives 2 000 mutated streams without a report --
accepting exactly those that zlib accepts.  The kernel runs this same header (tests/test_gpu_pngdec.py)."""
import zlib

import numpy as np
import pytest

from rewriting_amd import pngreader
from tests import pngdec_checks as D


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    directory = tmp_path_factory.mktemp('pngdec_host')
    path = D.build_host_program(directory, compiler='c++', sanitize=True)
    if path is None:
        pytest.skip('the sanitizer runtime does not link here')
    return path, directory


def test_hand_made_streams_defects_and_corpus_equal_the_twin(program):
    path, directory = program
    cases = [(stream, len(out)) for _, stream, out in D.hand_streams()]
    cases += [(stream, 700) for _, stream in D.defect_streams()]
    for _, data in D.corpus():
        parsed = pngreader.parse(data)
        cases.append((bytes(parsed.span), parsed.h * (1 + parsed.channels * parsed.w)))
    # every good stream also with one byte more and one byte less expected
    cases += [(stream, len(out) + k) for _, stream, out in D.hand_streams() for k in (-1, 1) if len(out) + k > 0]
    got = D.run_host_program(path, cases, directory)
    for k, ((stream, expect), result) in enumerate(zip(cases, got)):
        assert result == D.twin_result(stream, expect), 'case %d' % k
    assert [r[0] for r in got[:12]] == [D.OK] * 12


def _seeds():
    picture = D.smooth_image(7, 33, seed=2, period=16)
    stream = D.filter_stream(picture, [y % 5 for y in range(7)])
    text = bytes(np.random.RandomState(3).randint(97, 105, 700, dtype=np.uint8))

    def packed(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
        packer = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        return packer.compress(data) + packer.flush()
    hand = {name: (s, len(out)) for name, s, out in D.hand_streams()}
    return [(packed(stream, 0), 700), (packed(text, 9, zlib.Z_FIXED), 700), (packed(text, 9), 700), (packed(stream, 6), 700),
            hand['one distance code of length 1'], hand['repeat from the literal into the distance lengths']]


def _accepted(stream, expect):
    unpacker = zlib.decompressobj(-15)
    try:
        out = unpacker.decompress(stream)
    except zlib.error:
        return False
    return unpacker.eof and len(out) == expect


def test_fuzz_on_the_cpu(program):
    path, directory = program
    seeds = _seeds()
    assert len(seeds) == 6 and all(_accepted(s, n) for s, n in seeds)
    assert sorted(set((s[0] >> 1) & 3 for s, _ in seeds)) == [0, 1, 2]           # stored, fixed and dynamic blocks
    rng = np.random.RandomState(20)
    cases = []
    for k in range(2000):
        stream, expect = seeds[k % 6]
        data, kind, at = bytearray(stream), (k // 6) % 4, int(rng.randint(0, len(stream)))
        if kind == 0:
            data[at] ^= 1 << int(rng.randint(0, 8)) if k % 2 else int(rng.randint(1, 256))
        elif kind == 1:
            del data[at:]
        elif kind == 2:
            data.insert(at, int(rng.randint(0, 256)))
        else:
            del data[at]
        cases.append((bytes(data), expect))
    got = D.run_host_program(path, cases, directory)                             # exit 0, nothing on stderr
    accepted = [_accepted(s, n) for s, n in cases]
    assert 20 < sum(accepted) < 1980                                             # both kinds occur
    for k, ((stream, expect), (status, produced, adler)) in enumerate(zip(cases, got)):
        assert (status == D.OK) == accepted[k], 'mutation %d of seed %d: status %d' % (k, k % 6, status)
        if status == D.OK:
            assert produced == expect and adler == zlib.adler32(zlib.decompressobj(-15).decompress(stream)) & 0xffffffff


def test_the_rocm_compiler_builds_it_too(tmp_path):
    import os
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('no ROCm clang++ here')
    path = D.build_host_program(tmp_path, compiler=clang, sanitize=False)
    name, stream, out = D.hand_streams()[0]
    assert D.run_host_program(path, [(stream, len(out))], tmp_path) == [D.twin_result(stream, len(out))]
