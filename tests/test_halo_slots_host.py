"""The halo staging rule of the direct fp32 convolutions on the host.  csrc/rw_common.h states it once -- rw_halo_slot_of(),
which conv_halo_kernel, conv_up_halo_kernel and conv_halo_bf16x6_kernel (rw_conv.hip) call for each of a thread's slots --
and it is host-callable: a stand-alone program prints every slot's (global offset, mask, LDS offset) for a patch shape and
a tile, and the table must stage every patch position exactly once, zero what lies outside the image from a legal address,
and park the slots past the patch where no tap reads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)

XW = {32: 36, 16: 20, 8: 12}                         # LDS row pitch of a TW-wide tile
# (TW, TH) of every instantiation the launchers choose: stride 1 (patch (TH + 2) x (TW + 2)), quad tiles (TH + 1) x (TW + 1)
STRIDE1_TILES = [(32, 4), (32, 8), (32, 16), (16, 8), (16, 16), (16, 32), (8, 8)]
UP_TILES = [(32, 4), (32, 8), (16, 8), (16, 16), (8, 8)]
MAPS = [(5, 7), (9, 13), (24, 33)]                   # (h, w)

PROGRAM = r'''
#include "rw_common.h"
#include <cstdio>
#include <cstdlib>
// argv: groups of XH XW XUSED y0 x0 h w; per group one line per slot of the 256 threads: goff mask lds
int main(int argc, char** argv) {
  for (int i = 1; i + 6 < argc; i += 7) {
    int a[7];
    for (int k = 0; k < 7; ++k) a[k] = atoi(argv[i + k]);
    const int pslot = (a[0] * a[2] + 255) / 256;
    printf("config %d\n", pslot * 256);
    for (int pos = 0; pos < pslot * 256; ++pos) {
      int goff, lds;
      float mask;
      rw_halo_slot_of(pos, a[3], a[4], a[5], a[6], a[0], a[1], a[2], goff, mask, lds);
      printf("%d %a %d\n", goff, mask, lds);
    }
  }
  return 0;
}
'''


def _configs():
    """(up, TW, TH, y0, x0, h, w): the corner tiles and an interior one of every map, for every tile shape"""
    out = []
    for up, tiles in ((False, STRIDE1_TILES), (True, UP_TILES)):
        for tw, th in tiles:
            for h, w in MAPS:
                ty_last, tx_last = (h - 1) // th, (w - 1) // tw
                for ty, tx in sorted({(0, 0), (ty_last, tx_last), (ty_last // 2, tx_last // 2)}):
                    out.append((up, tw, th, ty * th, tx * tw, h, w))
    return out


CONFIGS = _configs()


def _patch(up, tw, th):
    return (th + 1, XW[tw], tw + 1) if up else (th + 2, XW[tw], tw + 2)          # XH, XW, XUSED


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    if HIPCC is None:
        pytest.skip('no hipcc')
    d = tmp_path_factory.mktemp('halo_slots_host')
    src, exe = str(d / 'slots.hip'), str(d / 'slots')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'rewriting_amd', 'csrc'),
                        src, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    args = []
    for up, tw, th, y0, x0, h, w in CONFIGS:
        args += [str(v) for v in _patch(up, tw, th) + (y0, x0, h, w)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, lines = [], iter(r.stdout.splitlines())
    for line in lines:
        n = int(line.split()[1])
        rows = [next(lines).split() for _ in range(n)]
        out.append([(int(g), float.fromhex(m), int(l)) for g, m, l in rows])
    assert len(out) == len(CONFIGS)
    return out


def test_the_configurations_cover_the_shapes_and_the_tiles():
    assert {(c[1], _patch(*c[:3])[1], _patch(*c[:3])[2]) for c in CONFIGS if not c[0]} == {(32, 36, 34), (16, 20, 18), (8, 12, 10)}
    assert {(c[1], _patch(*c[:3])[2]) for c in CONFIGS if c[0]} == {(32, 33), (16, 17), (8, 9)}
    for h, w in MAPS:
        mine = [c for c in CONFIGS if c[5:] == (h, w)]
        assert any(c[3] == 0 and c[4] == 0 for c in mine)
        assert any(c[3] + c[2] >= h and c[4] + c[1] >= w for c in mine)
    # an interior tile: no edge of the image inside its patch
    assert any(c[3] >= 1 and c[4] >= 1 and c[3] + c[2] + 1 <= c[5] and c[4] + c[1] + 1 <= c[6] for c in CONFIGS)


def test_every_patch_position_is_staged_once_and_the_padding_is_zeroed(tables):
    for cfg, table in zip(CONFIGS, tables):
        up, tw, th, y0, x0, h, w = cfg
        xh, xw, xused = _patch(up, tw, th)
        npos = xh * xused
        assert len(table) == -(-npos // 256) * 256 >= npos, cfg
        written = [lds for _, _, lds in table[:npos]]
        assert sorted(written) == sorted(r * xw + c for r in range(xh) for c in range(xused)), cfg
        assert len(set(written)) == npos, cfg
        for pos, (goff, mask, lds) in enumerate(table[:npos]):
            r, c = divmod(pos, xused)
            assert lds == r * xw + c, (cfg, pos)
            iy, ix = y0 - 1 + r, x0 - 1 + c
            if 0 <= iy < h and 0 <= ix < w:
                assert mask == 1.0 and goff == iy * w + ix, (cfg, pos)
            else:
                assert mask == 0.0 and 0 <= goff < h * w, (cfg, pos)


def test_the_slots_past_the_patch_land_where_no_tap_reads(tables):
    for cfg, table in zip(CONFIGS, tables):
        up, tw, th, y0, x0, h, w = cfg
        xh, xw, xused = _patch(up, tw, th)
        # LDS offsets the tile's lanes read: output (row, col) of the tile, stride 1 at (row + dy + 1, col + dx + 1) for the
        # nine taps, the quad tiles at (row + 1 + dy, col + 1 + dx) for the four shifts {0, -1}^2
        shifts = [(dy, dx) for dy in (-1, 0) for dx in (-1, 0)] if up else [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        read = {(row + 1 + dy) * xw + (col + 1 + dx) for row in range(th) for col in range(tw) for dy, dx in shifts}
        assert max(read) < xh * xw, cfg
        past = table[xh * xused:]
        for goff, mask, lds in past:
            assert lds == xw - 1 and mask == 0.0 and 0 <= goff < h * w, cfg
        assert not ({lds for _, _, lds in past} & read), cfg
        # and what the taps read is what was staged
        assert read <= {lds for _, _, lds in table[:xh * xused]}, cfg
