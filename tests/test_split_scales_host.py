"""The scale rule of the split-operand kernels on the host.  csrc/rw_common.h states it once -- rw_exp_above(), which
rw_split_scales<headroom>() (every kernel body) and rw_weight_scale_of() (the pack entries) go through -- and both are
host-callable: a stand-alone program prints what they give at the edges of fp32, and the documented arithmetic
(tests/split_model.py, through hip_emulation._input_exp) must give the same exponents for the headrooms 14 / 8 / 12."""
import math
import os
import shutil
import subprocess

import pytest
import torch

from tests import hip_emulation as E
from tests import split_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)

# 0; the smallest denormal; the smallest normal; just below and at a power of two; the largest f16; the clamp; infinity
INPUTS = ['0x0p+0', '0x1p-149', '0x1p-126', '0x1.fffffep-1', '0x1p+0', '0x1.ffcp+15', '0x1p+100', '0x1p+101', '0x1p+127', 'inf']

PROGRAM = r'''
#include "rw_common.h"
#include <cstdio>
#include <cstdlib>
template <int HEAD> static void scales(float am) {
  float in_scale, out_scale;
  rw_split_scales<HEAD>(am, 1.f, in_scale, out_scale);
  printf(" %a %a", in_scale, out_scale);
}
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const float am = strtof(argv[i], nullptr);
    printf("%a %d", am, rw_exp_above(am));
    scales<14>(am); scales<8>(am); scales<12>(am);
    printf(" %a\n", rw_weight_scale_of(am));
  }
  return 0;
}
'''


@pytest.fixture(scope='module')
def host_rows(tmp_path_factory):
    if HIPCC is None:
        pytest.skip('no hipcc')
    d = tmp_path_factory.mktemp('split_scales_host')
    src, exe = str(d / 'scales.hip'), str(d / 'scales')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'rewriting_amd', 'csrc'),
                        src, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe] + INPUTS, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(INPUTS)
    return rows


def test_the_exponent_and_the_scales_are_the_models(host_rows):
    """e and 2^(+-(headroom - e)) against top - e of the model, input by input; the clamp keeps every scale a normal float"""
    assert sorted(set(M.TOP.values())) == [8, 12, 14]
    for text, row in zip(INPUTS, host_rows):
        am = float.fromhex(text) if text != 'inf' else math.inf
        assert float.fromhex(row[0]) == am or (math.isinf(am) and row[0] == 'inf'), (text, row[0])
        e = int(row[1])
        for k, top in enumerate((14, 8, 12)):
            ev = int(E._input_exp(torch.full((E.BOUND_LANES,), am), torch.zeros(1, 1, 1, 1), None, top))
            assert top - e == ev, (text, top, e, ev)
            in_scale, out_scale = float.fromhex(row[2 + 2 * k]), float.fromhex(row[3 + 2 * k])
            assert in_scale == math.ldexp(1.0, ev) and out_scale == math.ldexp(1.0, -ev), (text, top, row)
            assert 2.0 ** -126 <= in_scale < math.inf and 2.0 ** -126 <= out_scale < math.inf


def test_the_exponents_at_the_edges(host_rows):
    """What the rule is documented to give: x < 2^e exactly at and below a power of two, -100 for zero and the denormals,
    100 from 2^100 on; the weight side maps an all-zero tensor to scale 1 and otherwise leaves 2^14 <= max |U| scale < 2^15"""
    e = {text: int(row[1]) for text, row in zip(INPUTS, host_rows)}
    assert e == {'0x0p+0': -100, '0x1p-149': -100, '0x1p-126': -100, '0x1.fffffep-1': 0, '0x1p+0': 1, '0x1.ffcp+15': 16,
                 '0x1p+100': 100, '0x1p+101': 100, '0x1p+127': 100, 'inf': 100}
    su = {text: float.fromhex(row[8]) for text, row in zip(INPUTS, host_rows)}
    assert su['0x0p+0'] == 1.0
    for text in ('0x1.fffffep-1', '0x1p+0', '0x1.ffcp+15'):
        assert 2.0 ** 14 <= float.fromhex(text) * su[text] < 2.0 ** 15, (text, su[text])
    assert su['0x1p-149'] == su['0x1p-126'] == 2.0 ** 115 and su['0x1p+101'] == su['inf'] == 2.0 ** -85
