"""The op layer's dtype dispatch and the half / double kernels' code, without a GPU: which wrapper of rewriting_amd.hip
each op calls for its input's dtype, what it refuses before anything is launched, and the shipped code objects of the
new kernels (no packed arithmetic, no mixed-precision FMA)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch


def test_other_dtypes_are_refused_naming_the_three_that_are_taken():
    from rewriting_amd.utils.stylegan2 import op
    x = torch.randn(2, 4, 8, 8)
    for bad in (torch.bfloat16, torch.int32):
        with pytest.raises(RuntimeError, match='float16, float32 or float64'):
            op.fused_leaky_relu(x.to(bad), torch.zeros(4, dtype=bad))
        with pytest.raises(RuntimeError, match='float16, float32 or float64'):
            op.upfirdn2d(x.to(bad), torch.ones(2, 2, dtype=bad))


def test_operands_in_another_dtype_are_refused_not_converted():
    from rewriting_amd.utils.stylegan2 import op
    x = torch.randn(2, 4, 8, 8)
    with pytest.raises(RuntimeError, match='bias is torch.float32 and the input torch.float16'):
        op.fused_leaky_relu(x.half(), torch.zeros(4))
    with pytest.raises(RuntimeError, match='bias is torch.float16 and the input torch.float64'):
        op.fused_leaky_relu(x.double(), torch.zeros(4).half())
    with pytest.raises(RuntimeError, match='kernel is torch.float32 and the input torch.float16'):
        op.upfirdn2d(x.half(), torch.ones(2, 2))


@pytest.mark.parametrize('dtype, suffix', [(torch.float32, ''), (torch.float16, '_f16'), (torch.float64, '_f64')])
def test_each_dtype_reaches_its_own_wrappers(dtype, suffix, monkeypatch):
    """fp32 makes exactly the calls it made before (hip.fused_bias_act, hip.bias_grad, hip.upfirdn2d_major); half and
    double go to the _f16 / _f64 forms, forward and backward, and get their results in their own dtype."""
    from rewriting_amd import hip
    from rewriting_amd.utils.stylegan2 import op
    from tests import hip_emulation
    calls = []

    def recording(name, fn):
        def call(*args):
            calls.append(name)
            return fn(*args)
        return call
    for name in ('fused_bias_act', 'bias_grad', 'upfirdn2d_major'):
        for sfx in ('', '_f16', '_f64'):
            monkeypatch.setattr(hip, name + sfx, recording(name + sfx, getattr(hip_emulation, name)))
    x = torch.randn(2, 4, 6, 6, dtype=dtype, requires_grad=True)
    b = torch.zeros(4, dtype=dtype, requires_grad=True)
    y = op.upfirdn2d(op.fused_leaky_relu(x, b), torch.ones(2, 2, dtype=dtype) / 4, up=2, pad=(1, 0))
    y.backward(torch.ones_like(y))
    assert y.dtype == x.grad.dtype == b.grad.dtype == dtype
    assert sorted(set(calls)) == sorted(n + suffix for n in ('bias_grad', 'fused_bias_act', 'upfirdn2d_major'))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-objdump'), reason='no llvm-objdump')
def test_half_and_double_kernels_ship_without_packed_or_mixed_arithmetic():
    """rw_ops.hip's kernels run beside the convolutions' MFMAs (its header): the half forms compute in scalar fp32
    (v_cvt_f32_f16 on load, v_cvt_f16_f32 / v_cvt_pk_f16_f32 at the store) and the double forms in scalar f64 -- no v_pk_*
    arithmetic and no v_fma_mix*, whose rounding to half would not be the f32 result rounded once.  Checked on the code
    objects of the library that ships."""
    from rewriting_amd import _lib
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    assert os.path.isfile(_lib.LIB_PATH), 'build the library first (rewriting_amd/csrc/build.sh)'
    kernels = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(_lib.LIB_PATH, os.path.join(d, 'lib.so'))
        r = subprocess.run([objdump, '--offloading', 'lib.so'], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for f in sorted(f for f in os.listdir(d) if 'hipv4-amdgcn' in f):
            text = subprocess.run([objdump, '-d', '--mcpu=gfx950', f], cwd=d, capture_output=True, text=True).stdout
            for m in re.finditer(r'^[0-9a-f]+ <(_Z\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)', text, re.M | re.S):
                if re.search(r'(fused_bias_act|bias_grad|upfirdn2d\w*)_kernelI(DF16_|d)', m.group(1)):
                    kernels[m.group(1)] = m.group(2)
    assert len(kernels) == 2 * (2 + 1 + 6), sorted(kernels)   # f16, f64 x (vector + scalar, bias_grad, 6 upfirdn2d)
    for name, body in kernels.items():
        insns = [l.split()[0] for l in body.splitlines() if l.strip() and not l.lstrip().startswith(';')]
        bad = [i for i in insns if i.startswith('v_pk_') or '_mix' in i]
        assert not bad, (name, sorted(set(bad)))
        if 'IDF16_' in name:
            assert 'v_cvt_f32_f16' in body, name
