"""Half and double forms of the L1 ops (fused_bias_act, bias_grad, upfirdn2d) on the GPU.

Bars (include/rewriting_hip.h, "Three dtypes here"): an f16 result is the f32 kernel's result on the widened inputs,
rounded to half once -- bit for bit; f64 fused_bias_act is the three operations of oracle/restatement.py in float64 --
bit for bit; f64 upfirdn2d is within 1e-13 x max|y| of the restatement (its conv2d sums in another order); a half
bias gradient is within one half ulp of the float64 sum plus 1e-6 x sum|g| for the fp32 accumulation.  The adjoints
(op/upfirdn2d.py _adjoint_pads, the double backward of op/fused_act.py) go through torch.autograd.gradcheck and
gradgradcheck in float64."""
import itertools
import math

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SQRT2 = 2 ** 0.5
CODES = [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)]        # act * 10 + grad = 10, 11, 12, 30, 31, 32

# (shape, cut at an offset of one element): (4, 16, 8, 8) aligned takes the 16-byte vector path (n and step_b multiples
# of 8); the offset view, the odd sizes and step_b = 4, 15 or 1 take the scalar path
FBA_CASES = [((4, 16, 8, 8), False), ((4, 16, 8, 8), True), ((3, 5, 7, 3), False), ((2, 6, 2, 2), False),
             ((5, 7), False), ((2, 8, 3, 5), False)]

# (major, h, w, minor, up, down, kh, kw, pads) reaching every branch of the upfirdn2d launcher
UPFIRDN_CASES = [
    (3, 9, 9, 1, 2, 1, 4, 4, (2, 1, 2, 1)),       # up2k4, ragged width (scalar stores)
    (2, 40, 150, 1, 2, 1, 4, 4, (2, 1, 2, 1)),    # up2k4, two 256-column tiles, 16-byte rows
    (2, 17, 34, 1, 1, 1, 4, 4, (1, 1, 1, 1)),     # plane 1/1 (the generator's Blur), ragged width
    (2, 12, 20, 1, 2, 1, 3, 3, (1, 1, 1, 1)),     # plane 2/1
    (2, 19, 24, 1, 1, 2, 4, 4, (1, 2, 1, 2)),     # plane 1/2
    (2, 11, 13, 1, 2, 2, 3, 5, (2, 0, -1, 1)),    # plane 2/2
    (2, 9, 8, 2, 1, 1, 3, 3, (1, 1, 1, 1)),       # general walk: minor 2
    (3, 7, 9, 1, 3, 3, 5, 4, (2, 1, 1, 2)),       # general walk: up / down 3
    (1, 8, 11, 3, 3, 1, 4, 4, (0, 2, 1, 1)),      # general walk: minor 3, up 3
]


def _cut(shape, offset, dtype, gen):
    n = math.prod(shape)
    buf = torch.randn(n + 1, generator=gen, dtype=torch.float64).to(dtype).to(DEV)
    return (buf[1:] if offset else buf[:n]).view(shape)


def _rand(shape, dtype, gen):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(DEV)


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    ints = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return torch.equal(a.contiguous().view(ints), b.contiguous().view(ints))


def _half_ulp(v):
    """one ulp of binary16 at |v| (subnormal spacing below 2^-14)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def _check_half_sum(got, g, dims):
    """bias_grad's bar: within one half ulp of the float64 sum, plus 1e-6 x sum|g| for the fp32 accumulation"""
    assert got.dtype == torch.float16
    want = g.double().sum(dims).cpu()
    err = (got.double().cpu() - want).abs()
    bar = _half_ulp(want) + 1e-6 * g.double().abs().sum(dims).cpu()
    assert bool((err <= bar).all()), (err - bar).max().item()


def test_f16_fused_bias_act_is_the_f32_kernel_rounded_once():
    from rewriting_amd import hip
    from rewriting_amd.utils.stylegan2 import op
    gen = torch.Generator().manual_seed(0)
    for (shape, offset), (act, grad), with_bias in itertools.product(FBA_CASES, CODES, (False, True)):
        x = _cut(shape, offset, torch.float16, gen)
        ref = _cut(shape, False, torch.float16, gen)
        b = _rand((shape[1],), torch.float16, gen) if with_bias else None
        got = hip.fused_bias_act_f16(x, b, ref, act, grad, 0.2, SQRT2)
        want = hip.fused_bias_act(x.float(), None if b is None else b.float(), ref.float(), act, grad, 0.2, SQRT2)
        assert _same_bits(got, want.half()), (shape, offset, act, grad, with_bias)
    for shape, offset in FBA_CASES:
        x = _cut(shape, offset, torch.float16, gen)
        b = _rand((shape[1],), torch.float16, gen)
        got = op.fused_leaky_relu(x, b)
        assert _same_bits(got, op.fused_leaky_relu(x.float(), b.float()).half()), (shape, offset)


def test_f16_upfirdn2d_is_the_f32_kernel_rounded_once():
    from rewriting_amd import hip
    from rewriting_amd.utils.stylegan2 import op
    gen = torch.Generator().manual_seed(1)
    for major, h, w, minor, up, down, kh, kw, pads in UPFIRDN_CASES:
        x = _rand((major, h, w, minor), torch.float16, gen)
        k = _rand((kh, kw), torch.float16, gen)
        got = hip.upfirdn2d_major_f16(x, k, up, up, down, down, *pads)
        want = hip.upfirdn2d_major(x.float(), k.float(), up, up, down, down, *pads)
        assert got.numel() > 0
        assert _same_bits(got, want.half()), (major, h, w, minor, up, down, kh, kw, pads)
    k4 = torch.tensor([1., 3., 3., 1.])
    k4 = (k4[None, :] * k4[:, None] / 16 * 4).half().to(DEV)
    x = _rand((2, 3, 16, 20), torch.float16, gen)
    for up, pad in ((1, (1, 1)), (2, (2, 1))):                         # Blur, Upsample
        got = op.upfirdn2d(x, k4, up=up, pad=pad)
        assert _same_bits(got, op.upfirdn2d(x.float(), k4.float(), up=up, pad=pad).half()), up


def test_f16_bias_grad_within_a_half_ulp_of_the_float64_sum():
    from rewriting_amd import hip
    gen = torch.Generator().manual_seed(2)
    for shape in [(8, 32, 16, 16), (3, 5, 7), (4, 3), (1, 7, 33, 65), (64, 2, 1, 1)]:
        g = _rand(shape, torch.float16, gen)
        dims = [0] + list(range(2, g.ndim))
        _check_half_sum(hip.bias_grad_f16(g), g, dims)


def test_f64_fused_bias_act_is_the_restatement_bit_for_bit():
    from rewriting_amd import hip
    from oracle import restatement as R
    gen = torch.Generator().manual_seed(3)
    for (shape, offset), (act, grad), with_bias in itertools.product(FBA_CASES, CODES, (False, True)):
        x = _cut(shape, offset, torch.float64, gen)
        ref = _cut(shape, False, torch.float64, gen)
        b = _rand((shape[1],), torch.float64, gen) if with_bias else None
        got = hip.fused_bias_act_f64(x, b, ref, act, grad, 0.2, SQRT2)
        want = R.fused_bias_act(x.cpu(), None if b is None else b.cpu(), ref.cpu(), act, grad, 0.2, SQRT2)
        assert _same_bits(got.cpu(), want), (shape, offset, act, grad, with_bias)


def test_f64_upfirdn2d_matches_the_restatement():
    from rewriting_amd import hip
    from oracle import restatement as R
    gen = torch.Generator().manual_seed(4)
    for major, h, w, minor, up, down, kh, kw, pads in UPFIRDN_CASES:
        x = _rand((major, h, w, minor), torch.float64, gen)
        k = _rand((kh, kw), torch.float64, gen)
        got = hip.upfirdn2d_major_f64(x, k, up, up, down, down, *pads).cpu()
        want = R.upfirdn2d_major(x.cpu(), k.cpu(), up, up, down, down, *pads)
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item(), (major, h, w, minor, up, down)


def test_fused_leaky_relu_adjoints_pass_gradcheck_in_float64():
    from rewriting_amd.utils.stylegan2 import op
    gen = torch.Generator().manual_seed(5)
    for shape in [(2, 3, 4, 5), (3, 4), (2, 8, 2, 2)]:
        b = _rand((shape[1],), torch.float64, gen)
        v = _rand(shape, torch.float64, gen)
        v = torch.where(v >= 0, v + 0.05, v - 0.05)                   # x + b at least 0.05 from the kink
        x = (v - b.view(1, -1, *([1] * (len(shape) - 2)))).requires_grad_(True)
        b.requires_grad_(True)
        assert torch.autograd.gradcheck(op.fused_leaky_relu, (x, b)), shape
        assert torch.autograd.gradgradcheck(op.fused_leaky_relu, (x, b)), shape


def _adjoint_configs():
    """(up, down, (pad0, pad1), kernel): the generator's Blur and Upsample, then seeded draws"""
    k4 = torch.tensor([1., 3., 3., 1.], dtype=torch.float64)
    k4 = k4[None, :] * k4[:, None] / 16 * 4
    out = [(1, 1, (1, 1), k4), (2, 1, (2, 1), k4)]
    rs = numpy.random.RandomState(2024)
    while len(out) < 24:
        up, down = int(rs.randint(1, 4)), int(rs.randint(1, 4))
        kh, kw = int(rs.randint(1, 6)), int(rs.randint(1, 6))
        pad = (int(rs.randint(-1, 4)), int(rs.randint(-1, 4)))
        out.append((up, down, pad, torch.from_numpy(rs.randn(kh, kw))))
    return out


def test_upfirdn2d_adjoints_pass_gradcheck_in_float64():
    from rewriting_amd.utils.stylegan2 import op
    gen = torch.Generator().manual_seed(6)
    checked = 0
    for up, down, pad, k in _adjoint_configs():
        h, w = 5, 6
        if min((h * up + pad[0] + pad[1] - k.shape[0]) // down, (w * up + pad[0] + pad[1] - k.shape[1]) // down) < 0:
            continue
        x = _rand((1, 2, h, w), torch.float64, gen).requires_grad_(True)
        kd = k.to(DEV)

        def f(t):
            return op.upfirdn2d(t, kd, up=up, down=down, pad=pad)
        assert torch.autograd.gradcheck(f, (x,)), (up, down, pad, tuple(k.shape))
        assert torch.autograd.gradgradcheck(f, (x,)), (up, down, pad, tuple(k.shape))
        checked += 1
    assert checked >= 20


def test_half_fused_leaky_relu_module_forward_and_backward():
    from rewriting_amd.utils.stylegan2 import op
    gen = torch.Generator().manual_seed(7)
    c = 16
    m = op.FusedLeakyReLU(c).to(DEV).half()
    with torch.no_grad():
        m.bias.copy_(_rand((c,), torch.float16, gen))
    x = _rand((4, c, 8, 8), torch.float16, gen).requires_grad_(True)
    g = _rand((4, c, 8, 8), torch.float16, gen)
    out = m(x)
    out.backward(g)
    assert out.dtype == x.grad.dtype == m.bias.grad.dtype == torch.float16
    x32 = x.detach().float().requires_grad_(True)
    b32 = m.bias.detach().float().requires_grad_(True)
    out32 = op.fused_leaky_relu(x32, b32)
    out32.backward(g.float())
    assert _same_bits(out.detach(), out32.detach().half())
    assert _same_bits(x.grad, x32.grad.half())
    _check_half_sum(m.bias.grad, x.grad, [0, 2, 3])


def test_other_dtypes_and_mixed_operands_are_refused_and_empty_inputs_stay_empty():
    from rewriting_amd.utils.stylegan2 import op
    x = torch.randn(2, 4, 8, 8, device=DEV)
    k = torch.ones(2, 2, device=DEV) / 4
    with pytest.raises(RuntimeError, match='float16, float32 or float64'):
        op.fused_leaky_relu(x.bfloat16(), torch.zeros(4, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match='float16, float32 or float64'):
        op.upfirdn2d(x.bfloat16(), k.bfloat16())
    with pytest.raises(RuntimeError, match='nothing is converted'):
        op.fused_leaky_relu(x.half(), torch.zeros(4, device=DEV))
    with pytest.raises(RuntimeError, match='nothing is converted'):
        op.upfirdn2d(x.half(), k)
    with pytest.raises(RuntimeError, match='nothing is converted'):
        op.upfirdn2d(x.double(), k.half())
    for dt in (torch.float16, torch.float32, torch.float64):
        e = torch.empty(0, 4, 8, 8, device=DEV, dtype=dt)
        y = op.fused_leaky_relu(e, torch.zeros(4, device=DEV, dtype=dt))
        assert y.dtype == dt and y.shape == e.shape
        y = op.upfirdn2d(e, k.to(dt), up=2, pad=(1, 0))
        assert y.dtype == dt and y.shape == (0, 4, 16, 16)
