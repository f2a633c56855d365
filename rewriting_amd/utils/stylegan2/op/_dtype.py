"""Which wrapper of ``rewriting_amd.hip`` an op calls for its input's dtype.

The reference's two modules dispatch float, double and half (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
utils/stylegan2/op/fused_bias_act_kernel.cu:79, upfirdn2d_kernel.cu:225); so do these: fp32
calls the plain wrapper (``hip.fused_bias_act``), half and double its ``_f16`` / ``_f64`` form.
"""
import torch

from .... import hip

_SUFFIX = {torch.float32: '', torch.float16: '_f16', torch.float64: '_f64'}


def wrapper(name, input, **operands):
    """``hip.<name>`` for ``input``'s dtype.  Raises RuntimeError, before anything is launched, for
    a dtype other than float16 / float32 / float64 and for an operand (``bias=``, ``refer=``,
    ``kernel=``; None = absent) whose dtype is not the input's: nothing is converted."""
    if input.dtype not in _SUFFIX:
        raise RuntimeError('rewriting_amd: %s takes float16, float32 or float64 tensors; the input is %s'
                           % (name, input.dtype))
    for what, t in operands.items():
        if t is not None and t.dtype != input.dtype:
            raise RuntimeError('rewriting_amd: %s: the %s is %s and the input %s; pass both in one dtype '
                               '(nothing is converted)' % (name, what, t.dtype, input.dtype))
    return getattr(hip, name + _SUFFIX[input.dtype])
