"""The leaf helpers of the tensor-level wrappers (ops.py, grid_ops.py): the current stream, the device / dtype / layout checks of
operands and outputs, and the pointer that keeps its tensor alive.  They depend on nothing but the binding (_lib.py)."""
import ctypes as C

import torch

from . import _lib


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """The current HIP stream of the current device as a void pointer.  torch.cuda.current_stream() builds a Stream object
    through several Python layers (9 us; a decode mini-batch issues ~40 launches, a training step ~2000): the raw-handle
    accessor behind it is used when this torch build exposes it."""
    if _lib.is_twin():
        return C.c_void_p(0)             # (the CPU twin is synchronous)
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32, name='tensor'):
    if _lib.is_twin():                   # explicit opt-in (cpu_twin.enable()): the g++ twin takes HOST tensors only
        if not isinstance(t, torch.Tensor) or t.is_cuda:
            raise RuntimeError('%s must be a CPU tensor while the CPU twin is loaded' % name)
    elif not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor: occlusions4d_amd runs only on the HIP library '
                           '(no CPU fallback)' % name)
    assert t.dtype == dtype, '%s must be %s, got %s' % (name, dtype, t.dtype)
    return t


def _rows(t, name='tensor'):
    """2-D view whose last dim is contiguous; returns (tensor, row stride in elements)."""
    assert t.dim() == 2, '%s must be 2-D, got %s' % (name, tuple(t.shape))
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


class _TensorPointer(C.c_void_p):
    """A void pointer that owns a reference to the tensor it points into: the memory stays allocated for as long as the pointer
    object lives, so a caller may build an argument list out of _ptr(<temporary tensor>) without the library reading or writing
    freed memory (on the host that is heap corruption; the device's caching allocator merely hides it)."""
    __slots__ = ('tensor',)


def _ptr(t):
    if t is None:
        return C.c_void_p(0)
    ptr = _TensorPointer(t.data_ptr())
    ptr.tensor = t
    return ptr


def _out(out, shape, device, dtype=torch.float32, name='out'):
    """The 2-D output of a launch -> (tensor, row stride in elements): allocated when `out` is None; a caller's `out` is
    adopted as it is -- it must be on the library's device kind, of `dtype`, exactly `shape`, with a contiguous last
    dimension (a copy made behind the caller's back would swallow the result)."""
    if out is None:
        return _rows(torch.empty(shape, dtype=dtype, device=device), name)
    o, ld = _rows(_dev(out, dtype, name), name)
    assert o is out and tuple(o.shape) == tuple(shape), \
        '%s must be a %s tensor with unit column stride, got %s with strides %s' % (name, tuple(shape), tuple(out.shape), out.stride())
    return o, ld


def _sized(query_fn, *args, dtype=torch.float32, device):
    """1-D buffer of the element count a `*_floats` / `*_workspace_*` query of the library returns for `args`; a negative
    count (the query rejected its arguments) raises the library's EINVAL error."""
    n = int(query_fn(*args))
    if n < 0:
        _lib.check(_lib.EINVAL)
    return torch.empty((n,), dtype=dtype, device=device)


def _inst_column(t, n, name, dtype=torch.float32):
    """(tensor, element stride) of an (n,) operand used as it is: a column view of a wider array keeps its stride."""
    t = _dev(t, dtype, name)
    assert tuple(t.shape) == (n,), '%s must be (%d,), got %s' % (name, n, tuple(t.shape))
    if n > 1 and t.stride(0) < 1:
        t = t.contiguous()
    return t, (t.stride(0) if n > 1 else 1)


def _merge_rows(t, name):
    """(tensor, row stride) of a track-merge operand: used IN PLACE (never a copy), so its last dim must be contiguous."""
    t = _dev(t, name=name)
    assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), '%s must be (n, g) with a contiguous last dim' % name
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


def _merge_column(t, n, name):
    if t is None:
        return None
    t = _dev(t, name=name)
    assert tuple(t.shape) == (n,) and t.is_contiguous(), '%s must be a contiguous (%d,) tensor' % (name, n)
    return t


def _int32_out(buf, shape, device, name):
    """A caller's contiguous int32 buffer of at least prod(shape) elements (its first ones are used, viewed as `shape`), or a new one."""
    count = 1
    for s in shape:
        count *= s
    if buf is None:
        return torch.empty(shape, dtype=torch.int32, device=device)
    buf = _dev(buf, torch.int32, name)
    assert buf.dim() == 1 and buf.shape[0] >= count and buf.is_contiguous(), \
        '%s must be a contiguous (>= %d,) tensor, got %s' % (name, count, tuple(buf.shape))
    return buf[:count].view(shape)
