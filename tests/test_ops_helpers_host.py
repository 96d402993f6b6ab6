"""The argument plumbing every wrapper of occlusions4d_amd.ops goes through (_out, _sized, _divisor, the shared body of
compact_rows / compact_rows_nosync), on the g++ twin with at most a few hundred rows.  No GPU."""
import math

import pytest
import torch

import occlusions4d_amd as pk

ops = pk.ops


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_divisor_is_the_fp32_rounding_of_sqrt_d():
    """What the wrappers computed per launch before: float(torch.tensor(math.sqrt(d), dtype=torch.float32)), bit for bit."""
    for d in range(1, 2049):
        want = float(torch.tensor(math.sqrt(d), dtype=torch.float32))
        got = ops._divisor(d)
        assert type(got) is float and got == want, (d, got, want)


def test_out_allocates(twin):
    for shape in ((5, 36), (1, 36), (0, 36)):
        o, ld = ops._out(None, shape, torch.device('cpu'))
        assert tuple(o.shape) == shape and o.dtype == torch.float32 and ld == 36 and o.stride(1) == 1
    o, ld = ops._out(None, (3, 7), torch.device('cpu'), dtype=torch.int32)
    assert o.dtype == torch.int32 and ld == 7


def test_out_adopts_a_row_strided_destination(twin):
    buf = torch.zeros(6, 40)
    view = buf[:, 4:40]                                      # (6, 36), row stride 40
    o, ld = ops._out(view, (6, 36), torch.device('cpu'))
    assert o is view and ld == 40
    full, ld = ops._out(buf, (6, 40), torch.device('cpu'))
    assert full is buf and ld == 40
    # ... and a wrapper writes through it: the columns outside the view stay untouched
    src = torch.arange(6 * 36, dtype=torch.float32).view(6, 36)
    assert ops.copy_rows(src, out=view) is view
    assert torch.equal(buf[:, 4:], src) and not buf[:, :4].any()


def test_out_rejects_what_it_cannot_adopt(twin):
    dev = torch.device('cpu')
    with pytest.raises(AssertionError):
        ops._out(torch.zeros(6, 35), (6, 36), dev)           # wrong shape
    with pytest.raises(AssertionError):
        ops._out(torch.zeros(7, 36), (6, 36), dev)
    with pytest.raises(AssertionError):
        ops._out(torch.zeros(6 * 36), (6, 36), dev)          # not 2-D
    with pytest.raises(AssertionError, match='must be torch.float32'):
        ops._out(torch.zeros(6, 36, dtype=torch.float64), (6, 36), dev)
    with pytest.raises(AssertionError, match='must be torch.int32'):
        ops._out(torch.zeros(6, 36), (6, 36), dev, dtype=torch.int32)
    with pytest.raises(AssertionError):
        ops._out(torch.zeros(36, 6).t(), (6, 36), dev)       # column-strided: _rows would have to copy
    with pytest.raises(AssertionError):
        ops._out(torch.zeros(6, 72)[:, ::2], (6, 36), dev)
    with pytest.raises(RuntimeError, match='must be a CPU tensor'):
        ops._out([[0.0] * 36] * 6, (6, 36), dev)             # not a tensor at all
    # the same rejections reach the caller of a wrapper
    src = torch.zeros(6, 36)
    for bad in (torch.zeros(6, 35), torch.zeros(6, 36, dtype=torch.float64), torch.zeros(36, 6).t()):
        with pytest.raises(AssertionError):
            ops.copy_rows(src, out=bad)
        with pytest.raises(AssertionError):
            ops.layernorm(src, None, None, out=bad)


def test_out_rejects_the_wrong_device_kind():
    """Without the twin the library takes CUDA tensors only: a host `out` is refused before anything is launched."""
    assert not pk._lib.is_twin()
    with pytest.raises(RuntimeError, match='out must be a CUDA tensor'):
        ops._out(torch.zeros(6, 36), (6, 36), torch.device('cpu'))
    with pytest.raises(RuntimeError, match='penult must be a CUDA tensor'):
        ops._out(torch.zeros(6, 36), (6, 36), torch.device('cpu'), name='penult')


def test_sized_allocates_what_the_query_returns(twin):
    seen = []

    def query(*args):
        seen.append(args)
        return 12

    buf = ops._sized(query, 3, 'x', device=torch.device('cpu'))
    assert tuple(buf.shape) == (12,) and buf.dtype == torch.float32 and seen == [(3, 'x')]
    assert ops._sized(query, dtype=torch.float64, device=torch.device('cpu')).dtype == torch.float64
    assert ops._sized(lambda: 0, device=torch.device('cpu')).numel() == 0


def test_sized_raises_the_library_error_on_a_negative_size(twin):
    with pytest.raises(AssertionError) as e:
        ops._sized(lambda *a: -1, 1, 2, device=torch.device('cpu'))
    with pytest.raises(AssertionError) as ref:
        pk._lib.check(pk._lib.EINVAL)
    assert str(e.value) == str(ref.value)


def _keys(n, mode):
    g = torch.Generator().manual_seed(n + 1)
    if mode == 'all':
        return torch.full((n,), 2.0)
    if mode == 'none':
        return torch.full((n,), -2.0)
    key = torch.rand(n, generator=g)
    key[::3] = 0.5                                           # ties with the threshold: strict decides
    return key


@pytest.mark.parametrize('strict', [True, False])
@pytest.mark.parametrize('mode', ['mixed', 'all', 'none'])
@pytest.mark.parametrize('n', [0, 1, 300])
def test_compact_rows_and_nosync_agree(twin, n, mode, strict):
    rows = torch.arange(n * 5, dtype=torch.float32).view(n, 5)
    key = _keys(n, mode)
    keep = (key > 0.5) if strict else (key >= 0.5)
    kept_rows, kept_key = ops.compact_rows(rows, key, 0.5, strict=strict)
    buf, count = ops.compact_rows_nosync(rows, key, 0.5, strict=strict)
    assert count.dtype == torch.int32 and tuple(count.shape) == (1,)
    c = int(count[0])
    assert c == int(keep.sum()) == kept_rows.shape[0] == kept_key.shape[0]
    assert tuple(buf.shape) == (n, 5) and tuple(kept_rows.shape) == (c, 5)
    assert torch.equal(kept_rows, rows[keep]) and torch.equal(kept_key, key[keep])
    assert torch.equal(buf[:c], kept_rows)


def test_compact_rows_reads_strided_rows_and_keys(twin):
    wide = torch.arange(64 * 8, dtype=torch.float32).view(64, 8)
    rows, key = wide[:, :3], wide[:, 7].remainder(5)         # row stride 8
    keyed = torch.stack([key, key], dim=1)[:, 0]             # key stride 2
    kept_rows, kept_key = ops.compact_rows(rows, keyed, 1.5)
    buf, count = ops.compact_rows_nosync(rows, keyed, 1.5)
    keep = key > 1.5
    assert torch.equal(kept_rows, rows[keep]) and torch.equal(kept_key, key[keep])
    assert int(count[0]) == int(keep.sum()) and torch.equal(buf[:int(count[0])], kept_rows)
