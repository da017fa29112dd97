"""Band-limited resampling on the device (vaenpvc_resample): what the reference's
librosa.load(filename, sr=16000) does to a wav of another rate (analyzer.py:40), without librosa."""
import ctypes as C

import numpy as np
import torch

from . import lib as L

_plans = {}                 # (rate_in, rate_out) -> (L, M, K)
_tables = {}                # (rate_in, rate_out) -> float64 NumPy [2K, L]
_dev_tables = {}            # (rate_in, rate_out, device) -> its device copy


def plan(rate_in, rate_out):
    """(L, M, K) of include/vaenpvc.h: L = rate_out / gcd, M = rate_in / gcd, K = ceil(64 / min(1, L / M)).  ValueError
    for a rate pair outside the library's limits."""
    key = (int(rate_in), int(rate_out))
    if key not in _plans:
        if not all(-2 ** 31 <= r < 2 ** 31 for r in key):
            raise ValueError('cannot resample %d -> %d Hz' % key)
        lib = L.load_library()
        up, down, half = C.c_int32(), C.c_int32(), C.c_int32()
        if lib.vaenpvc_resample_plan(key[0], key[1], C.byref(up), C.byref(down), C.byref(half)) != 0:
            raise ValueError(lib.vaenpvc_last_error().decode())
        _plans[key] = (up.value, down.value, half.value)
    return _plans[key]


def out_length(n, up, down):
    """Output samples of a segment of n input samples: (n L + M - 1) // M, librosa's ceil(n * ratio)."""
    return (int(n) * int(up) + int(down) - 1) // int(down)


def filter_table(rate_in, rate_out):
    """The weights T [2K, L] (float64 NumPy, read-only) from vaenpvc_resample_filter, cached per rate pair."""
    key = (int(rate_in), int(rate_out))
    if key not in _tables:
        up, down, half = plan(*key)
        t = np.empty((2 * half, up), np.float64)
        L.check(L.load_library().vaenpvc_resample_filter(key[0], key[1], t.ctypes.data), 'resample_filter')
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


def _device_table(rate_in, rate_out, dev):
    key = (int(rate_in), int(rate_out), dev)
    if key not in _dev_tables:
        _dev_tables[key] = torch.from_numpy(filter_table(rate_in, rate_out).copy()).to(dev)
    return _dev_tables[key]


def check_args(lengths, rate_in, rate_out):
    """Host-side checks of the binding (before any device work): sample counts and the rate pair.
    -> (lengths, (L, M, K))"""
    lengths = [int(n) for n in lengths]
    if not lengths or min(lengths) < 1:
        raise ValueError('lengths must be a non-empty list of sample counts >= 1 (got %s)' % (lengths,))
    return lengths, plan(rate_in, rate_out)


def resample(x, lengths, rate_in, rate_out=16000):
    """Segments of `lengths` samples at rate_in stored back to back in x (float32 CUDA [S_in]) -> (y, out_lengths): the
    segments at rate_out back to back (float32 CUDA [S_out], enqueued on the current stream) and their sample counts.
    A segment's outputs depend on its own samples only."""
    lengths, (up, down, half) = check_args(lengths, rate_in, rate_out)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 1:
        raise TypeError('x must be a 1-D float32 CUDA tensor')
    S_in = sum(lengths)
    if x.numel() != S_in:
        raise ValueError('x holds %d samples, lengths add up to %d' % (x.numel(), S_in))
    outs = [out_length(n, up, down) for n in lengths]
    S_out = sum(outs)
    dev = x.device
    lib = L.load_library()
    x = x.contiguous()
    table = _device_table(rate_in, rate_out, dev)
    offs = torch.tensor([[0] + lengths, [0] + outs], dtype=torch.int64).cumsum(1).to(dev)
    y = torch.empty(S_out, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.vaenpvc_resample(x.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), len(lengths), S_in, S_out,
                                     int(rate_in), int(rate_out), table.data_ptr(), y.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), 'resample')
    return y, outs
