"""Model-free WORLD-style feature analysis on the device (vaenpvc_analyze): the reference's
analyzer.py:25-47 (pyworld dio -> stonemask -> cheaptrick -> d4c and the record form) without pyworld."""
import math

import torch

from . import lib as L

FS = 16000
H = 513
TAPS = 1281                 # taps per band in the workspace (include/vaenpvc.h)
_ws = {}                    # device -> workspace tensor, grown on demand


def n_frames(S, fs=FS, frame_period=5.0):
    """T = (int)(1000 S / fs / frame_period) + 1 (GetSamplesForDIO), float64 on the host."""
    return int(1000.0 * S / fs / frame_period) + 1


def n_bands(f0_floor, f0_ceil):
    return 1 + int(math.log(f0_ceil / f0_floor) / math.log(2.0) * 2.0)


def layout(n_seg, S, F, nb):
    """Workspace regions of include/vaenpvc.h: name -> (byte offset, dtype, shape); plus the total under 'bytes'."""
    NBS, NES = S + n_seg, S // 2 + 2 * n_seg
    regs = [('mean', torch.float64, (n_seg,)), ('taps', torch.float64, (nb, TAPS)), ('band', torch.float64, (nb, NBS)),
            ('edges', torch.float64, (nb, 4, NES)), ('ecnt', torch.int32, (nb, 4, n_seg)),
            ('cand', torch.float64, (nb, F)), ('score', torch.float64, (nb, F))]
    regs += [(n, torch.float64, (F,)) for n in ('best', 's1', 's2', 'f0d', 'f0r', 'ap0', 'coarse')]
    regs += [('flags', torch.int32, (F,))]
    out, o = {}, 0
    for name, dt, shape in regs:
        out[name] = (o, dt, shape)
        o += (math.prod(shape) * (8 if dt == torch.float64 else 4) + 255) // 256 * 256
    out['bytes'] = o
    return out


def check_args(lengths, fs, frame_period, f0_floor, f0_ceil):
    """Host-side checks of the binding (before any device work): sample counts and the ABI's scalar limits."""
    lengths = [int(n) for n in lengths]
    if not lengths or min(lengths) < 1:
        raise ValueError('lengths must be a non-empty list of sample counts >= 1 (got %s)' % (lengths,))
    if int(fs) != FS:
        raise ValueError('only fs = 16000 is supported (got %r); resample first' % (fs,))
    frame_period = float(frame_period)
    if not (math.isfinite(frame_period) and 1.0 <= frame_period <= 50.0):
        raise ValueError('frame_period must be in [1, 50] ms (got %r)' % frame_period)
    f0_floor, f0_ceil = float(f0_floor), float(f0_ceil)
    if not (71.0 <= f0_floor < f0_ceil <= 800.0):
        raise ValueError('need 71 <= f0_floor < f0_ceil <= 800 (got %r, %r)' % (f0_floor, f0_ceil))
    return lengths, frame_period, f0_floor, f0_ceil


def analyze(x, lengths, fs=FS, frame_period=5.0, f0_floor=71.0, f0_ceil=500.0, return_workspace=False):
    """Utterances of `lengths` samples stored back to back in x (float32 CUDA [S], librosa's int16 / 32768 scale) ->
    (f0 [F], sp [F, 513] log10(sp / en), ap [F, 513], en [F], frames): float32 CUDA tensors enqueued on the current
    stream and the per-utterance frame counts.  With return_workspace=True the workspace tensor (include/vaenpvc.h
    layout, see `layout`) is appended."""
    lengths, frame_period, f0_floor, f0_ceil = check_args(lengths, fs, frame_period, f0_floor, f0_ceil)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 1:
        raise TypeError('x must be a 1-D float32 CUDA tensor')
    S = sum(lengths)
    if x.numel() != S:
        raise ValueError('x holds %d samples, lengths add up to %d' % (x.numel(), S))
    frames = [n_frames(n, fs, frame_period) for n in lengths]
    F = sum(frames)
    dev = x.device
    lib = L.load_library()
    n = len(lengths)
    need = int(lib.vaenpvc_analysis_workspace_bytes(n, S, F, fs, frame_period, f0_floor, f0_ceil))
    if need < 0:
        L.check(need, 'analysis_workspace_bytes')
    ws = _ws.get(dev)
    if ws is None or ws.numel() < need or return_workspace:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if not return_workspace:
            _ws[dev] = ws
    x = x.contiguous()
    offs = torch.tensor([[0] + lengths, [0] + frames], dtype=torch.int64).cumsum(1).to(dev)
    f0 = torch.empty(F, dtype=torch.float32, device=dev)
    en = torch.empty(F, dtype=torch.float32, device=dev)
    sp = torch.empty(F, H, dtype=torch.float32, device=dev)
    ap = torch.empty(F, H, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.vaenpvc_analyze(x.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), n, S, F, fs, frame_period,
                                    f0_floor, f0_ceil, f0.data_ptr(), sp.data_ptr(), ap.data_ptr(), en.data_ptr(),
                                    ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream), 'analyze')
    out = (f0, sp, ap, en, frames)
    return out + (ws,) if return_workspace else out


def region(ws, lay, name):
    """A workspace region as a tensor view (device)."""
    o, dt, shape = lay[name]
    nbytes = math.prod(shape) * (8 if dt == torch.float64 else 4)
    return ws[o:o + nbytes].view(dt).view(shape)
