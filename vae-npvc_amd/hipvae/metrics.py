"""Objective evaluation on the device (vaenpvc_mcd_dtw): mel-cepstral distortion in dB between two
utterances along their dynamic-time-warping path, with the log-F0 error and the voicing mismatch on the same path."""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L

H = 513
MAX_FRAMES = 4096           # per utterance and side (VAENPVC_MCD_MAX_FRAMES)
MAX_ORDER = 64
MAX_PAIRS = 65536
DB_FACTOR = 6.1418514637137541
FIELDS = ('mcd_db', 'path_length', 'd_end', 'lf0_rmse', 'n_voiced', 'n_voicing_mismatch', 'cost_sum', 'reserved')
_ws = {}                    # device -> workspace tensor, grown on demand
_W = {}                     # (device, order, alpha) -> W on the device


def mcep_matrix(order=24, alpha=0.42):
    """W [(order + 1), 513] float64 (host, NumPy) with mc = W L for L = 0.5 (ln 10 sp + ln en): vaenpvc_mcep_matrix."""
    order, alpha = int(order), float(alpha)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError('order must be in [1, %d] (got %r)' % (MAX_ORDER, order))
    if not (math.isfinite(alpha) and 0.0 <= alpha < 1.0):
        raise ValueError('alpha must be in [0, 1) (got %r)' % alpha)
    W = np.empty((order + 1, H), np.float64)
    L.check(L.load_library().vaenpvc_mcep_matrix(order, alpha, H, W.ctypes.data_as(C.c_void_p)), 'mcep_matrix')
    return W


def layout(n_pair, Fa, Fb, cells, order):
    """Workspace regions of include/vaenpvc.h: name -> (byte offset, dtype, shape); plus the total under 'bytes'."""
    F = Fa + Fb
    regs = [('mc', torch.float64, (F, order + 1)), ('lf0', torch.float64, (F,)), ('pinfo', torch.int64, (n_pair + 1, 6)),
            ('cost', torch.float64, (cells,)), ('code', torch.uint8, (cells,))]
    out, o = {}, 0
    for name, dt, shape in regs:
        out[name] = (o, dt, shape)
        o += (math.prod(shape) * (1 if dt == torch.uint8 else 8) + 255) // 256 * 256
    out['bytes'] = o
    return out


def region(ws, lay, name):
    """A workspace region as a tensor view (device)."""
    o, dt, shape = lay[name]
    nbytes = math.prod(shape) * (1 if dt == torch.uint8 else 8)
    return ws[o:o + nbytes].view(dt).view(shape)


def diag_index(Ta, Tb):
    """int64 [Ta, Tb]: where cell (i, j) of a pair stands inside the pair's slice of the `cost` and `code` regions and of
    D.  The cells are stored anti-diagonal after anti-diagonal (s = i + j ascending, i ascending inside a diagonal), so
    `flat[diag_index(Ta, Tb)]` is the Ta x Tb matrix."""
    i, j = np.indices((Ta, Tb), dtype=np.int64)
    s = i + j
    m, M, n = min(Ta, Tb), max(Ta, Tb), Ta + Tb - 1
    r = n - s
    pre = np.where(s <= m, s * (s + 1) // 2, np.where(s <= M, m * (m + 1) // 2 + (s - m) * m, Ta * Tb - r * (r + 1) // 2))
    return pre + i - np.maximum(0, s - Tb + 1)


def check_args(lengthsA, lengthsB, order=24, alpha=0.42):
    """Host-side checks of the binding (before any device work): the pairing, the frame counts and the ABI's scalar
    limits.  -> (lengthsA, lengthsB, order, alpha, cells)."""
    lengthsA, lengthsB = [int(n) for n in lengthsA], [int(n) for n in lengthsB]
    if not lengthsA or len(lengthsA) != len(lengthsB):
        raise ValueError('need the same number (>= 1) of utterances on both sides (got %d and %d)'
                         % (len(lengthsA), len(lengthsB)))
    if len(lengthsA) > MAX_PAIRS:
        raise ValueError('at most %d pairs per call (got %d)' % (MAX_PAIRS, len(lengthsA)))
    for n in lengthsA + lengthsB:
        if not 1 <= n <= MAX_FRAMES:
            raise ValueError('every utterance needs 1 .. %d frames (got %d); split longer ones' % (MAX_FRAMES, n))
    order, alpha = int(order), float(alpha)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError('order must be in [1, %d] (got %r)' % (MAX_ORDER, order))
    if not (math.isfinite(alpha) and 0.0 <= alpha < 1.0):
        raise ValueError('alpha must be in [0, 1) (got %r)' % alpha)
    return lengthsA, lengthsB, order, alpha, sum(a * b for a, b in zip(lengthsA, lengthsB))


def _side(name, sp, en, f0, lengths):
    F = sum(lengths)
    for t, shape, what in ((sp, (F, H), 'sp'), (en, (F,), 'en'), (f0, (F,), 'f0')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError('%s%s must be a float32 CUDA tensor' % (what, name))
        if tuple(t.shape) != shape:
            raise ValueError('%s%s has shape %s, the lengths ask for %s' % (what, name, tuple(t.shape), shape))
    return sp.contiguous(), en.contiguous(), f0.contiguous(), F


def mcd_dtw(spA, enA, f0A, lengthsA, spB, enB, f0B, lengthsB, order=24, alpha=0.42, return_path=False,
            return_workspace=False, return_D=False):
    """Pair p = utterance p of side A against utterance p of side B; the utterances of a side are stored back to back
    (sp [F, 513] = log10(sp / en), en [F], f0 [F]; float32 CUDA tensors).  Enqueues on the current stream and returns
    results, a float64 CUDA tensor [n_pair, 8] (FIELDS).  return_path: also a list of int32 CUDA tensors [P, 2] in forward
    order, (0, 0) first (this reads the path lengths back, i.e. synchronises).  return_D: also the accumulated-cost
    matrices as one float64 tensor [cells] (the cost region's layout: `diag_index`).  return_workspace: also the workspace tensor
    (include/vaenpvc.h layout, see `layout`)."""
    lengthsA, lengthsB, order, alpha, cells = check_args(lengthsA, lengthsB, order, alpha)
    spA, enA, f0A, Fa = _side('A', spA, enA, f0A, lengthsA)
    spB, enB, f0B, Fb = _side('B', spB, enB, f0B, lengthsB)
    dev = spA.device
    if spB.device != dev:
        raise ValueError('both sides must live on one device')
    lib = L.load_library()
    n = len(lengthsA)
    key = (dev, order, alpha)
    if key not in _W:
        if len(_W) > 16:
            _W.clear()
        _W[key] = torch.from_numpy(mcep_matrix(order, alpha)).to(dev)
    W = _W[key]
    need = int(lib.vaenpvc_mcd_workspace_bytes(n, Fa, Fb, cells, order))
    if need < 0:
        L.check(need, 'mcd_workspace_bytes')
    ws = _ws.get(dev)
    if ws is None or ws.numel() < need or return_workspace:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if not return_workspace:
            _ws[dev] = ws
    offs = torch.tensor([[0] + lengthsA, [0] + lengthsB], dtype=torch.int64).cumsum(1).to(dev)
    res = torch.empty(n, 8, dtype=torch.float64, device=dev)
    path = torch.empty(Fa + Fb, 2, dtype=torch.int32, device=dev) if return_path else None
    D = torch.empty(cells, dtype=torch.float64, device=dev) if return_D else None
    with torch.cuda.device(dev):
        L.check(lib.vaenpvc_mcd_dtw(spA.data_ptr(), enA.data_ptr(), f0A.data_ptr(), offs[0].data_ptr(), Fa,
                                    spB.data_ptr(), enB.data_ptr(), f0B.data_ptr(), offs[1].data_ptr(), Fb, n, cells,
                                    W.data_ptr(), order, res.data_ptr(), path.data_ptr() if return_path else None,
                                    D.data_ptr() if return_D else None, ws.data_ptr(), need,
                                    torch.cuda.current_stream(dev).cuda_stream), 'mcd_dtw')
    out = (res,)
    if return_path:
        P = res[:, 1].cpu().numpy().astype(np.int64)
        start = np.cumsum([0] + lengthsA)[:-1] + np.cumsum([0] + lengthsB)[:-1]
        out += ([path[int(s):int(s) + int(k)].flip(0) for s, k in zip(start, P)],)
    if return_D:
        out += (D,)
    if return_workspace:
        out += (ws,)
    return out[0] if len(out) == 1 else out
