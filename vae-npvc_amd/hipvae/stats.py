"""Training-set statistics on the device (vaenpvc_column_select, vaenpvc_speaker_stats): exact
per-column order statistics, the percentiles built from them, and the per-speaker log-F0 / global-variance statistics
that `build.py --device` writes.  No context: the functions take CUDA tensors and enqueue on the current stream."""
import ctypes as C
import math

import torch

from . import lib as L

MAX_RANKS = 8               # VAENPVC_SELECT_MAX_RANKS
_ws = {}                    # device -> workspace tensor, grown on demand


def _workspace(dev, need):
    ws = _ws.get(dev)
    if ws is None or ws.numel() < need:
        ws = _ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def _rows(t, what):
    """A float32 CUDA matrix whose rows are contiguous -> (F, H, row stride in floats)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError('%s must be a float32 CUDA tensor' % what)
    if t.dim() != 2:
        raise ValueError('%s must be 2-D (got shape %s)' % (what, tuple(t.shape)))
    F, H = t.shape
    if H < 1:
        raise ValueError('%s needs at least one column' % what)
    if H > 1 and t.stride(1) != 1:
        raise ValueError('%s: the columns of a row must be contiguous (stride %d)' % (what, t.stride(1)))
    ld = t.stride(0) if F > 1 else H
    if ld < H:
        raise ValueError('%s: row stride %d is shorter than a row of %d' % (what, ld, H))
    return F, H, ld


def column_select(x, ranks):
    """x [F, H] float32 CUDA tensor (a strided view with contiguous rows will do, e.g. records[:, :513]); ranks: 1 .. 8
    zero-based ranks in [0, F).  -> float32 [n_rank, H] with out[r, h] = sort(x[:, h])[ranks[r]], exact elements of the
    column.  Raises ValueError when x holds a NaN or an Inf (reads the device flag back, i.e. synchronises)."""
    F, H, ld = _rows(x, 'x')
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= MAX_RANKS:
        raise ValueError('need 1 .. %d ranks (got %d)' % (MAX_RANKS, len(ranks)))
    if F < 1:
        raise ValueError('an empty column has no order statistic')
    for r in ranks:
        if not 0 <= r < F:
            raise ValueError('rank %d outside [0, %d)' % (r, F))
    lib, dev = L.load_library(), x.device
    need = int(lib.vaenpvc_column_select_workspace_bytes(F, H, len(ranks)))
    if need < 0:
        L.check(need, 'column_select_workspace_bytes')
    ws = _workspace(dev, need)
    out = torch.empty(len(ranks), H, dtype=torch.float32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    host_ranks = (C.c_int64 * len(ranks))(*ranks)
    with torch.cuda.device(dev):
        L.check(lib.vaenpvc_column_select(x.data_ptr(), F, H, ld, C.cast(host_ranks, C.c_void_p), len(ranks),
                                          out.data_ptr(), flag.data_ptr(), ws.data_ptr(), need,
                                          torch.cuda.current_stream(dev).cuda_stream), 'column_select')
    if int(flag.item()) & 1:
        raise ValueError('column_select: the non-finite flag is set (x holds a NaN or an Inf)')
    return out


def percentile_ranks(F, qs):
    """[(lo, hi, g)] per q: in float64 v = (F - 1) q / 100, lo = floor(v), hi = min(lo + 1, F - 1), g = v - lo."""
    out = []
    for q in qs:
        q = float(q)
        if not 0.0 <= q <= 100.0:
            raise ValueError('percentile %r outside [0, 100]' % q)
        v = (F - 1) * q / 100.0
        lo = int(math.floor(v))
        out.append((lo, min(lo + 1, F - 1), v - lo))
    return out


def percentiles(x, qs):
    """Per-column percentiles of x [F, H] -> float32 [len(qs), H]: a + (b - a) g in float64, rounded once to float32,
    a / b the order statistics of ranks lo / hi (`percentile_ranks`), all fetched by one column_select call."""
    qs = list(qs)
    if not 1 <= 2 * len(qs) <= MAX_RANKS:
        raise ValueError('need 1 .. %d percentiles (got %d)' % (MAX_RANKS // 2, len(qs)))
    F = x.shape[0] if isinstance(x, torch.Tensor) and x.dim() == 2 else 0
    if F < 1:
        raise ValueError('an empty column has no percentile')
    pr = percentile_ranks(F, qs)
    v = column_select(x, [r for lo, hi, _ in pr for r in (lo, hi)]).double()
    g = torch.tensor([g for _, _, g in pr], dtype=torch.float64, device=x.device).unsqueeze(1)
    a, b = v[0::2], v[1::2]
    return (a + (b - a) * g).float()


def speaker_stats(sp, f0, lengths, speakers, n_spk):
    """sp [F, H] and f0 [F] float32 CUDA tensors (strided views will do) holding utterances of `lengths` frames back to
    back, `speakers[u]` in [0, n_spk) the speaker of utterance u.  -> (lf0 float64 [n_spk, 3] = count, mean, population
    std of ln f0 over f0 > 2; gv float64 [n_spk, H] = the mean utterance variance over the utterances of >= 2 frames;
    n_utt int64 [n_spk] = their number).  mean / std are NaN where the count is 0, gv where n_utt is 0."""
    F, H, ld = _rows(sp, 'sp')
    if not isinstance(f0, torch.Tensor) or f0.dtype != torch.float32 or not f0.is_cuda or f0.device != sp.device:
        raise TypeError('f0 must be a float32 CUDA tensor on the device of sp')
    if tuple(f0.shape) != (F,):
        raise ValueError('f0 has shape %s, sp asks for %s' % (tuple(f0.shape), (F,)))
    ld_f0 = f0.stride(0) if F > 1 else 1
    if ld_f0 < 1:
        raise ValueError('f0: element stride %d' % ld_f0)
    lengths, speakers, n_spk = [int(n) for n in lengths], [int(s) for s in speakers], int(n_spk)
    if not lengths or len(lengths) != len(speakers):
        raise ValueError('need one speaker per utterance and at least one utterance (got %d lengths, %d speakers)'
                         % (len(lengths), len(speakers)))
    if min(lengths) < 0 or sum(lengths) != F:
        raise ValueError('the lengths must be >= 0 and add up to the %d frames of sp (sum %d)' % (F, sum(lengths)))
    if n_spk < 1:
        raise ValueError('n_spk must be >= 1 (got %d)' % n_spk)
    for s in speakers:
        if not 0 <= s < n_spk:
            raise ValueError('speaker id %d outside [0, %d)' % (s, n_spk))
    lib, dev, n_seg = L.load_library(), sp.device, len(lengths)
    need = int(lib.vaenpvc_speaker_stats_workspace_bytes(F, n_seg, H))
    if need < 0:
        L.check(need, 'speaker_stats_workspace_bytes')
    ws = _workspace(dev, need)
    off = torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0).to(dev)
    spk = torch.tensor(speakers, dtype=torch.int32).to(dev)
    lf0 = torch.empty(n_spk, 3, dtype=torch.float64, device=dev)
    gv = torch.empty(n_spk, H, dtype=torch.float64, device=dev)
    n_utt = torch.empty(n_spk, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.vaenpvc_speaker_stats(sp.data_ptr(), ld, f0.data_ptr(), ld_f0, off.data_ptr(), spk.data_ptr(), n_seg,
                                          n_spk, F, H, lf0.data_ptr(), gv.data_ptr(), n_utt.data_ptr(), ws.data_ptr(),
                                          need, torch.cuda.current_stream(dev).cuda_stream), 'speaker_stats')
    return lf0, gv, n_utt
