"""Float64 NumPy restatement of the device statistics of build.py --device (hipvae.stats; test helper: the product never
imports it)."""
import math
import os

import numpy as np


def order_stats(x, ranks):
    """x [F, H] -> [len(ranks), H]: np.sort(x[:, h])[rank], exact elements of the column (the input's dtype)."""
    s = np.sort(np.asarray(x), axis=0)
    return s[np.asarray(ranks, np.int64)]


def percentile_ranks(F, qs):
    """[(lo, hi, g)] per q: in float64 v = (F - 1) q / 100, lo = floor(v), hi = min(lo + 1, F - 1), g = v - lo."""
    out = []
    for q in qs:
        v = (F - 1) * float(q) / 100.0
        lo = int(math.floor(v))
        out.append((lo, min(lo + 1, F - 1), v - lo))
    return out


def percentiles_sorted(s, qs):
    """Columns already sorted, s [F, H] -> float32 [len(qs), H]: a + (b - a) g in float64 between the bracketing order
    statistics a = s[lo], b = s[hi], rounded once to float32."""
    out = []
    for lo, hi, g in percentile_ranks(len(s), qs):
        a, b = s[lo].astype(np.float64), s[hi].astype(np.float64)
        out.append(a + (b - a) * g)
    return np.stack(out).astype(np.float32)


def percentiles(x, qs):
    """x [F, H] -> float32 [len(qs), H]: `percentiles_sorted` of its sorted columns."""
    return percentiles_sorted(np.sort(np.asarray(x), axis=0), qs)


def utterance_variance(s):
    """Biased per-bin variance of one utterance [N, H], two passes in float64."""
    s = np.asarray(s, np.float64)
    return ((s - s.mean(axis=0)) ** 2).mean(axis=0)


def speaker_stats(sp, f0, lengths, speakers, n_spk):
    """-> (lf0 float64 [n_spk, 3] = count, mean, population std of ln f0 over the speaker's frames with f0 > 2;
    gv float64 [n_spk, H] = mean over the speaker's utterances of >= 2 frames of the utterance variance;
    n_utt int64 [n_spk]).  NaN mean / std where the count is 0, NaN gv where n_utt is 0.  Utterances in offset order."""
    sp, f0 = np.asarray(sp), np.asarray(f0)
    H = sp.shape[1]
    lf0 = np.full((n_spk, 3), np.nan)
    gv = np.full((n_spk, H), np.nan)
    n_utt = np.zeros(n_spk, np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for s in range(n_spk):
        us = [u for u in range(len(lengths)) if speakers[u] == s]
        f = np.concatenate([f0[off[u]:off[u + 1]] for u in us]) if us else np.zeros(0, np.float32)
        lf = np.log(f[f > 2.].astype(np.float64))
        lf0[s, 0] = lf.size
        if lf.size:
            lf0[s, 1], lf0[s, 2] = lf.mean(), lf.std()
        parts = [utterance_variance(sp[off[u]:off[u + 1]]) for u in us if lengths[u] >= 2]
        n_utt[s] = len(parts)
        if parts:
            gv[s] = np.mean(np.stack(parts), axis=0)
    return lf0, gv, n_utt


E2E_PLAN = {'SF1': (0, [40, 2, 65]), 'SM1': (3, [300, 18]), 'TM3': (9, [30, 90, 57])}


def write_e2e_tree(root, seed=5):
    """The end-to-end training set of the build.py tests: 3 speakers x 2-3 .bin files of 2 .. 300 frames, written with
    analyzer.write_bin.  -> (file pattern, {speaker name: [records [N, 1029] per file, in sorted file order]})."""
    import analyzer
    rng = np.random.default_rng(seed)
    utts = {}
    for spk, (sid, lens) in E2E_PLAN.items():
        for u, n in enumerate(lens):
            sp = rng.uniform(-9, -3, 513) + rng.uniform(0.05, 0.8, 513) * rng.standard_normal((n, 513))
            ap = rng.uniform(0, 1, (n, 513))
            f0 = np.where(rng.random(n) > 0.3, rng.uniform(80, 300, n), 0.0)
            en = rng.uniform(1e-3, 1, n)
            path = os.path.join(root, 'bin', 'Training Set', spk, '1000%02d.bin' % u)
            utts.setdefault(spk, []).append(analyzer.write_bin(path, sp, ap, f0, en, sid))
    return os.path.join(root, 'bin', 'Training Set', '*', '*.bin'), utts


def e2e_restatement(utts, n_spk=10):
    """Float64 restatement of every file build.py writes for `utts`: {file name: float64 array}; plus the two bracketing
    order statistics of xmin / xmax under 'xmin.bracket' / 'xmax.bracket' ([2, 513], the input's float32)."""
    names = sorted(utts)
    recs = [r for spk in names for r in utts[spk]]
    allr = np.concatenate(recs)
    sp = allr[:, :513]
    lengths = [len(r) for r in recs]
    speakers = [int(r[0, -1]) for r in recs]
    lf0, gv, n_utt = speaker_stats(sp, allr[:, 1026], lengths, speakers, n_spk)
    out = {}
    for spk in names:
        sid = E2E_PLAN[spk][0]
        out[spk + '.npf'] = lf0[sid, 1:]
        if n_utt[sid] > 0:
            out[spk + '_gv.npf'] = gv[sid]
    s = np.sort(sp, axis=0)
    for name, q in (('xmin', 0.5), ('xmax', 99.5)):
        (lo, hi, g), = percentile_ranks(len(sp), [q])
        out[name + '.bracket'] = np.stack([s[lo], s[hi]])
        out[name + '.npf'] = s[lo].astype(np.float64) + (s[hi].astype(np.float64) - s[lo].astype(np.float64)) * g
    assert not float(g).is_integer()         # the frame count makes both percentiles interpolate
    return out


def ulp32(v):
    """Spacing of float32 at |v| (float64 array); the smallest subnormal where v rounds to 0."""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def within_ulp32(got32, want64, n=1):
    """got32 (float32) within n float32 ulp of the float64 value, NaN matching NaN."""
    got32, want64 = np.asarray(got32), np.asarray(want64, np.float64)
    both_nan = np.isnan(got32) & np.isnan(want64)
    with np.errstate(invalid='ignore'):
        ok = np.abs(got32.astype(np.float64) - want64) <= n * ulp32(want64)
    return bool(np.all(ok | both_nan))
