"""Float64 NumPy restatement of the device WORLD-style analysis (vaenpvc_analyze, csrc/gfx950_analysis.hip), test helper:
the product never imports it.  It states DESIGN.md section 15 step by step: DIO (f0 candidates from four event-interval
series per band, FixF0Contour), StoneMask, CheapTrick and D4C with pyworld's defaults as the reference's analyzer.py calls
them.  Sample-level equality with pyworld is not claimed (no WORLD source or pyworld exists anywhere this project runs).
NumPy only: no scipy."""
import math

import numpy as np

FS = 16000
N_CT = 1024                  # CheapTrick FFT size (513 bins)
H = N_CT // 2 + 1
N_D4C = 2048                 # D4C / LoveTrain FFT size at 16 kHz
EPS = 2.220446049250313e-16  # world::kEps: the deterministic floor that replaces WORLD's |randn| * kEps
SAFE = 1e-12                 # world::kMySafeGuardMinimum
MAXV = 100000.0              # world::kMaximumValue (the score of a rejected candidate)
CH_OCT = 2.0                 # DIO channels per octave
ALLOWED = 0.1                # DIO allowed_range
THRESHOLD = 0.85             # D4C threshold
Q1 = -0.15                   # CheapTrick q1
AP_UNVOICED = 1.0 - SAFE


def mround(v):
    """matlab_round: half away from zero, truncated to int."""
    return int(v + 0.5) if v > 0 else int(v - 0.5)


def n_frames(S, fs=FS, frame_period=5.0):
    """T = (int)(1000 S / fs / frame_period) + 1 (GetSamplesForDIO)."""
    return int(1000.0 * S / fs / frame_period) + 1


def n_bands(f0_floor, f0_ceil):
    return 1 + int(math.log(f0_ceil / f0_floor) / math.log(2.0) * CH_OCT)


def boundaries(f0_floor, f0_ceil):
    return [f0_floor * 2.0 ** ((b + 1) / CH_OCT) for b in range(n_bands(f0_floor, f0_ceil))]


def stonemask_fft_size(f0, fs=FS):
    h = int(1.5 * fs / f0 + 1.0)
    return int(2.0 ** (2 + int(math.log(h * 2.0 + 1.0) / math.log(2.0))))


# ---------------------------------------------------------------------------------------------------------------- DIO
def lowcut_taps(fs=FS):
    """Zero-phase low cut (50 Hz), taps at offsets -C..C: -hann / sum + delta."""
    C = mround(fs / 50.0)
    N = 2 * C + 1
    i = np.arange(1, N + 1)
    h = 0.5 - 0.5 * np.cos(i * 2.0 * np.pi / (N + 1))
    lc = -h / h.sum()
    lc[C] += 1.0
    return lc


def bandpass_taps(boundary_f0, fs=FS):
    """Nuttall window of 2L+1 taps, L = round(2 fs / boundary), modulated by cos(2 pi boundary m / fs)."""
    L = mround(fs / boundary_f0 * 2.0)
    n = 2 * L + 1
    t = np.arange(n) / (n - 1.0)
    w = 0.355768 - 0.487396 * np.cos(2 * np.pi * t) + 0.144232 * np.cos(4 * np.pi * t) - 0.012604 * np.cos(6 * np.pi * t)
    m = np.arange(-L, L + 1)
    return w * np.cos(2 * np.pi * boundary_f0 * m / fs)


def band_taps(boundary_f0, fs=FS):
    """The combined symmetric filter lowcut * bandpass, offsets -(C+L)..(C+L)."""
    return np.convolve(lowcut_taps(fs), bandpass_taps(boundary_f0, fs))


def band_signals(x, f0_floor=71.0, f0_ceil=500.0, fs=FS):
    """[nb, S+1]: y = [x, 0] minus its mean (DIO's y_length = S + 1), then band b = sum_q h_b[q] y[i + 1 + q]
    (the linear convolution WORLD computes with one FFT, delay-compensated by filter_length_half + 1)."""
    x = np.asarray(x, np.float64)
    y = np.concatenate([x, [0.0]])
    y = y - y.sum() / len(y)
    out = []
    for bf in boundaries(f0_floor, f0_ceil):
        h = band_taps(bf, fs)
        K = (len(h) - 1) // 2
        full = np.convolve(y, h)                 # full[n] = sum_j y[j] h[n - j]; symmetric h
        out.append(full[K + 1:K + 1 + len(y)])
    return np.array(out)


def fine_edges(s):
    """ZeroCrossingEngine's fine edges: e - s[e-1] / (s[e] - s[e-1]) at every e with s[e-1] > 0 >= s[e]."""
    s = np.asarray(s, np.float64)
    e = np.nonzero((s[:-1] > 0.0) & (s[1:] <= 0.0))[0] + 1
    return e - s[e - 1] / (s[e] - s[e - 1])


def events(band):
    """The four fine-edge series of one band: negative-going, positive-going, peaks, dips."""
    band = np.asarray(band, np.float64)
    d = band[1:] - band[:-1]                    # -(g[i] - g[i+1]) with g = -band: peaks are where d goes + -> -
    return [fine_edges(band), fine_edges(-band), fine_edges(d), fine_edges(-d)]


def interp_series(edges, t, fs=FS):
    """WORLD's interp1 (histc + linear, extrapolating with the end segments) of the interval series
    (fs / (e[i+1] - e[i]) at (e[i] + e[i+1]) / 2 / fs) at the times t."""
    e = np.asarray(edges, np.float64)
    loc = (e[:-1] + e[1:]) / 2.0 / fs
    val = fs / (e[1:] - e[:-1])
    n = len(loc)
    k = np.clip(np.searchsorted(loc, t, side='right'), 1, n - 1)
    s = (t - loc[k - 1]) / (loc[k] - loc[k - 1])
    return val[k - 1] + s * (val[k] - val[k - 1])


def band_candidates(ev, boundary_f0, t, f0_floor, f0_ceil, fs=FS):
    """(candidate, score / (candidate + 1e-12)) of one band at the frame times t."""
    if min(len(e) for e in ev) - 1 < 3:        # CheckEvent(number - 2) on each of the four interval counts
        return np.zeros(len(t)), np.full(len(t), MAXV / SAFE)
    v = [interp_series(e, t, fs) for e in ev]
    c = (v[0] + v[1] + v[2] + v[3]) / 4.0
    sc = np.sqrt(((v[0] - c) * (v[0] - c) + (v[1] - c) * (v[1] - c) + (v[2] - c) * (v[2] - c) +
                  (v[3] - c) * (v[3] - c)) / 3.0)
    bad = (c > boundary_f0) | (c < boundary_f0 / 2.0) | (c > f0_ceil) | (c < f0_floor)
    c = np.where(bad, 0.0, c)
    sc = np.where(bad, MAXV, sc)
    return c, sc / (c + SAFE)


def best_contour(cands, scores):
    """Per frame the candidate of the first band with the strictly smallest score."""
    best = cands[0].copy()
    tmp = scores[0].copy()
    for b in range(1, len(cands)):
        take = tmp > scores[b]
        tmp = np.where(take, scores[b], tmp)
        best = np.where(take, cands[b], best)
    return best


def _select(cur, past, cands, j):
    ref = (cur * 3.0 - past) / 2.0
    err = abs(ref - cands[0][j])
    best = cands[0][j]
    for b in range(1, len(cands)):
        e = abs(ref - cands[b][j])
        if e < err:
            err, best = e, cands[b][j]
    if abs(1.0 - best / ref) > ALLOWED:
        return 0.0
    return best


def fix_contour(best, cands, f0_floor, frame_period=5.0):
    """FixF0Contour's four steps; an utterance of T <= voice_range_minimum frames is all zero (pyworld's zeros)."""
    T = len(best)
    vrm = int(0.5 + 1000.0 / frame_period / f0_floor) * 2 + 1
    if T <= vrm:
        return np.zeros(T)
    base = np.zeros(T)
    base[vrm:T - vrm] = best[vrm:T - vrm]
    s1 = np.zeros(T)
    for i in range(vrm, T):
        s1[i] = base[i] if abs((base[i] - base[i - 1]) / (SAFE + base[i])) < ALLOWED else 0.0
    s2 = s1.copy()
    c = (vrm - 1) // 2
    for i in range(c, T - c):
        if np.any(s1[i - c:i + c + 1] == 0):
            s2[i] = 0.0
    neg, pos = [], []
    for i in range(1, T):
        if s2[i] == 0 and s2[i - 1] != 0:
            neg.append(i - 1)
        elif s2[i - 1] == 0 and s2[i] != 0:
            pos.append(i)
    s3 = s2.copy()
    for k in range(len(neg)):
        limit = T - 1 if k == len(neg) - 1 else neg[k + 1]
        for j in range(neg[k], limit):
            s3[j + 1] = _select(s3[j], s3[j - 1], cands, j + 1)
            if s3[j + 1] == 0:
                break
    s4 = s3.copy()
    for k in range(len(pos) - 1, -1, -1):
        limit = 1 if k == 0 else pos[k - 1]
        for j in range(pos[k], limit, -1):
            s4[j - 1] = _select(s4[j], s4[j + 1], cands, j - 1)
            if s4[j - 1] == 0:
                break
    return s4


def dio(x, f0_floor=71.0, f0_ceil=500.0, fs=FS, frame_period=5.0, bands=None):
    """-> dict of the DIO stages.  `bands` replaces the band signals (the GPU tests pass the device's own)."""
    S = len(x)
    T = n_frames(S, fs, frame_period)
    t = np.arange(T) * frame_period / 1000.0
    bs = band_signals(x, f0_floor, f0_ceil, fs) if bands is None else np.asarray(bands, np.float64)
    bfs = boundaries(f0_floor, f0_ceil)
    ev = [events(b) for b in bs]
    cs = [band_candidates(ev[b], bfs[b], t, f0_floor, f0_ceil, fs) for b in range(len(bfs))]
    cands = np.array([c for c, _ in cs])
    scores = np.array([s for _, s in cs])
    best = best_contour(cands, scores)
    f0 = fix_contour(best, cands, f0_floor, frame_period)
    return {'t': t, 'bands': bs, 'events': ev, 'cands': cands, 'scores': scores, 'best': best, 'f0': f0}


# ------------------------------------------------------------------------------------------------------ StoneMask
def _fix_f0(P, num, N, f0, nh, fs=FS):
    num_s = den_s = 0.0
    for i in range(nh):
        k = min(mround(f0 * N / fs * (i + 1)), N // 2)        # clamped: WORLD would read past N/2 + 1
        inst = 0.0 if P[k] == 0.0 else k * fs / N + num[k] / P[k] * fs / 2.0 / np.pi
        a = math.sqrt(P[k])
        num_s += a * inst
        den_s += a * (i + 1.0)
    return num_s / (den_s + SAFE)


def stonemask_frame(x, t, f0, fs=FS, detail=False):
    """Refined f0 of one frame; (refined, fell_back) with detail=True."""
    if f0 <= 40.0 or f0 > fs / 12.0:
        return (0.0, False) if detail else 0.0
    S = len(x)
    h = int(1.5 * fs / f0 + 1.0)
    n = 2 * h + 1
    wl = n / fs
    N = stonemask_fft_size(f0, fs)
    bt = (np.arange(n) - h) / fs
    raw = np.array([mround((t + b) * fs) for b in bt])
    tmp = (raw - 1.0) / fs - t
    mw = 0.42 + 0.5 * np.cos(2.0 * np.pi * tmp / wl) + 0.08 * np.cos(4.0 * np.pi * tmp / wl)
    dw = np.empty(n)
    dw[0] = -mw[1] / 2.0
    dw[1:-1] = -(mw[2:] - mw[:-2]) / 2.0
    dw[-1] = mw[-2] / 2.0
    xs = x[np.clip(raw - 1, 0, S - 1)]
    M = np.fft.rfft(xs * mw, N)
    D = np.fft.rfft(xs * dw, N)
    num = M.real * D.imag - M.imag * D.real
    P = M.real * M.real + M.imag * M.imag
    tent = _fix_f0(P, num, N, f0, 2, fs)
    mean = 0.0 if (tent <= 0.0 or tent > f0 * 2) else _fix_f0(P, num, N, tent, 6, fs)
    back = abs(mean - f0) > f0 * 0.2
    r = f0 if back else mean
    return (r, back) if detail else r


# ---------------------------------------------------------------------------------------------------- shared pieces
def windowed(x, t, f0, kind, ratio, fs=FS):
    """common.cpp GetWindowedWaveform without the randn() safeguard: window (hanning / blackman), samples clamped to the
    signal, the window-weighted mean removed.  -> (waveform [2h+1], window)."""
    h = mround(ratio * fs / f0 / 2.0)
    k = np.arange(-h, h + 1)
    origin = mround(t * fs + 0.001)
    xs = np.asarray(x, np.float64)[np.clip(origin + k, 0, len(x) - 1)]
    pos = (2.0 * k / ratio) / fs
    if kind == 'hanning':
        w = 0.5 * np.cos(np.pi * pos * f0) + 0.5
    else:
        w = 0.42 + 0.5 * np.cos(np.pi * pos * f0) + 0.08 * np.cos(np.pi * pos * f0 * 2)
    wave = xs * w
    wave = wave - w * (wave.sum() / w.sum())
    return wave, w


def dc_correction(P, f0, N, fs=FS):
    P = np.asarray(P, np.float64)
    ul = 2 + int(f0 * N / fs)
    out = P.copy()
    dy = np.append(P[1:ul + 1] - P[:ul], 0.0)           # delta_y over x_length = ul + 1 points
    for i in range(ul - 1):
        q = (i * fs / N - f0) / (-fs / N)
        b = int(q)
        out[i] = P[i] + (P[b] + dy[b] * (q - b))
    return out


def linear_smoothing(P, width, N, fs=FS):
    P = np.asarray(P, np.float64)
    bd = int(width * N / fs) + 1
    half = N // 2
    mirror = np.concatenate([P[bd:0:-1], P[:half], P[half:half - bd - 1:-1]])
    seg = np.cumsum(mirror * fs / N)
    x0 = -(bd - 0.5) * fs / N
    dx = fs / N
    dy = np.append(seg[1:] - seg[:-1], 0.0)
    fa = np.arange(half + 1) / N * fs - width / 2.0

    def q(xi):
        v = (xi - x0) / dx
        b = v.astype(np.int64)
        return seg[b] + dy[b] * (v - b)
    lo = q(fa)
    hi = q(fa + width)
    return (hi - lo) / width


# ---------------------------------------------------------------------------------------------------- CheapTrick
def ct_f0_floor(fs=FS, N=N_CT):
    return 3.0 * fs / (N - 3.0)


def cheaptrick_frame(x, t, f0, fs=FS, N=N_CT):
    """Linear power envelope [N/2 + 1] of one frame."""
    f = 500.0 if f0 <= ct_f0_floor(fs, N) else f0
    h = mround(1.5 * fs / f)
    k = np.arange(-h, h + 1)
    origin = mround(t * fs + 0.001)
    xs = np.asarray(x, np.float64)[np.clip(origin + k, 0, len(x) - 1)]
    w = 0.5 * np.cos(np.pi * (k / 1.5 / fs) * f) + 0.5
    w = w / math.sqrt((w * w).sum())
    wave = xs * w
    wave = wave - w * (wave.sum() / w.sum())
    X = np.fft.rfft(wave, N)
    P = X.real * X.real + X.imag * X.imag
    P = dc_correction(P, f, N, fs)
    P = linear_smoothing(P, f * 2.0 / 3.0, N, fs) + EPS
    q = np.arange(1, N // 2 + 1) / fs
    sl = np.concatenate([[1.0], np.sin(np.pi * f * q) / (np.pi * f * q)])
    cl = np.concatenate([[(1.0 - 2.0 * Q1) + 2.0 * Q1], (1.0 - 2.0 * Q1) + 2.0 * Q1 * np.cos(2.0 * np.pi * q * f)])
    lg = np.log(P)
    full = np.concatenate([lg, lg[N // 2 - 1:0:-1]])
    C = np.fft.fft(full).real[:N // 2 + 1]
    env = np.fft.irfft(C * sl * cl / N, N) * N        # unnormalised c2r of the real, even lifted cepstrum
    return np.exp(env[:N // 2 + 1])


# ------------------------------------------------------------------------------------------------------------ D4C
def lovetrain_frame(x, t, f0, fs=FS):
    if f0 == 0.0:
        return 0.0
    f = max(f0, 40.0)
    N = int(2.0 ** (1 + int(math.log(3.0 * fs / 40.0 + 1) / math.log(2.0))))
    b0, b1, b2 = int(math.ceil(100.0 * N / fs)), int(math.ceil(4000.0 * N / fs)), int(math.ceil(7900.0 * N / fs))
    wave, _ = windowed(x, t, f, 'blackman', 3.0, fs)
    X = np.fft.rfft(wave, N)
    P = X.real * X.real + X.imag * X.imag
    P[:b0 + 1] = 0.0
    c = np.cumsum(P[:b2 + 1])
    return 0.0 if c[b2] == 0.0 else c[b1] / c[b2]


def _centroid(x, t, f, N, fs):
    wave, _ = windowed(x, t, f, 'blackman', 4.0, fs)
    p = (wave * wave).sum()
    if p > 0.0:
        wave = wave / math.sqrt(p)
    A = np.fft.rfft(wave, N)
    B = np.fft.rfft(wave * (np.arange(len(wave)) + 1.0), N)
    return B.real * A.real + A.imag * B.imag


def nuttall(n):
    t = np.arange(n) / (n - 1.0)
    return 0.355768 - 0.487396 * np.cos(2 * np.pi * t) + 0.144232 * np.cos(4 * np.pi * t) - 0.012604 * np.cos(6 * np.pi * t)


def d4c_coarse(x, t, f0, fs=FS, N=N_D4C):
    """The one coarse aperiodicity (dB) of a voiced frame at 16 kHz, after the f0-based revision."""
    f = max(47.0, f0)
    n_ap = int(min(15000.0, fs / 2.0 - 3000.0) / 3000.0)
    assert n_ap == 1
    sc = _centroid(x, t - 0.25 / f, f, N, fs) + _centroid(x, t + 0.25 / f, f, N, fs)
    sc = dc_correction(sc, f, N, fs)
    wave, _ = windowed(x, t, f, 'hanning', 4.0, fs)
    X = np.fft.rfft(wave, N)
    sp = dc_correction(X.real * X.real + X.imag * X.imag, f, N, fs)
    sp = linear_smoothing(sp, f, N, fs)
    with np.errstate(divide='ignore', invalid='ignore'):
        gd = np.where(sp > 0.0, sc / sp, 0.0)
    gd = linear_smoothing(gd, f / 2.0, N, fs)
    gd = gd - linear_smoothing(gd, f, N, fs)
    wl = int(3000.0 * N / fs) * 2 + 1
    win = nuttall(wl)
    center = int(3000.0 * N / fs)
    hw = wl // 2
    X = np.fft.rfft(gd[center - hw:center - hw + wl] * win, N)
    P = np.sort(X.real * X.real + X.imag * X.imag)
    c = np.cumsum(P)
    bd = mround(N * 8.0 / wl)
    coarse = 0.0 if c[N // 2] == 0.0 else 10 * math.log10(c[N // 2 - bd - 1] / c[N // 2])
    return min(0.0, coarse + (f - 100) / 50.0)


def ap_from_coarse(coarse, fs=FS, N=N_CT):
    """interp1 over [0, 3000, fs/2] of [-60, coarse, -1e-12] dB at the N/2 + 1 bins, then 10^(dB / 20)."""
    xa = np.array([0.0, 3000.0, fs / 2.0])
    ya = np.array([-60.0, coarse, -SAFE])
    fa = np.arange(N // 2 + 1) * fs / N
    k = np.clip(np.searchsorted(xa, fa, side='right'), 1, 2)
    s = (fa - xa[k - 1]) / (xa[k] - xa[k - 1])
    return 10.0 ** ((ya[k - 1] + s * (ya[k] - ya[k - 1])) / 20.0)


# ---------------------------------------------------------------------------------------------------- the whole run
def analyze(x, fs=FS, frame_period=5.0, f0_floor=71.0, f0_ceil=500.0, bands=None, dio_f0=None):
    """One utterance x [S] (float64 in [-1, 1]) -> dict with f0 (refined), sp (linear), ap, the record's sp / en, and
    the intermediates.  `bands` / `dio_f0` replace those stages' results (the GPU tests feed the device's own)."""
    if fs != FS:
        raise ValueError('only fs = 16000 is specified')
    x = np.asarray(x, np.float64)
    d = dio(x, f0_floor, f0_ceil, fs, frame_period, bands)
    f0d = d['f0'] if dio_f0 is None else np.asarray(dio_f0, np.float64)
    t = d['t']
    T = len(t)
    f0 = np.zeros(T)
    back = np.zeros(T, bool)
    for i in range(T):
        f0[i], back[i] = stonemask_frame(x, t[i], f0d[i], fs, detail=True)
    sp = np.array([cheaptrick_frame(x, t[i], f0[i], fs) for i in range(T)])
    ap0 = np.array([lovetrain_frame(x, t[i], f0[i], fs) for i in range(T)])
    ap = np.full((T, H), AP_UNVOICED)
    coarse = np.zeros(T)
    for i in range(T):
        if f0[i] == 0 or ap0[i] <= THRESHOLD:
            continue
        coarse[i] = d4c_coarse(x, t[i], f0[i], fs)
        ap[i] = ap_from_coarse(coarse[i], fs)
    en = np.sum(sp + 1e-10, axis=1)
    rec_sp = np.log10(sp / en[:, None])
    d.update(f0_dio=f0d, f0=f0, fell_back=back, sp_lin=sp, ap0=ap0, coarse=coarse, ap=ap, en=en, sp=rec_sp)
    return d


def max_fft_size(f0_floor, f0_ceil, fs=FS):
    """Largest FFT any stage derives from the f0 limits (StoneMask at f0_floor; CheapTrick, LoveTrain, D4C fixed)."""
    return max(stonemask_fft_size(f0_floor, fs), N_CT, N_D4C,
               int(2.0 ** (1 + int(math.log(3.0 * fs / 40.0 + 1) / math.log(2.0)))),
               int(2.0 ** (1 + int(math.log(4.0 * fs / 47.0 + 1) / math.log(2.0)))))
