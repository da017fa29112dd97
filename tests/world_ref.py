"""Float64 NumPy restatement of the device WORLD-style synthesis (vaenpvc_synthesize, csrc/gfx950_synth.hip), test helper:
the product never imports it.  It states DESIGN.md section 14 step by step; sample-level equality with pyworld is not
claimed (no WORLD source or pyworld exists anywhere this project runs).  Vectorised over pulses, in blocks of pulses to
bound memory.  The noise is oracle/philox_ref.normal, the NumPy form of the device draw."""
import numpy as np

from oracle import philox_ref

N = 1024                   # FFT size
H = N // 2 + 1             # spectral bins (513)
F0_CEIL = 1000.0           # VAENPVC_SYNTH_F0_CEIL
F0_UNVOICED = 500.0
FLT_MIN = float(np.finfo(np.float32).tiny)
AP_LO, AP_HI = 0.001, 0.999999999999
TWO_PI = 2.0 * np.pi
BLOCK = 1024               # pulses per vectorised block


def n_samples(T, frame_period, fs):
    """S = floor(T * frame_period_ms * fs / 1000) (pyworld's y_length), host float64."""
    return int(np.floor(T * frame_period * fs / 1000.0))


def capacity(S, fs):
    """Most pulses an utterance of S samples can hold: floor(S * 1000 / fs) + 1 (pulses beyond it are dropped)."""
    return S * 1000 // fs + 1


def coarse(f0, fs):
    """cf0 / cvuv [T+1]: f0 below fs/N + 1 Hz or non-finite -> 0 (unvoiced), one point extrapolated at T * Pd."""
    f0 = np.asarray(f0, np.float64)
    lowest = fs / N + 1.0
    with np.errstate(invalid='ignore'):
        cf0 = np.where(np.isfinite(f0) & (f0 >= lowest), f0, 0.0)
    cvuv = (cf0 != 0.0).astype(np.float64)
    if len(cf0) == 1:
        return np.append(cf0, cf0[0]), np.append(cvuv, cvuv[0])
    return np.append(cf0, 2.0 * cf0[-1] - cf0[-2]), np.append(cvuv, 2.0 * cvuv[-1] - cvuv[-2])


def time_base(f0, S, fs, frame_period):
    """Per-sample f0 f [S] and voicing vuv [S], the float64 phase, and the pulses: sample i [P] and fractional shift x [P]."""
    cf0, cvuv = coarse(f0, fs)
    T = len(cf0) - 1
    Pd = frame_period / 1000.0
    pos = (np.arange(S) / fs) / Pd
    k = np.minimum(np.floor(pos).astype(np.int64), T - 1)
    frac = pos - k
    fi = cf0[k] + (cf0[k + 1] - cf0[k]) * frac
    vi = cvuv[k] + (cvuv[k + 1] - cvuv[k]) * frac
    vuv = vi > 0.5
    f = np.where(vuv, fi, F0_UNVOICED)
    f = np.where(f < F0_CEIL, f, F0_CEIL)
    phase = np.cumsum(TWO_PI * f / fs)          # sequential float64 accumulation
    w = np.fmod(phase, TWO_PI)
    i = np.nonzero(np.abs(w[1:] - w[:-1]) > np.pi)[0]
    i = i[:capacity(S, fs)]
    x = -(w[i] - TWO_PI) / (w[i + 1] - (w[i] - TWO_PI))
    return f, vuv, i, x


def min_phase(a):
    """Minimum-phase spectrum of the log-amplitude a [..., N/2+1]: exp(FFT(fold(real(IFFT(mirror(a))))))[..., :N/2+1]."""
    full = np.concatenate([a, a[..., -2:0:-1]], axis=-1)
    c = np.fft.ifft(full, axis=-1).real
    ch = np.zeros_like(c)
    ch[..., 0] = c[..., 0]
    ch[..., 1:N // 2] = 2.0 * c[..., 1:N // 2]
    ch[..., N // 2] = c[..., N // 2]
    return np.exp(np.fft.fft(ch, axis=-1)[..., :H])


def dc_window():
    """WORLD's DC remover, normalised: sum over all N points is 1."""
    i = np.arange(N // 2)
    h = 0.5 - 0.5 * np.cos(TWO_PI * (i + 1.0) / (N + 1))
    w = np.concatenate([h, h[::-1]])
    return w / (2.0 * h.sum())


def pulse_spectra(sp, en, ap, i_p, fs, frame_period):
    """E (linear envelope) and R (squared aperiodicity ratio) at the pulses' unshifted times, [P, H] float64."""
    T = sp.shape[0]
    Pd = frame_period / 1000.0
    q = (i_p / fs) / Pd
    fl = np.minimum(T - 1, np.floor(q)).astype(np.int64)
    ce = np.minimum(T - 1, np.ceil(q)).astype(np.int64)
    a = (q - fl)[:, None]
    Sp = np.abs(np.asarray(en, np.float64)[:, None] * np.power(10.0, np.asarray(sp, np.float64)))
    E = (1.0 - a) * Sp[fl] + a * Sp[ce]
    c = np.clip(np.asarray(ap, np.float64), AP_LO, AP_HI)
    R = ((1.0 - a) * c[fl] + a * c[ce]) ** 2
    return E, R


def segments(f0, sp, en, ap, fs=16000, frame_period=5.0, seed=0, parts=('per', 'aper')):
    """One utterance -> pulse samples i [P], segment lengths ns [P] and the segments r [P, N] (float64)."""
    T = len(f0)
    S = n_samples(T, frame_period, fs)
    if S < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, N))
    _, vuv, i_p, x = time_base(f0, S, fs, frame_period)
    P = len(i_p)
    if P == 0:
        return i_p, np.zeros(0, np.int64), np.zeros((0, N))
    ns = np.zeros(P, np.int64)
    ns[:-1] = np.minimum(np.diff(i_p), N)
    noise = philox_ref.normal(int(i_p[-1] - i_p[0]) + 1, seed).astype(np.float64)
    wd = dc_window()
    kk = np.arange(H)
    jj = np.arange(N)
    r = np.zeros((P, N))
    for b0 in range(0, P, BLOCK):
        sl = slice(b0, min(P, b0 + BLOCK))
        ib, xb, nb, vb = i_p[sl], x[sl], ns[sl], vuv[i_p[sl]]
        E, R = pulse_spectra(sp, en, ap, ib, fs, frame_period)
        live = nb > 0
        out = np.zeros((len(ib), N))
        if 'per' in parts:
            on = vb & (R[:, 0] <= 0.999) & live
            with np.errstate(divide='ignore'):
                a = 0.5 * np.log(np.maximum(E * (1.0 - R) + 1e-12, FLT_MIN))
            M = min_phase(a) * np.exp(-1j * TWO_PI * kk[None, :] * xb[:, None] / N)
            per = np.fft.fftshift(np.fft.irfft(M, N, axis=-1) * N, axes=-1)
            d = per[:, N // 2:].sum(axis=-1, keepdims=True)
            per[:, :N // 2] = -d * wd[None, :N // 2]
            per[:, N // 2:] -= d * wd[None, N // 2:]
            out += np.where(on[:, None], per * np.sqrt(nb)[:, None], 0.0)
        if 'aper' in parts:
            idx = (ib - i_p[0])[:, None] + jj[None, :]
            msk = jj[None, :] < nb[:, None]
            z = np.where(msk, noise[np.minimum(idx, len(noise) - 1)], 0.0)
            mean = z.sum(axis=-1) / np.maximum(nb, 1)
            z = np.where(msk, z - mean[:, None], 0.0)
            with np.errstate(divide='ignore'):
                a = 0.5 * np.log(np.maximum(np.where(vb[:, None], E * R, E), FLT_MIN))
            A = np.fft.rfft(z, N, axis=-1) * min_phase(a)
            out += np.fft.fftshift(np.fft.irfft(A, N, axis=-1) * N, axes=-1)
        r[sl] = np.where(live[:, None], out / N, 0.0)
    return i_p, ns, r


def synthesize(f0, sp, en, ap, fs=16000, frame_period=5.0, seed=0, parts=('per', 'aper')):
    """One utterance: f0 [T], sp [T, H] (log10, energy-normalised), en [T], ap [T, H] -> y [S] float64."""
    S = n_samples(len(f0), frame_period, fs)
    y = np.zeros(S)
    i_p, _, r = segments(f0, sp, en, ap, fs, frame_period, seed, parts)
    for p in range(len(i_p)):
        lo = int(i_p[p]) - N // 2 + 1
        a, b = max(0, lo), min(S, lo + N)
        if a < b:
            y[a:b] += r[p, a - lo:b - lo]
    return y


def batch(f0, sp, en, ap, lengths, fs=16000, frame_period=5.0, seed=0, parts=('per', 'aper')):
    """Utterances of `lengths` frames stored back to back -> the list of their waveforms."""
    out, o = [], 0
    for T in lengths:
        out.append(synthesize(f0[o:o + T], sp[o:o + T], en[o:o + T], ap[o:o + T], fs, frame_period, seed, parts))
        o += T
    return out
