"""Float64 NumPy restatement of the resampler of DESIGN.md section 18 (include/vaenpvc.h, vaenpvc_resample): plan,
weight table and the resampling of a list of segments.  It does not import the library.

Rates rate_in -> rate_out, g = gcd, L = rate_out / g, M = rate_in / g, s = min(1, L / M), K = ceil(Z / s).  Prototype in
input-sample time t:  h(t) = s R sinc(s R t) I0(B sqrt(1 - v^2)) / I0(B),  v = s t / Z,  h = 0 where |v| >= 1.  Output m
of a segment of n samples (m < (n L + M - 1) // M) sits at u = m M / L and is
    y[m] = sum_{j = -K+1 .. K} x[floor(u) + j] h(frac(u) - j)
with x zero outside the segment, summed in float64 in ascending j, rounded once to float32.  Z, B and R are the values
resampy documents for `kaiser_best`."""
import math

import numpy as np

Z = 64
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596
MAX_TABLE = 1 << 24


def plan(rate_in, rate_out):
    """(L, M, K); integer arithmetic only."""
    g = math.gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    K = (Z * M + L - 1) // L if M > L else Z
    return L, M, K


def out_length(n, L, M):
    return (n * L + M - 1) // M


def h(t, L, M):
    """The prototype at input-sample times t (float64 array)."""
    t = np.asarray(t, np.float64)
    s = L / M if M > L else 1.0
    c = s * ROLLOFF
    v = s * t / Z
    inside = np.abs(v) < 1.0
    w = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - v * v, 0.0))) / np.i0(BETA)
    return np.where(inside, c * np.sinc(c * t) * w, 0.0)


def table(rate_in, rate_out):
    """T [2K, L]: T[j + K - 1, r] = h(((r M) mod L) / L - j)."""
    L, M, K = plan(rate_in, rate_out)
    frac = ((np.arange(L, dtype=np.int64) * M) % L).astype(np.float64) / float(L)
    j = np.arange(-K + 1, K + 1, dtype=np.float64)
    return h(frac[None, :] - j[:, None], L, M)


def resample_segment(x, rate_in, rate_out, T=None, as_float32=True):
    """One segment.  float32 (the one rounding) unless as_float32 is False."""
    L, M, K = plan(rate_in, rate_out)
    T = table(rate_in, rate_out) if T is None else T
    x = np.asarray(x, np.float64)
    n = len(x)
    n_out = out_length(n, L, M)
    m = np.arange(n_out, dtype=np.int64)
    q = (m * M) // L
    r = m % L
    xp = np.concatenate([np.zeros(K), x, np.zeros(K + 1)])      # xp[i + K] = x[i]
    acc = np.zeros(n_out)
    for jj in range(2 * K):                                      # ascending j = jj - K + 1, one product and one sum each
        acc = acc + xp[q + jj + 1] * T[jj, r]
    return acc.astype(np.float32) if as_float32 else acc


def resample(xs, rate_in, rate_out, as_float32=True):
    """A list of segments -> the list of their resampled versions (each from its own samples alone)."""
    T = table(rate_in, rate_out)
    return [resample_segment(x, rate_in, rate_out, T, as_float32) for x in xs]


def within_one_ulp32(got, want32):
    """Every element of the float32 array `got` is within one float32 ulp (np.spacing) of the float32 array want32."""
    got, want32 = np.asarray(got), np.asarray(want32)
    assert got.dtype == np.float32 and want32.dtype == np.float32 and got.shape == want32.shape
    d = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    return bool(np.all(d <= np.spacing(np.abs(want32)).astype(np.float64)))
