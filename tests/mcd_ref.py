"""Float64 NumPy restatement of the DTW-aligned mel-cepstral distortion (the device path is
csrc/gfx950_dtw.hip behind hipvae.metrics.mcd_dtw).  Written for clarity: the DP is a Python double loop.

Inputs per utterance are what a .bin record holds (float32): sp [T, 513] = log10(sp / en), en [T], f0 [T]."""
import numpy as np

H = 513
N = 1024
DB_FACTOR = 6.1418514637137541          # 10 sqrt(2) / ln 10 (VAENPVC_MCD_DB_FACTOR)


def log_amplitude(sp, en):
    """L[t, k] = 0.5 (ln 10 sp[t, k] + ln en[t])"""
    sp = np.asarray(sp, np.float64)
    en = np.asarray(en, np.float64)
    return 0.5 * (np.log(10.0) * sp + np.log(en)[:, None])


def warp(omega, alpha):
    """Phase of the first-order all-pass: w(omega) = omega + 2 atan(alpha sin omega / (1 - alpha cos omega))."""
    return omega + 2.0 * np.arctan(alpha * np.sin(omega) / (1.0 - alpha * np.cos(omega)))


def freqt(c1, m2, alpha):
    """SPTK's freqt: c1 [m1 + 1, ...] (coefficients of cos(m omega)) -> [m2 + 1, ...] (coefficients of cos(m w(omega))).
    Trailing axes are carried along, so a matrix of column vectors transforms in one pass."""
    c1 = np.asarray(c1, np.float64)
    m1 = c1.shape[0] - 1
    b = 1.0 - alpha * alpha
    g = np.zeros((m2 + 1,) + c1.shape[1:])
    for i in range(m1, -1, -1):
        d = g.copy()
        g[0] = c1[i] + alpha * d[0]
        if m2 >= 1:
            g[1] = b * d[0] + alpha * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
    return g


def cepstrum_matrix():
    """CT [513, 513]: ct = CT L, the one-sided real cepstrum of the 1024-point symmetric extension of L
    (ct[0] = c[0], ct[m] = 2 c[m], ct[512] = c[512])."""
    n = np.arange(H)
    edge = np.where((n == 0) | (n == H - 1), 1.0, 2.0)
    cos = np.cos(np.pi * ((n[:, None] * n[None, :]) % N) / 512.0)
    return edge[:, None] * cos * edge[None, :] / N


def mcep_matrix(order=24, alpha=0.42):
    """W [(order + 1), 513] with mc = W L."""
    return freqt(np.eye(H), order, alpha) @ cepstrum_matrix()


def mcep(sp, en, W):
    """mc[t] = W L[t], frame by frame: equal frames give equal coefficients bit for bit wherever they stand (one matrix
    product over all frames may block its rows differently)."""
    return np.stack([W @ l for l in log_amplitude(sp, en)])


def cost_matrix(mcA, mcB):
    """d(i, j) = sqrt(sum_{m >= 1} (mcA[i, m] - mcB[j, m])^2): the gain coefficient is left out."""
    d = mcA[:, None, 1:] - mcB[None, :, 1:]
    return np.sqrt((d * d).sum(-1))


def diag_index(Ta, Tb):
    """Where cell (i, j) stands when the matrix is stored anti-diagonal after anti-diagonal (s = i + j ascending, i
    ascending inside a diagonal): the layout of the device's cost, code and D.  int64 [Ta, Tb]."""
    i, j = np.indices((Ta, Tb))
    order = np.lexsort((i.ravel(), (i + j).ravel()))
    idx = np.empty(Ta * Tb, np.int64)
    idx[order] = np.arange(Ta * Tb)
    return idx.reshape(Ta, Tb)


def dp(cost):
    """D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)); on equal values the predecessor is the diagonal (code 0),
    then (i-1, j) (code 1), then (i, j-1) (code 2).  -> D, codes (uint8; (0, 0) holds 0)."""
    Ta, Tb = cost.shape
    c = np.asarray(cost, np.float64).tolist()          # Python floats are the same IEEE doubles; lists index faster
    inf = float('inf')
    D, code = [], []
    for i in range(Ta):
        up_row = D[i - 1] if i > 0 else None
        Di, ki, ci = [], [], c[i]
        for j in range(Tb):
            if i == 0 and j == 0:
                Di.append(ci[0])
                ki.append(0)
                continue
            best, k = (up_row[j - 1], 0) if i > 0 and j > 0 else (inf, 0)
            up = up_row[j] if i > 0 else inf
            left = Di[j - 1] if j > 0 else inf
            if up < best:
                best, k = up, 1
            if left < best:
                best, k = left, 2
            Di.append(ci[j] + best)
            ki.append(k)
        D.append(Di)
        code.append(ki)
    return np.array(D, np.float64).reshape(Ta, Tb), np.array(code, np.uint8).reshape(Ta, Tb)


def backtrace(code):
    """The path from (Ta-1, Tb-1) to (0, 0) in that (back-trace) order, int32 [P, 2]."""
    i, j = code.shape[0] - 1, code.shape[1] - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        k = 2 if i == 0 else 1 if j == 0 else int(code[i, j])
        if k == 0:
            i, j = i - 1, j - 1
        elif k == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return np.array(path, np.int32)


def log_f0(f0):
    """ln f0 where f0 > 1 (voiced), otherwise -1 (the workspace's lf0 region)."""
    f0 = np.asarray(f0, np.float32)
    v = f0 > 1.0
    return np.where(v, np.log(np.where(v, f0, 2.0).astype(np.float64)), -1.0)


def path_sums(cost, path, lfA, lfB, D_end=np.nan):
    """The eight result fields, summed in back-trace order with one rounding per operation."""
    s = 0.0
    sq = 0.0
    nboth = nmis = 0
    for i, j in path:
        s = s + cost[i, j]
        va, vb = lfA[i] >= 0.0, lfB[j] >= 0.0
        if va and vb:
            e = lfA[i] - lfB[j]
            sq = sq + e * e
            nboth += 1
        elif va != vb:
            nmis += 1
    P = len(path)
    rmse = np.sqrt(np.float64(sq) / np.float64(nboth)) if nboth else np.nan
    return np.array([(DB_FACTOR * s) / np.float64(P), P, D_end, rmse, nboth, nmis, s, 0.0], np.float64)


def min_gap(D, path):
    """Smallest relative gap between the best and the second-best predecessor over the path's interior decisions (cells
    with i > 0 and j > 0): how far the path is from a near-tie.  inf when there is no such cell."""
    gap = np.inf
    for i, j in path:
        if i > 0 and j > 0:
            c = np.sort([D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]])
            gap = min(gap, (c[1] - c[0]) / max(abs(c[1]), 1e-300))
    return gap


def mcd_pair(spA, enA, f0A, spB, enB, f0B, order=24, alpha=0.42, W=None, full=False):
    """One pair end to end -> the eight result fields (and with full=True a dict of every intermediate)."""
    if W is None:
        W = mcep_matrix(order, alpha)
    mcA, mcB = mcep(spA, enA, W), mcep(spB, enB, W)
    cost = cost_matrix(mcA, mcB)
    D, code = dp(cost)
    path = backtrace(code)
    res = path_sums(cost, path, log_f0(f0A), log_f0(f0B), D[-1, -1])
    if full:
        return dict(mcA=mcA, mcB=mcB, cost=cost, D=D, code=code, path=path, results=res)
    return res


def mcd_batch(spA, enA, f0A, lengthsA, spB, enB, f0B, lengthsB, order=24, alpha=0.42, return_path=False):
    """The host twin of hipvae.metrics.mcd_dtw on NumPy arrays: utterances stored back to back -> results [n_pair, 8]
    (and the forward-order paths)."""
    W = mcep_matrix(order, alpha)
    oa = np.concatenate([[0], np.cumsum(lengthsA)])
    ob = np.concatenate([[0], np.cumsum(lengthsB)])
    out, paths = [], []
    for p in range(len(lengthsA)):
        a, b = slice(oa[p], oa[p + 1]), slice(ob[p], ob[p + 1])
        r = mcd_pair(spA[a], enA[a], f0A[a], spB[b], enB[b], f0B[b], W=W, full=True)
        out.append(r['results'])
        paths.append(r['path'][::-1].copy())
    out = np.array(out)
    return (out, paths) if return_path else out
