"""Float64 restatement of the global-variance (GV) post-filter and of its speaker statistics (test helper: the product
never imports it).  Domain: the log10 spectral envelope sp; an utterance is one .bin file, all of its frames."""
import numpy as np

V_MIN = 1e-8


def utterance_variance(s):
    """v_u[d] = (1/N) sum_t (s[t,d] - mu_u[d])^2 (biased)."""
    s = np.asarray(s, np.float64)
    return ((s - s.mean(axis=0)) ** 2).mean(axis=0)


def speaker_gv(utterances):
    """g_spk[d]: mean of v_u[d] over the speaker's utterances with N >= 2 (float64)."""
    vs = [utterance_variance(s) for s in utterances if len(s) >= 2]
    return np.mean(np.stack(vs), axis=0)


def postfilter(c, g):
    """One converted utterance c [N, H] (sp domain) -> out [N, H]: mu_c + sqrt(g / v_c) (c - mu_c) where v_c > 1e-8,
    c elsewhere."""
    c = np.asarray(c, np.float64)
    g = np.asarray(g, np.float64)
    mu = c.mean(axis=0)
    v = ((c - mu) ** 2).mean(axis=0)
    on = v > V_MIN
    scale = np.sqrt(g / np.where(on, v, 1.0))
    return np.where(on, mu + scale * (c - mu), c), on


def tanhize_backward(x, xmin, xmax):
    x = np.asarray(x, np.float64)
    xmin = np.asarray(xmin, np.float64)
    return (x * 0.5 + 0.5) * (np.asarray(xmax, np.float64) - xmin) + xmin


def batch(x, lengths, xmin, xmax, g):
    """Decoder output x [F, H] (Tanhize domain) holding utterances of `lengths` frames back to back -> filtered sp
    (float64) and the per-utterance masks of filtered bins."""
    out, masks, o = [], [], 0
    for n in lengths:
        r, on = postfilter(tanhize_backward(x[o:o + n], xmin, xmax), g)
        out.append(r)
        masks.append(on)
        o += n
    return np.concatenate(out, axis=0), masks
