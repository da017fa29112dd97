"""Device statistics (vaenpvc_column_select, vaenpvc_speaker_stats, csrc/gfx950_stats.hip) against the float64 / exact
restatement tests/stats_ref.py: order statistics, determinism, the non-finite flag, speaker statistics, and
`build.py --device` end to end against the host path."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import stats_ref
from helpers import PKG

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N_PATTERNS = 9


def load_build():
    spec = importlib.util.spec_from_file_location('vaenpvc_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pattern_column(rng, F, kind):
    if kind == 0:                                      # log-spectrum-like
        return 3 * rng.standard_normal(F) - 8
    if kind == 1:                                      # five distinct values only
        return rng.choice(np.array([-11.5, -8.0, -7.99, 0.25, 3.0]), F)
    if kind == 2:                                      # all equal
        return np.full(F, -6.125)
    if kind == 3:                                      # +-0.0 among a few others
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), F)
    if kind == 4:                                      # mixed signs, many binades
        return rng.standard_normal(F) * 10.0 ** rng.integers(-6, 6, F)
    if kind == 5:                                      # base + k ulps: only the lowest mantissa byte differs
        base = np.float32(-7.3125).view(np.uint32) & np.uint32(0xffffff00)
        return (base + rng.integers(0, 256, F).astype(np.uint32)).view(np.float32)
    if kind == 6:                                      # denormals of both signs
        bits = rng.integers(1, 1 << 23, F).astype(np.uint32) | (rng.integers(0, 2, F).astype(np.uint32) << np.uint32(31))
        return bits.view(np.float32)
    if kind == 7:                                      # strictly increasing
        return np.arange(F) * 0.37 - 50.0
    return 1e4 - np.arange(F) * 1.75                   # strictly decreasing


@functools.lru_cache(maxsize=None)
def case(F, H=513):
    """(x [F, H] float32, its columns sorted [F, H]): column h holds pattern h % 9.  Computed once, never modified."""
    rng = np.random.default_rng(1000 + F)
    x = np.stack([np.asarray(pattern_column(rng, F, h % N_PATTERNS), np.float32) for h in range(H)], axis=1)
    x = np.ascontiguousarray(x)
    srt = np.ascontiguousarray(np.sort(np.ascontiguousarray(x.T), axis=1).T)
    assert np.array_equal(srt[[0, F - 1]], stats_ref.order_stats(x, [0, F - 1]))
    x.setflags(write=False)
    srt.setflags(write=False)
    return x, srt


def on_device(x, ld):
    """x [F, H] on the device with row stride ld: ld == H contiguous; otherwise the leading columns of a record buffer
    [F, ld] whose other columns hold garbage (NaN, Inf, huge values: the select must not look at them)."""
    F, H = x.shape
    if ld == H:
        return torch.tensor(x, device=DEV)
    rng = np.random.default_rng(7)
    rec = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0], np.float32), (F, ld))
    rec[:, :H] = x
    return torch.from_numpy(rec).to(DEV)[:, :H]


def rank_sets(F):
    pr = stats_ref.percentile_ranks(F, [0.5, 99.5])
    mid = F // 2
    return [[0, F - 1], [r for lo, hi, _ in pr for r in (lo, hi)], [mid, 0, mid, F - 1, mid]]


@pytest.mark.parametrize('ld', ['H', 1029])
@pytest.mark.parametrize('H', [1, 37, 513])
@pytest.mark.parametrize('F', [1, 2, 3, 255, 256, 257, 4099])
def test_column_select_exact(F, H, ld):
    from hipvae import stats
    x, srt = case(F)
    x, srt = x[:, :H], srt[:, :H]
    d = on_device(x, H if ld == 'H' else ld)
    assert d.stride(0) == (H if ld == 'H' else ld) or F == 1
    for ranks in rank_sets(F):
        got = stats.column_select(d, ranks).cpu().numpy()
        assert got.shape == (len(ranks), H) and got.dtype == np.float32
        assert np.array_equal(got, srt[ranks]), (F, H, ld, ranks)
    qs = [0.5, 99.5, 37.3]
    p = stats.percentiles(d, qs).cpu().numpy()
    assert p.dtype == np.float32 and stats_ref.within_ulp32(p, stats_ref.percentiles_sorted(srt, qs).astype(np.float64))


def test_column_select_large_eight_ranks():
    from hipvae import stats
    F = 70001
    x, srt = case(F)
    pr = stats_ref.percentile_ranks(F, [0.5, 99.5])
    ranks = [r for lo, hi, _ in pr for r in (lo, hi)] + [0, F - 1, 65536, 12345]
    d = torch.tensor(x, device=DEV)
    got = stats.column_select(d, ranks).cpu().numpy()
    assert np.array_equal(got, srt[ranks])
    assert np.array_equal(got, stats_ref.order_stats(x, ranks))
    qs = [0.5, 99.5, 37.3]
    p = stats.percentiles(d, qs).cpu().numpy()
    assert np.array_equal(p, stats_ref.percentiles_sorted(srt, qs))      # the same float64 operations, rounded once


def test_column_select_deterministic_and_column_local():
    from hipvae import stats
    F = 4099
    x, _ = case(F)
    d = torch.tensor(x, device=DEV)
    ranks = rank_sets(F)[1]
    a = stats.column_select(d, ranks)
    b = stats.column_select(d, ranks)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    view = d[:, 100:137]                                                  # H = 37, ld = 513
    alone = stats.column_select(view, ranks)
    copy = stats.column_select(view.contiguous(), ranks)                  # H = ld = 37
    assert torch.equal(alone.view(torch.int32), a[:, 100:137].contiguous().view(torch.int32))
    assert torch.equal(copy.view(torch.int32), alone.view(torch.int32))


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_column_select_flags_non_finite(value):
    from hipvae import stats
    x = case(257)[0][:, :37].copy()
    d = torch.from_numpy(x).to(DEV)
    assert stats.column_select(d, [0, 256]).shape == (2, 37)              # finite: no error
    x[200, 36] = value
    with pytest.raises(ValueError, match='non-finite flag'):
        stats.column_select(torch.from_numpy(x).to(DEV), [0, 256])
    with pytest.raises(ValueError, match='non-finite flag'):
        stats.percentiles(torch.from_numpy(x).to(DEV), [0.5, 99.5])
    assert stats.column_select(d, [0, 256]).shape == (2, 37)              # the flag does not stick


def speaker_case(lengths, seed):
    rng = np.random.default_rng(seed)
    F = sum(lengths)
    sp = (rng.uniform(-9, -3, 513) + rng.uniform(0.05, 0.8, 513) * rng.standard_normal((F, 513))).astype(np.float32)
    f0 = rng.choice(np.array([0.0, 1.5, 2.0], np.float32), F)
    voiced = rng.random(F) > 0.4
    f0[voiced] = rng.uniform(60, 400, int(voiced.sum())).astype(np.float32)
    return sp, f0


def check_speaker_stats(got, want):
    (lf0, gv, n_utt), (rlf0, rgv, rn) = got, want
    assert np.array_equal(n_utt, rn)
    assert np.array_equal(lf0[:, 0], rlf0[:, 0])                          # counts are exact
    assert stats_ref.within_ulp32(lf0[:, 1:].astype(np.float32), rlf0[:, 1:])
    assert stats_ref.within_ulp32(gv.astype(np.float32), rgv)
    assert np.array_equal(np.isnan(gv), np.isnan(rgv)) and np.array_equal(np.isnan(lf0), np.isnan(rlf0))


def test_speaker_stats_against_float64():
    from hipvae import stats
    lengths, speakers, n_spk = [1, 2, 3, 57, 700], [0, 0, 3, 3, 9], 10
    sp, f0 = speaker_case(lengths, 3)
    f0[:6] = [2.0, 0.0, 180.0, 1.5, 2.0, 2.0000002]
    run = lambda s, f, l, k: tuple(t.cpu().numpy() for t in stats.speaker_stats(
        torch.from_numpy(s).to(DEV), torch.from_numpy(f).to(DEV), l, k, n_spk))
    base = run(sp, f0, lengths, speakers)
    check_speaker_stats(base, stats_ref.speaker_stats(sp, f0, lengths, speakers, n_spk))
    assert base[2].tolist() == [1, 0, 0, 2, 0, 0, 0, 0, 0, 1]
    assert base[0][0, 0] == (f0[:3] > 2).sum() and base[0][1, 0] == 0 and np.isnan(base[0][1, 1:]).all()

    # the same utterances between other speakers': 5 has one 1-frame utterance only, 7 has frames but none voiced
    others = [1, 5, 40, 9]
    osp, of0 = speaker_case(others, 4)
    of0[1:6] = [0.0, 1.5, 2.0, 0.0, 1.0]
    of0[46:] = [2.0, 0.0, 1.5, 0.0, 0.0, 2.0, 1.5, 0.0, 0.0]
    order = [('o', 0), ('o', 1), ('b', 0), ('b', 1), ('o', 2), ('b', 2), ('b', 3), ('o', 3), ('b', 4)]
    ospk = [5, 7, 1, 7]
    bo, oo = np.cumsum([0] + lengths), np.cumsum([0] + others)
    sp2 = np.concatenate([(sp[bo[i]:bo[i + 1]] if w == 'b' else osp[oo[i]:oo[i + 1]]) for w, i in order])
    f02 = np.concatenate([(f0[bo[i]:bo[i + 1]] if w == 'b' else of0[oo[i]:oo[i + 1]]) for w, i in order])
    len2 = [(lengths if w == 'b' else others)[i] for w, i in order]
    spk2 = [(speakers if w == 'b' else ospk)[i] for w, i in order]
    emb = run(sp2, f02, len2, spk2)
    check_speaker_stats(emb, stats_ref.speaker_stats(sp2, f02, len2, spk2, n_spk))
    assert emb[2][5] == 0 and emb[0][5, 0] == (of0[:1] > 2).sum()
    assert emb[0][7, 0] == 0 and np.isnan(emb[0][7, 1:]).all() and emb[2][7] == 2
    for s in (0, 3, 9):                                                   # same bytes wherever the utterances stand
        for a, b in zip(base, emb):
            assert a[s].tobytes() == b[s].tobytes(), s
    for s in (2, 4, 6, 8):
        assert emb[0][s, 0] == 0 and emb[2][s] == 0 and np.isnan(emb[1][s]).all()

    # strided inputs: sp and f0 as columns of one record buffer
    rec = np.full((sum(lengths), 1029), np.nan, np.float32)
    rec[:, :513], rec[:, 1026] = sp, f0
    d = torch.from_numpy(rec).to(DEV)
    strided = tuple(t.cpu().numpy() for t in stats.speaker_stats(d[:, :513], d[:, 1026], lengths, speakers, n_spk))
    for a, b in zip(base, strided):
        assert a.tobytes() == b.tobytes()


def test_speaker_stats_rejects_malformed_layout():
    from hipvae import stats
    sp = torch.zeros(10, 513, device=DEV)
    f0 = torch.zeros(10, device=DEV)
    for lengths, speakers in (([4, 5], [0, 1]), ([4, 6], [0]), ([4, 6], [0, 10]), ([4, 6], [-1, 0]), ([-1, 11], [0, 0]),
                              ([], [])):
        with pytest.raises(ValueError):
            stats.speaker_stats(sp, f0, lengths, speakers, 10)


def test_build_device_end_to_end(tmp_path, monkeypatch):
    pattern, utts = stats_ref.write_e2e_tree(str(tmp_path / 'data'))
    ref = stats_ref.e2e_restatement(utts)
    build = load_build()
    out = {}
    for mode, argv in (('host', []), ('device', ['--device'])):
        wd = tmp_path / mode
        wd.mkdir()
        monkeypatch.chdir(wd)
        build.main(argv + ['--train_file_pattern', pattern])
        out[mode] = {n: np.fromfile(str(wd / 'etc' / n), np.float32) for n in sorted(os.listdir(str(wd / 'etc')))}
    assert sorted(out['host']) == sorted(out['device']) == sorted(k for k in ref if k.endswith('.npf'))
    for name in sorted(out['host']):
        host, dev, want = out['host'][name], out['device'][name], ref[name]
        assert host.shape == dev.shape == want.shape, name
        err = np.abs(dev.astype(np.float64) - want) / stats_ref.ulp32(want)
        print('%s: device max %.3f float32 ulp from the restatement' % (name, err.max()))
        assert stats_ref.within_ulp32(dev, want), (name, err.max())
        if name in ('xmin.npf', 'xmax.npf'):
            a, b = ref[name[:-4] + '.bracket']
            assert np.all((a <= dev) & (dev <= b)) and np.all((a <= host) & (host <= b)), name
        else:
            slack = np.abs(host.astype(np.float64) - want) + stats_ref.ulp32(want)
            assert np.all(np.abs(dev.astype(np.float64) - host.astype(np.float64)) <= slack), name
