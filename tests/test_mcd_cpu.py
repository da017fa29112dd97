"""DTW-aligned mel-cepstral distortion without a GPU: the float64 restatement (tests/mcd_ref.py) against ground truth, the
library's host-side matrix and argument checks, and evaluate.py's host logic with the device call replaced by the
restatement."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mcd_ref as R
from hipvae import lib as L
from hipvae import metrics

E_ARG, E_WS = -1, -2
OMEGA = np.pi * np.arange(513) / 512.0


def warped_series(a, alpha):
    return sum(a[m] * np.cos(m * R.warp(OMEGA, alpha)) for m in range(len(a)))


def records(L_amp, en=None):
    """(sp, en) float64 with log_amplitude(sp, en) == L_amp up to rounding."""
    en = np.ones(L_amp.shape[0]) if en is None else np.asarray(en, np.float64)
    return (2.0 * L_amp - np.log(en)[:, None]) / np.log(10.0), en


def distinct_frames(T, seed, order=24, alpha=0.42):
    """T log-amplitude frames with well separated mel-cepstra (a random warped cosine series each)."""
    rng = np.random.default_rng(seed)
    return np.stack([warped_series(rng.standard_normal(order + 1), alpha) for _ in range(T)])


def test_restatement_recovers_a_warped_cosine_series():
    a = np.random.default_rng(0).standard_normal(25)
    W = R.mcep_matrix(24, 0.42)
    assert np.abs(W @ warped_series(a, 0.42) - a).max() <= 1e-13
    assert np.linalg.cond(W) < 3.0
    # alpha = 0: plain cepstrum truncation
    assert np.abs(R.mcep_matrix(24, 0.0) @ warped_series(a, 0.0) - a).max() <= 1e-13


def test_db_factor_from_first_principles():
    """alpha = 0, one frame against one frame, LA - LB = sum a_m cos(m omega): mcd_db = (10 / ln 10) sqrt(2 sum a_m^2), which
    is the RMS difference of the two spectra in dB (20 log10 amplitude) over the 1024-point circle."""
    rng = np.random.default_rng(1)
    a = np.concatenate([[0.0], 0.1 * rng.standard_normal(24)])
    LB = warped_series(rng.standard_normal(25), 0.0)[None]
    LA = LB + warped_series(a, 0.0)[None]
    (spA, enA), (spB, enB) = records(LA), records(LB)
    res = R.mcd_pair(spA, enA, [0.0], spB, enB, [0.0], order=24, alpha=0.0)
    want = 10.0 / np.log(10.0) * np.sqrt(2.0 * (a[1:] ** 2).sum())
    assert abs(res[0] - want) <= 1e-12 * want
    assert res[1] == 1 and res[2] == res[6]
    assert abs(R.DB_FACTOR - 10.0 * np.sqrt(2.0) / np.log(10.0)) <= 1e-15
    db = 20.0 / np.log(10.0) * (LA - LB)[0]                       # amplitude difference in dB per bin
    circle = np.concatenate([db, db[-2:0:-1]])                   # the 1024-point symmetric extension
    assert len(circle) == 1024
    assert abs(np.sqrt((circle ** 2).mean()) - want) <= 1e-12 * want


def test_identical_and_doubled_sequences():
    LA = distinct_frames(12, 2)
    sp, en = records(LA, en=np.linspace(50.0, 900.0, 12))
    f0 = np.where(np.arange(12) % 3 == 0, 0.0, 120.0 + np.arange(12))
    full = R.mcd_pair(sp, en, f0, sp, en, f0, full=True)
    assert full['results'][0] == 0.0 and full['results'][1] == 12
    assert np.array_equal(full['path'][::-1], np.stack([np.arange(12)] * 2, 1))
    assert full['results'][3] == 0.0 and full['results'][4] == 8 and full['results'][5] == 0
    idx = np.repeat(np.arange(12), 2)
    full = R.mcd_pair(sp, en, f0, sp[idx], en[idx], f0[idx], full=True)
    assert full['results'][0] == 0.0 and full['results'][1] == 24
    assert np.array_equal(full['path'][::-1], np.stack([idx, np.arange(24)], 1))


def test_constant_gain_changes_nothing():
    LA, LB = distinct_frames(9, 3), distinct_frames(11, 4)
    (spA, enA), (spB, enB) = records(LA), records(LB)
    f0A, f0B = np.full(9, 100.0), np.full(11, 140.0)
    r0 = R.mcd_pair(spA, enA, f0A, spB, enB, f0B, full=True)
    r1 = R.mcd_pair(spA, 7.5 * enA, f0A, spB, enB, f0B, full=True)
    assert np.array_equal(r0['path'], r1['path'])
    assert abs(r0['results'][0] - r1['results'][0]) <= 1e-10 * r0['results'][0]
    assert np.abs(r0['mcA'][:, 0] - r1['mcA'][:, 0]).min() > 0.1          # the gain went into the coefficient left out


def test_known_monotone_warp_is_recovered():
    Ta = 15
    LA = distinct_frames(Ta, 5)
    rng = np.random.default_rng(6)
    steps = np.concatenate([np.ones(Ta - 1, int), np.zeros(10, int)])
    rng.shuffle(steps)
    w = np.concatenate([[0], np.cumsum(steps)])                           # monotone, steps of 0 or 1, onto 0 .. Ta-1
    sp, en = records(LA)
    full = R.mcd_pair(sp, en, np.zeros(Ta), sp[w], en[w], np.zeros(len(w)), full=True)
    assert full['results'][0] == 0.0 and full['results'][1] == len(w)
    assert np.array_equal(full['path'][::-1], np.stack([w, np.arange(len(w))], 1))


def test_tie_order_on_a_hand_made_matrix():
    """On equal values: the diagonal, then (i-1, j), then (i, j-1)."""
    cost = np.ones((3, 3))
    D, code = R.dp(cost)
    assert np.array_equal(D, [[1, 2, 3], [2, 2, 3], [3, 3, 3]])
    assert np.array_equal(code, [[0, 2, 2], [1, 0, 0], [1, 0, 0]])       # (1, 1): all three equal -> the diagonal
    assert np.array_equal(R.backtrace(code), [[2, 2], [1, 1], [0, 0]])
    cost = np.array([[1.0, 1.0, 9.0], [1.0, 9.0, 1.0], [9.0, 1.0, 1.0]])
    D, code = R.dp(cost)
    # (1, 1): diagonal 1, up 2, left 2 -> diagonal; (1, 2): diag 2, up 11, left 10 -> diagonal;
    # (2, 2): diag D(1,1) = 10, up D(1,2) = 3, left D(2,1) = 3 -> the tie goes to (i-1, j)
    assert D[1, 2] == 3 and D[2, 1] == 3 and D[2, 2] == 4
    assert code[2, 2] == 1 and code[1, 2] == 0 and code[2, 1] == 0
    assert np.array_equal(R.backtrace(code), [[2, 2], [1, 2], [0, 1], [0, 0]])
    # up strictly smaller than left
    cost = np.array([[1.0, 5.0], [2.0, 1.0]])
    D, code = R.dp(cost)
    assert code[1, 1] == 0 and D[1, 1] == 2


def test_path_sums_on_a_hand_made_path():
    cost = np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5
    path = np.array([[2, 3], [2, 2], [1, 1], [0, 1], [0, 0]], np.int32)
    f0A = np.array([100.0, 0.0, 200.0], np.float32)
    f0B = np.array([0.5, 110.0, 0.0, 220.0], np.float32)                # 0.5 <= 1: unvoiced
    lfA, lfB = R.log_f0(f0A), R.log_f0(f0B)
    assert lfA[1] == -1.0 and lfB[0] == -1.0 and lfB[2] == -1.0
    res = R.path_sums(cost, path, lfA, lfB, D_end=42.0)
    s = 11.5 + 10.5 + 5.5 + 1.5 + 0.5
    assert res[6] == s and res[1] == 5 and res[2] == 42.0 and res[0] == R.DB_FACTOR * s / 5
    # voiced on both sides: (2, 3) and (0, 1); one side only: (2, 2), (1, 1), (0, 0)
    e = [np.log(200.0) - np.log(220.0), np.log(100.0) - np.log(110.0)]
    assert res[4] == 2 and res[5] == 3
    assert abs(res[3] - np.sqrt((e[0] ** 2 + e[1] ** 2) / 2)) <= 1e-15
    assert np.isnan(R.path_sums(cost, path[2:3], lfA, lfB)[3])          # no voiced cell: NaN


@pytest.mark.parametrize('order,alpha', [(24, 0.42), (24, 0.0), (40, 0.55), (1, 0.3), (64, 0.8)])
def test_library_matrix_matches_restatement(order, alpha):
    """Both run a float64 recursion of 513 steps with gain <= (1 + alpha) / (1 - alpha): about 513 * 2.4 * 1.1e-16 = 1.4e-13
    of the largest entry at alpha = 0.42; the bar is 1e-12 * max |W| for a different but valid operation order."""
    W, ref = metrics.mcep_matrix(order, alpha), R.mcep_matrix(order, alpha)
    assert W.shape == (order + 1, 513) and W.dtype == np.float64
    assert np.abs(W - ref).max() <= 1e-12 * np.abs(ref).max()
    if alpha < 0.6:
        a = np.random.default_rng(order).standard_normal(order + 1)
        assert np.abs(W @ warped_series(a, alpha) - a).max() <= 1e-13


def test_mcep_matrix_rejections():
    lib = L.load_library()
    buf = np.empty((65, 513))
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.vaenpvc_mcep_matrix(24, 0.42, 513, p) == 0
    for order, alpha, H, ptr in ((0, 0.42, 513, p), (65, 0.42, 513, p), (-1, 0.42, 513, p), (24, 1.0, 513, p),
                                 (24, -0.1, 513, p), (24, float('nan'), 513, p), (24, 0.42, 512, p), (24, 0.42, 1025, p),
                                 (24, 0.42, 513, None)):
        assert lib.vaenpvc_mcep_matrix(order, alpha, H, ptr) == E_ARG, (order, alpha, H)
    for order, alpha in ((0, 0.42), (65, 0.42), (24, 1.0), (24, -0.5), (24, float('inf'))):
        with pytest.raises(ValueError):
            metrics.mcep_matrix(order, alpha)


def test_mcd_workspace_formula_and_rejections():
    lib = L.load_library()
    ok = (3, 700, 650, 151000, 24)
    lay = metrics.layout(*ok)
    assert lib.vaenpvc_mcd_workspace_bytes(*ok) == lay['bytes']
    a256 = lambda b: (b + 255) // 256 * 256                                # noqa: E731
    assert lay['bytes'] == a256(1350 * 25 * 8) + a256(1350 * 8) + a256(4 * 6 * 8) + a256(151000 * 8) + a256(151000)
    assert [lay[k][0] % 256 for k in ('mc', 'lf0', 'pinfo', 'cost', 'code')] == [0] * 5
    # a large call: the cell count needs 64 bits
    big = (54, 54 * 4096, 54 * 4096, 54 * 4096 * 4096, 24)
    assert lib.vaenpvc_mcd_workspace_bytes(*big) == metrics.layout(*big)['bytes'] > 9 * 54 * 4096 * 4096
    mx = 4096
    for i, v in ((0, 0), (0, -1), (0, 65537), (1, 2), (1, 3 * mx + 1), (2, 0), (2, 3 * mx + 1), (3, 699), (3, 700 * 650 + 1),
                 (3, 0), (3, -5), (4, 0), (4, 65), (4, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.vaenpvc_mcd_workspace_bytes(*bad) == E_ARG, (i, v)
    assert lib.vaenpvc_mcd_workspace_bytes(1, mx, mx, mx * mx, 64) > 0     # the stated maximum is accepted
    assert lib.vaenpvc_mcd_workspace_bytes(1, mx + 1, mx, mx * mx, 24) == E_ARG
    assert lib.vaenpvc_mcd_workspace_bytes(2, 2 * mx, 2 * mx, 2 * mx * mx + 1, 24) == E_ARG


def test_mcd_dtw_argument_checks_without_device():
    lib = L.load_library()
    n, Fa, Fb, cells, order = 3, 700, 650, 151000, 24
    need = lib.vaenpvc_mcd_workspace_bytes(n, Fa, Fb, cells, order)
    # fake device addresses, far apart and aligned: every rejection happens before a launch
    names = ('spA', 'enA', 'f0A', 'oA', 'spB', 'enB', 'f0B', 'oB', 'W', 'res', 'path', 'D', 'ws')
    base = {k: (i + 1) << 32 for i, k in enumerate(names)}

    def call(**kw):
        a = dict(base, n=n, Fa=Fa, Fb=Fb, cells=cells, order=order, nb=need)
        a.update(kw)
        return lib.vaenpvc_mcd_dtw(a['spA'], a['enA'], a['f0A'], a['oA'], a['Fa'], a['spB'], a['enB'], a['f0B'], a['oB'],
                                   a['Fb'], a['n'], a['cells'], a['W'], a['order'], a['res'], a['path'], a['D'], a['ws'],
                                   a['nb'], None)
    for kw in ({'n': 0}, {'n': -3}, {'n': 65537}, {'Fa': 2}, {'Fb': 2}, {'Fa': 3 * 4096 + 1}, {'Fb': 3 * 4096 + 1},
               {'cells': 699}, {'cells': Fa * Fb + 1}, {'cells': 0}, {'order': 0}, {'order': 65},
               {'spA': None}, {'enA': None}, {'f0A': None}, {'oA': None}, {'spB': None}, {'enB': None}, {'f0B': None},
               {'oB': None}, {'W': None}, {'res': None},
               {'res': base['spA']}, {'path': base['W']}, {'D': base['oB']}, {'path': base['res']}, {'D': base['ws']},
               {'res': base['ws'] + 256}, {'ws': base['ws'] + 16}):
        assert call(**kw) == E_ARG, kw
    for kw in ({'ws': None}, {'nb': need - 1}, {'nb': 0}):
        assert call(**kw) == E_WS, kw
    assert b'workspace' in lib.vaenpvc_last_error()


def test_diagonal_layout():
    """cost, code and D are stored anti-diagonal after anti-diagonal; the binding's closed form against the definition."""
    assert np.array_equal(R.diag_index(2, 3), [[0, 1, 3], [2, 4, 5]])
    for Ta, Tb in ((1, 1), (1, 7), (7, 1), (5, 5), (3, 9), (9, 3), (64, 33), (33, 64), (130, 171)):
        idx = metrics.diag_index(Ta, Tb)
        assert idx.dtype == np.int64 and np.array_equal(idx, R.diag_index(Ta, Tb)), (Ta, Tb)
        assert np.array_equal(np.sort(idx.ravel()), np.arange(Ta * Tb))


def test_binding_host_checks():
    for la, lb in (([], []), ([5], [5, 6]), ([0], [4]), ([4], [0]), ([4097], [10]), ([10], [4097]), ([3, -1], [2, 2])):
        with pytest.raises(ValueError):
            metrics.check_args(la, lb)
    for order, alpha in ((0, 0.42), (65, 0.42), (24, 1.0), (24, -0.01), (24, float('nan'))):
        with pytest.raises(ValueError):
            metrics.check_args([5], [6], order, alpha)
    assert metrics.check_args([5, 4096], [7, 1], 24, 0) == ([5, 4096], [7, 1], 24, 0.0, 35 + 4096)
    sp = torch.zeros(5, 513)
    with pytest.raises(TypeError):                                       # host tensors are refused, not copied
        metrics.mcd_dtw(sp, torch.ones(5), torch.zeros(5), [5], sp, torch.ones(5), torch.zeros(5), [5])


# ---- evaluate.py host logic, the device call replaced by the restatement -------------------------------------------------

def fake_mcd_dtw(calls):
    def f(spA, enA, f0A, lengthsA, spB, enB, f0B, lengthsB, order=24, alpha=0.42, **kw):
        calls.append((list(lengthsA), list(lengthsB), order, alpha))
        n = lambda t: t.cpu().numpy()                                      # noqa: E731
        return torch.from_numpy(R.mcd_batch(n(spA), n(enA), n(f0A), lengthsA, n(spB), n(enB), n(f0B), lengthsB,
                                            order=order, alpha=alpha))
    return f


def write_bin(path, T, seed, spk, quiet=()):
    rng = np.random.default_rng(seed)
    k = np.arange(513) / 513.0
    r = np.zeros((T, 1029), np.float32)
    walk = np.cumsum(0.05 * rng.standard_normal((T, 4)), 0)
    r[:, :513] = -6.0 - 2.5 * k + sum(walk[:, q:q + 1] * np.cos((q + 1) * np.pi * k) for q in range(4))
    r[:, 513:1026] = 0.5
    r[:, 1026] = np.where(rng.random(T) > 0.3, rng.uniform(90, 250, T), 0.0)
    r[:, 1027] = rng.uniform(500.0, 1500.0, T)
    for t in quiet:
        r[t, 1027] = 1e-3                                                 # > 50 dB under the rest
    r[:, 1028] = spk
    os.makedirs(os.path.dirname(path), exist_ok=True)
    r.tofile(path)
    return r


@pytest.fixture
def corpus(tmp_path):
    root = str(tmp_path)
    recs = {}
    for u, (Ts, Tt) in enumerate([(14, 11), (9, 13), (12, 12)]):
        recs['SF1', u] = write_bin(os.path.join(root, 'bin', 'SF1', '1000%d.bin' % u), Ts, 10 + u, 0, quiet=(0, 5))
        recs['TM3', u] = write_bin(os.path.join(root, 'bin', 'TM3', '1000%d.bin' % u), Tt, 20 + u, 9, quiet=(2,))
    write_bin(os.path.join(root, 'bin', 'SF1', '20000.bin'), 5, 1, 0)      # no partner
    write_bin(os.path.join(root, 'bin', 'TM3', '30000.bin'), 5, 2, 9)      # no partner
    write_bin(os.path.join(root, 'bin', 'TM3', '30001.bin'), 5, 3, 9)
    return root, recs


def read_tsv(path):
    lines = [ln.rstrip('\n').split('\t') for ln in open(path)]
    return lines[0], lines[1:]


def test_evaluate_pairing_and_energy_floor():
    import evaluate as E
    pairs, only_s, only_t = E.pair_files(['/a/SF1/2.bin', '/a/SF1/1.bin', '/a/SF1/9.bin'], ['/b/TM3/1.bin', '/b/TM3/2.bin',
                                                                                            '/b/TM3/7.bin'])
    assert pairs == [('1', '/a/SF1/1.bin', '/b/TM3/1.bin'), ('2', '/a/SF1/2.bin', '/b/TM3/2.bin')]
    assert only_s == ['/a/SF1/9.bin'] and only_t == ['/b/TM3/7.bin']
    en = np.array([1000.0, 0.1001, 0.0999, 1000.0 * 10 ** -3.9, 5.0], np.float32)
    assert E.energy_keep(en, 40.0).tolist() == [True, True, False, True, True]
    assert E.energy_keep(en, 20.0).tolist() == [True, False, False, False, False]
    assert E.energy_keep(en, 0.0).all() and E.energy_keep(en, -3.0).all()


@pytest.mark.parametrize('floor_db', [40.0, 0.0])
def test_evaluate_model_free_report(corpus, monkeypatch, capsys, floor_db):
    import evaluate as E
    root, recs = corpus
    calls = []
    monkeypatch.setattr(metrics, 'mcd_dtw', fake_mcd_dtw(calls))
    monkeypatch.setattr(E, 'default_device', lambda: 'cpu')
    out = E.main(['--src', 'SF1', '--trg', 'TM3', '--file_pattern', os.path.join(root, 'bin', '{}', '*.bin'),
                  '--output_dir', os.path.join(root, 'out'), '--energy_floor_db', str(floor_db), '--batch_frames', '25',
                  '--order', '20', '--alpha', '0.4'])
    assert out == os.path.join(root, 'out', 'mcd-SF1-TM3.tsv')
    text = capsys.readouterr().out
    assert '3 pairs; 1 source and 2 target files without a partner' in text
    for name in ('20000.bin', '30000.bin', '30001.bin'):
        assert 'No partner: ' + os.path.join(root, 'bin', 'SF1' if name[0] == '2' else 'TM3', name) in text
    drop_s, drop_t = (2, 1) if floor_db > 0 else (0, 0)
    # --batch_frames 25 counts source frames before the floor: 14 + 9 | 12
    assert calls == [([14 - drop_s, 9 - drop_s], [11 - drop_t, 13 - drop_t], 20, 0.4), ([12 - drop_s], [12 - drop_t], 20, 0.4)]
    head, rows = read_tsv(out)
    assert tuple(head) == E.COLUMNS
    assert [r[0] for r in rows] == ['10000', '10001', '10002', 'MEAN_WEIGHTED_BY_PATH', 'MEAN']
    col = {c: i for i, c in enumerate(head)}
    want = []
    for u in range(3):
        s, t = recs['SF1', u], recs['TM3', u]
        ks, kt = E.energy_keep(s[:, 1027], floor_db), E.energy_keep(t[:, 1027], floor_db)
        assert ks.sum() == len(s) - drop_s and kt.sum() == len(t) - drop_t
        res = R.mcd_pair(s[ks, :513], s[ks, 1027], s[ks, 1026], t[kt, :513], t[kt, 1027], t[kt, 1026], order=20, alpha=0.4)
        want.append(res)
        r = rows[u]
        assert int(r[col['src_frames']]) == ks.sum() and int(r[col['trg_frames']]) == kt.sum()
        assert int(r[col['path_src']]) == res[1]
        assert abs(float(r[col['mcd_src_db']]) - res[0]) < 1e-6
        assert abs(float(r[col['voicing_mismatch_src']]) - res[5] / res[1]) < 1e-6
        if res[4] > 0:
            assert abs(float(r[col['lf0_rmse_src']]) - res[3]) < 1e-6
        # model-free: the converted columns are empty
        assert r[col['mcd_conv_db']] == 'nan' and r[col['path_conv']] == 'nan' and r[col['lf0_rmse_conv']] == 'nan'
    want = np.array(want)
    weighted = (want[:, 0] * want[:, 1]).sum() / want[:, 1].sum()
    assert abs(float(rows[3][col['mcd_src_db']]) - weighted) < 1e-6
    assert abs(float(rows[4][col['mcd_src_db']]) - want[:, 0].mean()) < 1e-6
    assert abs(weighted - R.DB_FACTOR * want[:, 6].sum() / want[:, 1].sum()) < 1e-9
    assert abs(float(rows[4][col['path_src']]) - want[:, 1].mean()) < 1e-6
    assert rows[3][col['mcd_conv_db']] == 'nan'
    assert 'source vs target' in text and '%.6f' % weighted in text


def test_evaluate_group_with_a_conversion(corpus, monkeypatch):
    """The converted side: convert_fn's tensors are filtered with the SOURCE's energy mask, f0 goes through f0_fn, en is the
    source's; both comparisons land in the row."""
    import evaluate as E
    root, recs = corpus
    calls = []
    monkeypatch.setattr(metrics, 'mcd_dtw', fake_mcd_dtw(calls))
    group = []
    for u in range(2):
        s = E.read_features(os.path.join(root, 'bin', 'SF1', '1000%d.bin' % u))
        t = E.read_features(os.path.join(root, 'bin', 'TM3', '1000%d.bin' % u))
        group.append(('1000%d' % u, s, t))
    shift = lambda sps: [torch.from_numpy(np.ascontiguousarray(sp[:, ::-1] * 1.0)) for sp in sps]      # noqa: E731
    rows = E.evaluate_group(group, 'cpu', floor_db=40.0, convert_fn=shift, f0_fn=lambda f0: f0 * 2.0)
    assert [c[:2] for c in calls] == [([12, 7], [10, 12])] * 2
    for u, row in enumerate(rows):
        s, t = recs['SF1', u], recs['TM3', u]
        ks, kt = E.energy_keep(s[:, 1027], 40.0), E.energy_keep(t[:, 1027], 40.0)
        conv = R.mcd_pair(s[ks, :513][:, ::-1], s[ks, 1027], 2.0 * s[ks, 1026], t[kt, :513], t[kt, 1027], t[kt, 1026])
        base = R.mcd_pair(s[ks, :513], s[ks, 1027], s[ks, 1026], t[kt, :513], t[kt, 1027], t[kt, 1026])
        assert row['mcd_conv_db'] == conv[0] and row['path_conv'] == conv[1] and row['mcd_src_db'] == base[0]
        assert row['voicing_mismatch_conv'] == conv[5] / conv[1]
        assert row['lf0_rmse_conv'] == conv[3] or (np.isnan(conv[3]) and np.isnan(row['lf0_rmse_conv']))
        assert row['mcd_conv_db'] != row['mcd_src_db']
    w, m = E.mean_rows(rows)
    assert abs(w['mcd_conv_db'] - sum(r['mcd_conv_db'] * r['path_conv'] for r in rows) / sum(r['path_conv'] for r in rows)) < 1e-12
    assert abs(m['mcd_conv_db'] - np.mean([r['mcd_conv_db'] for r in rows])) < 1e-12


def test_evaluate_flags():
    import evaluate as E
    a = E.parse_args(['--src', 'SF2', '--trg', 'TF1'])
    assert (a.order, a.alpha, a.energy_floor_db, a.batch_frames, a.gv, a.checkpoint, a.trg_pattern) == \
        (24, 0.42, 40.0, 16384, False, None, None)
    with pytest.raises(ValueError):
        E.parse_args(['--checkpoint', 'x/model.ckpt-1'])
    with pytest.raises(ValueError):
        E.main(['--file_pattern', '/nonexistent/{}/*.bin'])
