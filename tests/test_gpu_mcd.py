"""Device MCD / DTW (vaenpvc_mcd_dtw, csrc/gfx950_dtw.hip) on one mixed batch: the continuous stages (mel-cepstra, ln f0,
cost matrix, read from the documented workspace) against the float64 restatement (tests/mcd_ref.py) within bars, the
discrete stages (DP, back-trace, path sums) exactly on the device's own cost matrix, the whole call against the full
restatement, exact ties, bit-for-bit batch invariance, and `evaluate.py` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcd_ref as R
from helpers import load_arch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'vae-npvc_amd')
# bars: about 3x the largest value measured on an MI355X on this batch; whatever is measured, none
# may exceed 1e-9 of the largest entry (more means float32 arithmetic got in somewhere)
MC_REL = 9e-15         # max |mc - ref| / max |ref| over the batch (measured 2.9e-15)
LF0_REL = 6e-16        # ln f0, relative (measured 2.0e-16)
COST_REL = 2e-15       # max |d - ref| / max |ref| per pair, the reference computed from the DEVICE's mel-cepstra
#                        (measured 5.6e-16)
E2E_REL = 5e-14        # max |d - ref| / max |ref| per pair against the restatement's own mel-cepstra (measured 1.6e-14);
#                        mcd_db's bar is this one scaled by sqrt(2) 10 / ln 10, in units of the pair's largest cost
#                        (measured 3.9e-14 against the bar's 3.1e-13)
GAP_MIN = 1e-8         # the restatement's smallest relative gap between best and second-best predecessor on a path
SEED = 15              # picked on the CPU: the smallest gap over the batch is 1.1e-6 (seeds 11 .. 23 give 2e-9 .. 1e-6)
LEN_A = [1, 3, 37, 130, 300, 64, 1100, 520, 9, 2100, 3100]
LEN_B = [6, 5, 29, 171, 260, 90, 1210, 433, 2, 40, 25]


def random_walk_side(T, rng, start=None):
    """Smooth random-walk spectra in the record form: sp [T, 513] = log10(sp / en) built from 16 cosine coefficients that
    each walk in time, en, and an f0 track with voiced and unvoiced runs."""
    k = np.arange(513) / 512.0
    c0 = rng.standard_normal(16) * 0.3 if start is None else start
    c = c0 + np.cumsum(0.05 * rng.standard_normal((T, 16)), 0)
    sp = -6.0 - 2.5 * k[None] + sum(c[:, q:q + 1] * np.cos((q + 1) * np.pi * k)[None] / (1 + 0.3 * q) for q in range(16))
    en = rng.uniform(100.0, 2000.0, T)
    f0 = np.zeros(T)
    t = 0
    while t < T:
        n = min(int(rng.integers(1, 40)), T - t)
        if rng.random() < 0.7:
            f0[t:t + n] = rng.uniform(80, 300) * (1 + 0.03 * np.sin(np.arange(n) / 5.0))
        t += n
    return sp.astype(np.float32), en.astype(np.float32), f0.astype(np.float32)


def mixed_batch(seed=SEED):
    rng = np.random.default_rng(seed)
    start = rng.standard_normal(16) * 0.3
    A = [random_walk_side(T, rng, start) for T in LEN_A]
    B = [random_walk_side(T, rng, start) for T in LEN_B]
    return A, B


def cat(side, which=None):
    idx = range(len(side)) if which is None else which
    return [torch.from_numpy(np.concatenate([side[u][q] for u in idx])).cuda() for q in range(3)]


def run(A, B, which=None, **kw):
    from hipvae import metrics
    idx = list(range(len(A))) if which is None else list(which)
    a, b = cat(A, idx), cat(B, idx)
    out = metrics.mcd_dtw(a[0], a[1], a[2], [len(A[u][1]) for u in idx], b[0], b[1], b[2], [len(B[u][1]) for u in idx],
                          **kw)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def batch():
    from hipvae import metrics
    A, B = mixed_batch()
    res, paths, D, ws = run(A, B, return_path=True, return_D=True, return_workspace=True)
    Fa, Fb = sum(LEN_A), sum(LEN_B)
    cells = sum(a * b for a, b in zip(LEN_A, LEN_B))
    lay = metrics.layout(len(LEN_A), Fa, Fb, cells, 24)
    reg = {k: metrics.region(ws, lay, k).cpu().numpy() for k in lay if k != 'bytes'}
    W = R.mcep_matrix(24, 0.42)
    ref = [R.mcd_pair(*A[u], *B[u], W=W, full=True) for u in range(len(A))]
    return dict(A=A, B=B, res=res.cpu().numpy(), paths=[p.cpu().numpy() for p in paths], D=D.cpu().numpy(), reg=reg,
                Fa=Fa, Fb=Fb, cells=cells, ref=ref, W=W)


def per_pair(b):
    """-> (u, Ta, Tb, frame offset A, frame offset B, cell offset)"""
    oa = ob = oc = 0
    for u, (Ta, Tb) in enumerate(zip(LEN_A, LEN_B)):
        yield u, Ta, Tb, oa, ob, oc
        oa, ob, oc = oa + Ta, ob + Tb, oc + Ta * Tb


def test_batch_shape():
    assert len(LEN_A) >= 8 and all(a != b for a, b in zip(LEN_A, LEN_B))
    assert 1 in LEN_A and min(max(a, b) for a, b in zip(LEN_A, LEN_B)) <= 6
    assert any(min(a, b) > 1024 for a, b in zip(LEN_A, LEN_B))            # diagonals longer than a workgroup
    assert max(LEN_A) > 3072                                              # four rows per thread in the DP kernel


def test_pair_table(batch):
    pi = batch['reg']['pinfo']
    for u, Ta, Tb, oa, ob, oc in per_pair(batch):
        assert pi[u, 0] == oc and pi[u, 2] == oa and pi[u, 3] == ob and pi[u, 4] == Ta and pi[u, 5] == Tb
    assert pi[-1, 0] == batch['cells']


def test_mcep_and_lf0_match_restatement(batch):
    mc = batch['reg']['mc']
    ref = np.concatenate([r['mcA'] for r in batch['ref']] + [r['mcB'] for r in batch['ref']])
    err = np.abs(mc - ref).max() / np.abs(ref).max()
    print('mcep rel err %.3e (bar %.1e)' % (err, MC_REL))
    assert MC_REL <= 1e-9 and err <= MC_REL
    f0 = np.concatenate([s[2] for s in batch['A']] + [s[2] for s in batch['B']])
    want = R.log_f0(f0)
    got = batch['reg']['lf0']
    assert np.array_equal(got == -1.0, want == -1.0)
    v = want >= 0
    err = (np.abs(got - want)[v] / want[v]).max()
    print('lf0 rel err %.3e (bar %.1e)' % (err, LF0_REL))
    assert err <= LF0_REL


def test_cost_matrix_matches_restatement(batch):
    mc, Fa = batch['reg']['mc'], batch['Fa']
    worst = worst_e2e = 0.0
    for u, Ta, Tb, oa, ob, oc in per_pair(batch):
        got = batch['reg']['cost'][oc:oc + Ta * Tb][R.diag_index(Ta, Tb)]
        ref = R.cost_matrix(mc[oa:oa + Ta], mc[Fa + ob:Fa + ob + Tb])       # from the device's own mel-cepstra
        worst = max(worst, np.abs(got - ref).max() / ref.max())
        full = batch['ref'][u]['cost']
        worst_e2e = max(worst_e2e, np.abs(got - full).max() / full.max())
    print('cost rel err %.3e (bar %.1e); against the full restatement %.3e (bar %.1e)' % (worst, COST_REL, worst_e2e,
                                                                                         E2E_REL))
    assert COST_REL <= 1e-9 and E2E_REL <= 1e-9
    assert worst <= COST_REL and worst_e2e <= E2E_REL


def test_dp_and_trace_exact_on_device_costs(batch):
    """The device's own cost matrix and ln f0 through the restatement's DP, back-trace and sums: D, the predecessor bytes,
    the path, P and every result field are identical (one addition and comparisons per cell; the sums run in the same
    order with one rounding per operation, sqrt and the division are correctly rounded on both sides)."""
    lf0, Fa = batch['reg']['lf0'], batch['Fa']
    for u, Ta, Tb, oa, ob, oc in per_pair(batch):
        cost = batch['reg']['cost'][oc:oc + Ta * Tb][R.diag_index(Ta, Tb)]
        D, code = R.dp(cost)
        assert np.array_equal(batch['D'][oc:oc + Ta * Tb][R.diag_index(Ta, Tb)], D), u
        assert np.array_equal(batch['reg']['code'][oc:oc + Ta * Tb][R.diag_index(Ta, Tb)], code), u
        path = R.backtrace(code)
        assert np.array_equal(batch['paths'][u], path[::-1]), u
        want = R.path_sums(cost, path, lf0[oa:oa + Ta], lf0[Fa + ob:Fa + ob + Tb], D[-1, -1])
        got = batch['res'][u]
        assert np.array_equal(got, want, equal_nan=True), (u, got, want)
        assert got[1] == len(path) and max(Ta, Tb) <= got[1] <= Ta + Tb - 1


def test_end_to_end_against_full_restatement(batch):
    """Same path and P as the restatement run on its own mel-cepstra and costs.  That only holds when no decision on the path
    is a near-tie, which is asserted (not skipped) on the restatement's side."""
    worst = 0.0
    for u, Ta, Tb, oa, ob, oc in per_pair(batch):
        ref = batch['ref'][u]
        gap = R.min_gap(ref['D'], ref['path'])
        assert gap > GAP_MIN, (u, gap)
        assert np.array_equal(batch['paths'][u], ref['path'][::-1]), u
        got, want = batch['res'][u], ref['results']
        assert got[1] == want[1] and got[4] == want[4] and got[5] == want[5], u
        scale = ref['cost'].max()
        worst = max(worst, abs(got[0] - want[0]) / scale)
        assert abs(got[0] - want[0]) <= E2E_REL * R.DB_FACTOR * scale, u
        assert abs(got[2] - want[2]) <= E2E_REL * scale * got[1], u
        if want[4] > 0:
            assert abs(got[3] - want[3]) <= 1e-12 * max(want[3], 1e-2), u    # ln f0 is within 1 ulp (9e-16) on either side
    print('mcd_db abs err / max cost %.3e (bar %.1e)' % (worst, E2E_REL * R.DB_FACTOR))


def tie_case(seed, Ta, Tb, alphabet):
    """Both sides drawn from a few distinct frames: most costs repeat exactly, so the DP meets exact ties all over."""
    rng = np.random.default_rng(seed)
    sp, en, f0 = random_walk_side(alphabet, rng)
    sp = np.round(sp * 8) / 8                                             # integer-valued spectra (in eighths)
    ia, ib = rng.integers(0, alphabet, Ta), rng.integers(0, alphabet, Tb)
    return (sp[ia], en[ia], f0[ia]), (sp[ib], en[ib], f0[ib])


def test_exact_ties():
    from hipvae import metrics
    # (a) B = A with repeated frames (all frames of A distinct): zero-cost path, against the FULL restatement
    rng = np.random.default_rng(3)
    sp, en, f0 = random_walk_side(90, rng)
    sp = np.round(sp * 8) / 8
    rep = np.repeat(np.arange(90), rng.integers(1, 4, 90))
    A, B = [(sp, en, f0)], [(sp[rep], en[rep], f0[rep])]
    res, paths = run(A, B, return_path=True)
    ref = R.mcd_pair(*A[0], *B[0], full=True)
    assert np.array_equal(paths[0].cpu().numpy(), ref['path'][::-1])
    assert np.array_equal(paths[0].cpu().numpy(), np.stack([rep, np.arange(len(rep))], 1))
    r = res.cpu().numpy()[0]
    assert r[0] == 0.0 and r[1] == len(rep) and r[2] == 0.0 and r[3] == 0.0 and r[5] == 0
    # (b) two sequences over a 5-frame alphabet: at most 25 distinct costs; the restatement's DP on the device's costs
    A, B = zip(*[tie_case(s, Ta, Tb, 5) for s, Ta, Tb in ((1, 200, 170), (2, 1300, 64), (3, 33, 47))])
    res, paths, D, ws = run(list(A), list(B), return_path=True, return_D=True, return_workspace=True)
    lens = [(len(a[1]), len(b[1])) for a, b in zip(A, B)]
    cells = sum(a * b for a, b in lens)
    lay = metrics.layout(3, sum(a for a, _ in lens), sum(b for _, b in lens), cells, 24)
    cost_all = metrics.region(ws, lay, 'cost').cpu().numpy()
    oc = 0
    for u, (Ta, Tb) in enumerate(lens):
        cost = cost_all[oc:oc + Ta * Tb][R.diag_index(Ta, Tb)]
        assert len(np.unique(cost)) <= 25
        Dr, code = R.dp(cost)
        ties = sum(1 for i in range(1, Ta) for j in range(1, Tb)
                   if len({Dr[i - 1, j - 1], Dr[i - 1, j], Dr[i, j - 1]}) < 3) if Ta * Tb < 40000 else None
        assert ties is None or ties > 50, ties
        assert np.array_equal(D.cpu().numpy()[oc:oc + Ta * Tb][R.diag_index(Ta, Tb)], Dr), u
        assert np.array_equal(paths[u].cpu().numpy(), R.backtrace(code)[::-1]), u
        oc += Ta * Tb


def test_batch_invariance(batch):
    A, B = batch['A'], batch['B']
    for u in (0, 4, 6, 10):
        res, paths = run(A, B, which=[u], return_path=True)
        assert np.array_equal(res.cpu().numpy()[0], batch['res'][u], equal_nan=True), u
        assert np.array_equal(paths[0].cpu().numpy(), batch['paths'][u]), u
    order = [7, 1, 10, 4, 0, 6, 3, 9, 5, 2, 8]
    res, paths = run(A, B, which=order, return_path=True)
    res = res.cpu().numpy()
    for j, u in enumerate(order):
        assert np.array_equal(res[j], batch['res'][u], equal_nan=True), u
        assert np.array_equal(paths[j].cpu().numpy(), batch['paths'][u]), u
    # without the optional outputs: the same results
    assert np.array_equal(run(A, B).cpu().numpy(), batch['res'], equal_nan=True)


def test_device_skips_pairs_that_break_the_contract():
    """Offsets the binding would refuse, handed to the ABI directly: the pair is skipped, its results are NaN, its
    neighbours are untouched."""
    from hipvae import lib as L
    from hipvae import metrics
    A, B = mixed_batch()
    idx = [2, 3, 5]
    a, b = cat(A, idx), cat(B, idx)
    la, lb = [LEN_A[u] for u in idx], [LEN_B[u] for u in idx]
    good = run(A, B, which=idx).cpu().numpy()
    Fa, Fb, cells = sum(la), sum(lb), sum(x * y for x, y in zip(la, lb))
    offA = torch.tensor(np.cumsum([0] + la), dtype=torch.int64).cuda()
    offB = torch.tensor([0, lb[0], lb[0], Fb], dtype=torch.int64).cuda()          # pair 1 has no frames on side B
    lib = L.load_library()
    need = lib.vaenpvc_mcd_workspace_bytes(3, Fa, Fb, cells, 24)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    W = torch.from_numpy(metrics.mcep_matrix(24, 0.42)).cuda()
    res = torch.full((3, 8), 7.0, dtype=torch.float64, device='cuda')
    L.check(lib.vaenpvc_mcd_dtw(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), offA.data_ptr(), Fa, b[0].data_ptr(),
                                b[1].data_ptr(), b[2].data_ptr(), offB.data_ptr(), Fb, 3, cells, W.data_ptr(), 24,
                                res.data_ptr(), None, None, ws.data_ptr(), need,
                                torch.cuda.current_stream().cuda_stream), 'mcd_dtw')
    torch.cuda.synchronize()
    res = res.cpu().numpy()
    assert np.array_equal(res[0], good[0], equal_nan=True) and np.all(np.isnan(res[1]))
    assert res[2][1] >= max(la[2], lb[1] + lb[2]) and np.isfinite(res[2][0])      # pair 2 now spans B's last two utterances


def write_records(path, side, spk):
    sp, en, f0 = side
    r = np.zeros((len(en), 1029), np.float32)
    r[:, :513], r[:, 513:1026], r[:, 1026], r[:, 1027], r[:, 1028] = sp, 0.5, f0, en, spk
    os.makedirs(os.path.dirname(path), exist_ok=True)
    r.tofile(path)


def test_cli_end_to_end(tmp_path):
    import evaluate as E
    from model.vae import ConvVAE
    root = str(tmp_path)
    rng = np.random.default_rng(21)
    sides = {}
    for u, (Ts, Tt) in enumerate([(60, 75), (48, 40), (90, 66)]):
        for spk, sid, T in (('SF1', 0, Ts), ('TM3', 9, Tt)):
            sp, en, f0 = random_walk_side(T, rng)
            en[[1, T // 2]] = 1e-3                                        # two silent frames per file
            sides[spk, u] = (sp, en, f0)
            write_records(os.path.join(root, 'bin', 'Testing Set', spk, '1000%02d.bin' % u), sides[spk, u], sid)
    write_records(os.path.join(root, 'bin', 'Testing Set', 'SF1', '100099.bin'), random_walk_side(20, rng), 0)
    allsp = np.concatenate([s[0] for s in sides.values()])
    etc = os.path.join(root, 'etc')
    os.makedirs(etc)
    np.percentile(allsp, 0.5, axis=0).astype(np.float32).tofile(os.path.join(etc, 'xmin.npf'))
    np.percentile(allsp, 99.5, axis=0).astype(np.float32).tofile(os.path.join(etc, 'xmax.npf'))
    np.array([5.0, 0.25], np.float32).tofile(os.path.join(etc, 'SF1.npf'))
    np.array([4.7, 0.30], np.float32).tofile(os.path.join(etc, 'TM3.npf'))
    arch = load_arch()
    logdir = os.path.join(root, 'logdir', 'train', 'stamp')
    os.makedirs(logdir)
    with open(os.path.join(logdir, 'architecture-vae-vcc2016.json'), 'w') as fp:
        json.dump(arch, fp)
    machine = ConvVAE(arch, seed=8)
    torch.save({'params': machine.engine.params.cpu(), 'step': 7}, os.path.join(logdir, 'model.ckpt-7'))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    rows_by_floor = {}
    for floor in ('40', '0'):
        out_dir = os.path.join(root, 'eval' + floor)
        r = subprocess.run([sys.executable, os.path.join(PKG, 'evaluate.py'), '--src', 'SF1', '--trg', 'TM3', '--model',
                            'ConvVAE', '--checkpoint', os.path.join(logdir, 'model.ckpt-7'), '--output_dir', out_dir,
                            '--file_pattern', os.path.join(root, 'bin', 'Testing Set', '{}', '*.bin'),
                            '--energy_floor_db', floor], capture_output=True, text=True, env=env, cwd=root, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert 'No partner: ' + os.path.join(root, 'bin', 'Testing Set', 'SF1', '100099.bin') in r.stdout
        lines = [ln.rstrip('\n').split('\t') for ln in open(os.path.join(out_dir, 'mcd-SF1-TM3.tsv'))]
        assert tuple(lines[0]) == E.COLUMNS
        rows = lines[1:]
        assert [x[0] for x in rows] == ['100000', '100001', '100002', 'MEAN_WEIGHTED_BY_PATH', 'MEAN']
        rows_by_floor[floor] = rows
        col = {c: i for i, c in enumerate(lines[0])}
        A, B = [], []
        for u in range(3):
            s, t = sides['SF1', u], sides['TM3', u]
            ks, kt = E.energy_keep(s[1], float(floor)), E.energy_keep(t[1], float(floor))
            drop = 2 if floor == '40' else 0
            assert ks.sum() == len(s[1]) - drop and kt.sum() == len(t[1]) - drop
            assert int(rows[u][col['src_frames']]) == ks.sum() and int(rows[u][col['trg_frames']]) == kt.sum()
            A.append(tuple(q[ks] for q in s))
            B.append(tuple(q[kt] for q in t))
        direct = run(A, B).cpu().numpy()
        for u in range(3):
            assert rows[u][col['mcd_src_db']] == '%.6f' % direct[u, 0]
            assert int(rows[u][col['path_src']]) == direct[u, 1]
            conv = float(rows[u][col['mcd_conv_db']])
            assert np.isfinite(conv) and conv > 0 and int(rows[u][col['path_conv']]) >= max(len(A[u][1]), len(B[u][1]))
        w = (direct[:, 0] * direct[:, 1]).sum() / direct[:, 1].sum()
        assert abs(float(rows[3][col['mcd_src_db']]) - w) < 2e-6
    assert [r[1] for r in rows_by_floor['0'][:3]] == ['60', '48', '90']
    assert [r[1] for r in rows_by_floor['40'][:3]] == ['58', '46', '88']
