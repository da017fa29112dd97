"""Device statistics builder, host side: the exports and argument checks of vaenpvc_column_select / vaenpvc_speaker_stats
(none of which touch a device), the `--device` flag of build.py, the host path's independence of torch, and the float64
restatement (tests/stats_ref.py) against NumPy and against the host build.py."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import stats_ref
from helpers import PKG
from hipvae import lib as L

E_ARG, E_WS = -1, -2


def load_build():
    spec = importlib.util.spec_from_file_location('vaenpvc_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stats_symbols_exported():
    lib = L.load_library()
    assert lib.vaenpvc_abi_version() == L.ABI_VERSION == 4
    for n in ('vaenpvc_column_select_workspace_bytes', 'vaenpvc_column_select', 'vaenpvc_speaker_stats_workspace_bytes',
              'vaenpvc_speaker_stats'):
        assert hasattr(lib, n) and n in L.SIGNATURES


def test_column_select_argument_checks_without_device():
    lib = L.load_library()
    F, H, ld, n = 1000, 513, 1029, 4
    need = lib.vaenpvc_column_select_workspace_bytes(F, H, n)
    assert need >= n * H * 256 * 4                                       # the digit histograms of every rank
    assert lib.vaenpvc_column_select_workspace_bytes((1 << 31) - 1, H, 8) > 0
    for bad in ((0, H, n), (-1, H, n), (1 << 31, H, n), (F, 0, n), (F, -1, n), (F, H, 0), (F, H, 9), (F, H, -1)):
        assert lib.vaenpvc_column_select_workspace_bytes(*bad) == E_ARG, bad
    # fake device addresses: every rejection happens before a launch
    x, out, flag, ws = 1 << 20, 64 << 20, 96 << 20, 128 << 20

    def call(ranks=(0, 4, 994, 999), **kw):
        a = dict(x=x, F=F, H=H, ld=ld, n=len(ranks), out=out, flag=flag, ws=ws, nb=need)
        a.update(kw)
        host = (C.c_int64 * max(len(ranks), 1))(*ranks)
        rk = None if kw.get('no_ranks') else C.cast(host, C.c_void_p)
        return lib.vaenpvc_column_select(a['x'], a['F'], a['H'], a['ld'], rk, a['n'], a['out'], a['flag'], a['ws'],
                                         a['nb'], None)
    for kw in ({'x': None}, {'out': None}, {'flag': None}, {'no_ranks': True}, {'F': -1}, {'F': 0}, {'H': 0}, {'H': -3},
               {'ld': H - 1}, {'ld': 0}, {'n': 0}, {'n': 9}, {'n': -1}):
        assert call(**kw) == E_ARG, kw
        assert lib.vaenpvc_last_error()
    for ranks in ((-1, 0), (0, F), (5, 1 << 40), (F,)):
        assert call(ranks=ranks) == E_ARG, ranks
        assert b'rank' in lib.vaenpvc_last_error()
    assert call(ranks=tuple(range(8)), nb=lib.vaenpvc_column_select_workspace_bytes(F, H, 8) - 1) == E_WS
    assert call(nb=need - 1) == E_WS
    assert b'workspace too small' in lib.vaenpvc_last_error()
    assert call(ws=None) == E_WS
    assert call(ws=ws + 4) == E_ARG                                       # workspace alignment
    assert b'aligned' in lib.vaenpvc_last_error()


def test_speaker_stats_argument_checks_without_device():
    lib = L.load_library()
    F, H, n_seg, n_spk = 1000, 513, 5, 10
    need = lib.vaenpvc_speaker_stats_workspace_bytes(F, n_seg, H)
    assert need >= n_seg * H * 8
    for bad in ((-1, n_seg, H), (F, 0, H), (F, -1, H), (F, n_seg, 0), (F, n_seg, -2)):
        assert lib.vaenpvc_speaker_stats_workspace_bytes(*bad) == E_ARG, bad
    sp, f0, off, spk, lf0, gv, nu, ws = (k << 20 for k in (1, 32, 40, 41, 42, 43, 44, 128))

    def call(**kw):
        a = dict(sp=sp, ld=1029, f0=f0, ldf=1029, off=off, spk=spk, n_seg=n_seg, n_spk=n_spk, F=F, H=H, lf0=lf0, gv=gv,
                 nu=nu, ws=ws, nb=need)
        a.update(kw)
        return lib.vaenpvc_speaker_stats(a['sp'], a['ld'], a['f0'], a['ldf'], a['off'], a['spk'], a['n_seg'], a['n_spk'],
                                         a['F'], a['H'], a['lf0'], a['gv'], a['nu'], a['ws'], a['nb'], None)
    for kw in ({'sp': None}, {'f0': None}, {'off': None}, {'spk': None}, {'lf0': None}, {'gv': None}, {'nu': None},
               {'F': -1}, {'H': 0}, {'n_seg': 0}, {'n_seg': -1}, {'n_spk': 0}, {'ld': H - 1}, {'ldf': 0}):
        assert call(**kw) == E_ARG, kw
        assert lib.vaenpvc_last_error()
    assert call(nb=need - 1) == E_WS
    assert b'workspace too small' in lib.vaenpvc_last_error()
    assert call(ws=None) == E_WS
    assert call(ws=ws + 8) == E_ARG


def test_build_device_flag_defaults_off():
    b = load_build()
    assert b.parse_args([]).device is False
    assert b.parse_args(['--device']).device is True
    assert b.parse_args(['--device', '--train_file_pattern', 'x/*.bin']).train_file_pattern == 'x/*.bin'


def test_host_build_imports_neither_torch_nor_the_library(tmp_path):
    """In a fresh interpreter: build.main without --device leaves torch and hipvae out of sys.modules."""
    rng = np.random.default_rng(1)
    for spk, sid, n in (('SF1', 0, 12), ('TM3', 9, 7)):
        d = tmp_path / 'bin' / 'Training Set' / spk
        d.mkdir(parents=True)
        r = rng.standard_normal((n, 1029)).astype(np.float32)
        r[:, 1026] = rng.uniform(80, 300, n)
        r[:, -1] = sid
        r.tofile(str(d / '100000.bin'))
    code = ('import importlib.util, sys\n'
            'spec = importlib.util.spec_from_file_location("vaenpvc_build", sys.argv[1])\n'
            'mod = importlib.util.module_from_spec(spec)\n'
            'spec.loader.exec_module(mod)\n'
            'mod.main(["--train_file_pattern", sys.argv[2]])\n'
            'bad = sorted(n for n in sys.modules if n.split(".")[0] in ("torch", "hipvae", "analyzer"))\n'
            'print("LOADED", bad)\n'
            'sys.exit(3 if bad else 0)\n')
    r = subprocess.run([sys.executable, '-c', code, os.path.join(PKG, 'build.py'),
                        str(tmp_path / 'bin' / 'Training Set' / '*' / '*.bin')], cwd=str(tmp_path), capture_output=True,
                       text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'LOADED []' in r.stdout
    assert sorted(os.listdir(str(tmp_path / 'etc'))) == ['SF1.npf', 'SF1_gv.npf', 'TM3.npf', 'TM3_gv.npf', 'xmax.npf',
                                                         'xmin.npf']


@pytest.mark.parametrize('F', [1, 2, 3, 7, 200, 201, 202, 401, 4099])
def test_restated_percentiles_match_numpy_float64(F):
    rng = np.random.default_rng(F)
    x = (3 * rng.standard_normal((F, 23)) - 8).astype(np.float32)
    x[:, 5] = np.round(x[:, 5])                                          # ties
    x[:, 6] = -4.25
    qs = [0.5, 99.5, 0.0, 100.0, 50.0, 37.3]
    got = stats_ref.percentiles(x, qs)
    assert got.dtype == np.float32 and got.shape == (len(qs), 23)
    x64 = x.astype(np.float64)
    for k, q in enumerate(qs):
        want = np.percentile(x64, q, axis=0)
        assert stats_ref.within_ulp32(got[k], want), (F, q, np.abs(got[k] - want).max())
        assert stats_ref.within_ulp32(got[k], want.astype(np.float32).astype(np.float64)), (F, q)
    assert np.array_equal(stats_ref.order_stats(x, [0, F - 1, 0]), np.stack([x.min(axis=0), x.max(axis=0), x.min(axis=0)]))


def test_restated_speaker_stats(tmp_path, monkeypatch):
    """The restatement reproduces the host build.py's GV bytes; the distance of the host's float32 log-F0 statistics
    from it is printed: the end-to-end GPU test allows the device that distance plus one float32 ulp."""
    pattern, utts = stats_ref.write_e2e_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    load_build().main(['--train_file_pattern', pattern])
    ref = stats_ref.e2e_restatement(utts)
    etc = str(tmp_path / 'etc')
    assert sorted(os.listdir(etc)) == sorted(k for k in ref if k.endswith('.npf'))
    for name in sorted(ref):
        if name.endswith('_gv.npf'):
            got = np.fromfile(os.path.join(etc, name), np.float32)
            assert np.array_equal(got, ref[name].astype(np.float32)), name
    for spk in utts:
        host = np.fromfile(os.path.join(etc, spk + '.npf'), np.float32)
        want = ref[spk + '.npf']
        dist = np.abs(host.astype(np.float64) - want)
        print('%s.npf host float32 %s, float64 restatement %s, distance %s = %s float32 ulp'
              % (spk, host, want, dist, dist / stats_ref.ulp32(want)))
        # float32 logs (half an ulp of ~5.5 each) and float32 pairwise sums: a few ulp of ln f0 ~ 5e-7; 1e-5 is 20 of them
        assert np.all(dist < 1e-5), (spk, dist)
    # count, NaN and n_utt conventions on a layout with an absent speaker, a 1-frame one and an unvoiced one
    sp = np.arange(24, dtype=np.float32).reshape(8, 3) ** 2
    f0 = np.array([100, 0, 2.0, 200, 1.5, 0, 2.0, 150], np.float32)
    lf0, gv, n_utt = stats_ref.speaker_stats(sp, f0, [3, 1, 2, 2], [0, 1, 2, 0], 4)
    assert lf0[:, 0].tolist() == [2, 1, 0, 0] and n_utt.tolist() == [2, 0, 1, 0]
    assert np.isnan(lf0[2:, 1:]).all() and np.isnan(gv[1]).all() and np.isnan(gv[3]).all()
    assert np.allclose(lf0[0, 1:], [np.log([100, 150]).mean(), np.log([100, 150]).std()])
    assert np.allclose(gv[0], (sp[:3].var(axis=0) + sp[6:].var(axis=0)) / 2)
