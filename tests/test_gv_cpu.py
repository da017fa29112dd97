"""Global-variance post-filter, host side: the statistics builder (build.py), the `--gv` flag of convert.py and its
checks before any device work, and the argument checks of the C entry points (none of which touch a device)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import gv_ref
from helpers import PKG, load_arch
from hipvae import lib as L


def load_build():
    spec = importlib.util.spec_from_file_location('vaenpvc_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_tree(root, seed=0):
    """Synthetic .bin tree: three speakers, utterances of 1 to 90 frames (one of 1 frame, one speaker with only that one)."""
    rng = np.random.default_rng(seed)
    utts = {}
    plan = {'SF1': (0, [40, 1, 65]), 'SM1': (3, [1]), 'TM3': (9, [30, 90, 2, 57])}
    for spk, (sid, lens) in plan.items():
        d = os.path.join(root, 'bin', 'Training Set', spk)
        os.makedirs(d)
        for u, n in enumerate(lens):
            r = rng.standard_normal((n, 1029)).astype(np.float32)
            r[:, :513] = rng.uniform(-9, -3, 513) + rng.uniform(0.05, 0.8, 513) * rng.standard_normal((n, 513))
            r[:, 1026] = np.where(rng.random(n) > 0.3, rng.uniform(80, 300, n), 0.0)
            r[:, -1] = sid
            r.tofile(os.path.join(d, '1000%02d.bin' % u))
            utts.setdefault(spk, []).append(r)
    return utts


def test_build_writes_reference_stats_and_gv(tmp_path, monkeypatch):
    import analyzer
    utts = write_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    load_build().main(['--train_file_pattern', os.path.join(str(tmp_path), 'bin', 'Training Set', '*', '*.bin')])
    etc = os.path.join(str(tmp_path), 'etc')
    files = sorted(os.listdir(etc))
    assert files == ['SF1.npf', 'SF1_gv.npf', 'SM1.npf', 'TM3.npf', 'TM3_gv.npf', 'xmax.npf', 'xmin.npf']
    allr = np.concatenate([r for spk in sorted(utts) for r in utts[spk]])
    for name, q in (('xmin', 0.5), ('xmax', 99.5)):
        assert os.path.getsize(os.path.join(etc, name + '.npf')) == 513 * 4
        got = np.fromfile(os.path.join(etc, name + '.npf'), np.float32)
        assert np.array_equal(got, np.percentile(allr[:, :513], q, axis=0).astype(np.float32))
    for spk, rs in utts.items():
        # build.py:41-51 on the speaker's frames, float32 arithmetic as in the reference
        f0 = np.concatenate([r[:, 1026] for r in rs])
        f0 = np.log(f0[f0 > 2.])
        assert os.path.getsize(os.path.join(etc, spk + '.npf')) == 8
        assert np.array_equal(np.fromfile(os.path.join(etc, spk + '.npf'), np.float32),
                              np.asarray([f0.mean(), f0.std()], np.float32))
        if spk == 'SM1':
            continue                     # its only utterance has 1 frame: no GV statistics
        assert os.path.getsize(os.path.join(etc, spk + '_gv.npf')) == 513 * 4
        want = gv_ref.speaker_gv([r[:, :513] for r in rs]).astype(np.float32)
        assert np.array_equal(np.fromfile(os.path.join(etc, spk + '_gv.npf'), np.float32), want)
    assert analyzer.load_npf(os.path.join(etc, 'TM3_gv.npf')).shape == (513,)


def test_build_rejects_mixed_speaker_file(tmp_path, monkeypatch):
    write_tree(str(tmp_path))
    bad = os.path.join(str(tmp_path), 'bin', 'Training Set', 'TM3', '100001.bin')
    r = np.fromfile(bad, np.float32).reshape(-1, 1029)
    r[5, -1] = 0
    r.tofile(bad)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match='100001.bin'):
        load_build().main(['--train_file_pattern', os.path.join(str(tmp_path), 'bin', 'Training Set', '*', '*.bin')])


def test_convert_gv_flag_defaults_off():
    import convert as conv_cli
    assert conv_cli.parse_args(['--model', 'ConvVAE']).gv is False
    assert conv_cli.parse_args(['--model', 'ConvVAE', '--gv']).gv is True


def _convert_tree(root):
    logdir = os.path.join(root, 'logdir', 'train', 'stamp')
    os.makedirs(logdir)
    with open(os.path.join(logdir, 'architecture-vae-vcc2016.json'), 'w') as fp:
        json.dump(load_arch(), fp)
    os.makedirs(os.path.join(root, 'etc'))
    return ['--src', 'SF1', '--trg', 'TM3', '--model', 'ConvVAE', '--checkpoint', os.path.join(logdir, 'model.ckpt-7'),
            '--output_dir', os.path.join(root, 'logdir'), '--gv']


@pytest.mark.parametrize('content', ['missing', 'short', 'negative', 'nan'])
def test_convert_gv_file_checked_before_device_work(tmp_path, monkeypatch, content):
    import analyzer
    import convert as conv_cli
    argv = _convert_tree(str(tmp_path))
    path = os.path.join('.', 'etc', 'TM3_gv.npf')
    g = np.full(513, 0.04, np.float32)
    if content == 'short':
        g = g[:512]
    elif content == 'negative':
        g[7] = -1e-3
    elif content == 'nan':
        g[300] = np.nan
    if content != 'missing':
        g.tofile(os.path.join(str(tmp_path), 'etc', 'TM3_gv.npf'))

    def no_device(*a, **k):
        raise AssertionError('device work before the GV file was checked')
    monkeypatch.setattr(analyzer, 'Tanhize', no_device)
    monkeypatch.chdir(tmp_path)
    with pytest.raises((FileNotFoundError, ValueError)) as e:
        conv_cli.main(argv)
    assert path in str(e.value)


def test_gv_symbols_exported():
    lib = L.load_library()
    assert lib.vaenpvc_abi_version() == L.ABI_VERSION == 4
    for n in ('vaenpvc_gv_workspace_bytes', 'vaenpvc_gv_postfilter'):
        assert hasattr(lib, n) and n in L.SIGNATURES


def test_gv_argument_checks_without_device():
    lib = L.load_library()
    F, n, H = 1000, 3, 513
    need = lib.vaenpvc_gv_workspace_bytes(F, n, H)
    assert need >= n * H * 16                                            # at least the per-bin map of every utterance
    assert lib.vaenpvc_gv_workspace_bytes(1 << 20, 1, 513) > 0          # F beyond 2^16 (and 2^18) is accepted
    for bad in ((-1, n, H), (F, 0, H), (F, -2, H), (F, n, 0), (F, n, -1)):
        assert lib.vaenpvc_gv_workspace_bytes(*bad) == L.MODE_INFER - 1  # VAENPVC_E_ARG
    # fake device addresses: every rejection happens before a launch
    x, off, lo, hi, g, sp, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 64 << 20, 128 << 20

    def call(**kw):
        a = dict(x=x, off=off, n=n, F=F, H=H, lo=lo, hi=hi, g=g, sp=sp, ws=ws, nb=need)
        a.update(kw)
        return lib.vaenpvc_gv_postfilter(a['x'], a['off'], a['n'], a['F'], a['H'], a['lo'], a['hi'], a['g'], a['sp'],
                                         a['ws'], a['nb'], None)
    E_ARG, E_WS = -1, -2
    for kw in ({'n': 0}, {'n': -1}, {'F': -1}, {'H': 0}, {'H': -5}, {'x': None}, {'off': None}, {'lo': None},
               {'hi': None}, {'g': None}, {'sp': None}, {'sp': x + 4}, {'x': sp - 8}):
        assert call(**kw) == E_ARG, kw
    assert call(nb=need - 1) == E_WS
    assert b'workspace too small' in lib.vaenpvc_last_error()
    assert call(ws=None) == E_WS
    assert call(ws=ws + 4) == E_ARG                                       # workspace alignment
