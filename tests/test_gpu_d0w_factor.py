"""Decoder layer 0's and the merge layer's weight gradients from ONE plane GEMM (csrc/gfx950_layers.hip: d0w_factor_on).

h_f = z_f Wz + T[y_f] goes straight into decoder layer 0's transposed conv, so dW_conv, dWz and the per-speaker sums of d(h) follow
from dWc = z^T du0 and S[s] = sum_{f: y_f = s} du0_f pushed through the conv kernels as 138 pseudo-frames.  Everything is compared
against the float64 oracle run inside the test, with the bars and the comparison of tests/test_gpu_parity.py (compare_everything);
which route the backward pass took is read back from the context (Engine.d0w_route, include/vaenpvc.h: VAENPVC_D0W_ROUTE_*)."""
import numpy as np
import pytest
import torch

import test_gpu_parity as TP
from oracle import convvae_oracle as O

pytestmark = pytest.mark.gpu

ROUTE_FP32, ROUTE_FACTOR, ROUTE_PLANES, ROUTE_PLANES_REDO = 0, 1, 2, 3
# both sites on the plane kernels at any batch size, for every precision (bits 28 and 26 of both masks cleared: plane GEMMs and
# every conv site on the view GEMMs -- the selection of test_view_conv_layers_against_oracle)
FORCED = TP.VIEW_CONV
SMALL = [(37, 5), (257, 12), (1, 7)]   # the batches the plane-kernel tests pin: ragged tiles; one frame = a K = 1 GEMM and nine empty speakers


@pytest.mark.parametrize('precision', ['bf16x2', 'bf16x3'])
@pytest.mark.parametrize('F,seed', SMALL)
def test_forced_route_at_small_batches(F, seed, precision, monkeypatch):
    """VAENPVC_D0W_FACTOR=2: the route wherever the kernels serve the shape.  Every forward tensor and every gradient; at one frame
    the nine absent speakers' rows of S are exact zeros and must contribute nothing."""
    monkeypatch.setenv('VAENPVC_D0W_FACTOR', '2')
    eng = TP.make_engine('vcc', 'auto', FORCED, precision=precision)
    fails = TP.compare_everything(eng, F, seed, '%s d0w-factor F%d ' % (precision, F))
    assert eng.d0w_route == ROUTE_FACTOR, 'the factorised route did not run'
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('precision', ['bf16x2', 'bf16x3', 'bf16'])
def test_default_selection_at_1027_frames(precision):
    """The default switch (1) and the default kernel selection just above the threshold: ragged tiles everywhere, all ten speakers
    present.  Three operand planes keep decoder layer 0's weight gradient on the exact-fp32 kernel (no plane route to replace)."""
    F, seed = 1027, 31
    P, x, y, eps, R = TP.oracle_case(F, seed)
    assert len(np.unique(y)) == 10
    eng = TP.make_engine('vcc', 'auto', precision=precision)
    if precision == 'bf16':
        fails = []
        l3, grads = TP.run_train(eng, P, x, y, eps)
        _, G = TP.oracle_grads(eng, TP.ARCHS['vcc'], P, x, y, eps)
        assert np.isfinite(grads).all()
        TP.check('bf16 d0w-factor F1027 loss3', l3, np.array([R['G'], R['D_KL'], R['logP']]), TP.BF16_TOL_ACT, fails)
        for name, (off, shape) in eng.layout.items():
            n = int(np.prod(shape))
            TP.check('bf16 d0w-factor F1027 grad ' + name, grads[off:off + n].reshape(shape), G[name], TP.BF16_TOL_GRAD, fails)
    else:
        fails = TP.compare_everything(eng, F, seed, '%s d0w-factor default F%d ' % (precision, F))
    assert eng.d0w_route == (ROUTE_FP32 if precision == 'bf16x3' else ROUTE_FACTOR)
    assert not fails, '\n'.join(fails)


def test_a_batch_with_one_speaker():
    """All frames of one speaker: nine rows of S are zero, one is the whole column sum.  The gradients of emb, Wy and the three merge
    biases are functions of D^T(S) alone (every tensor is checked)."""
    F, key = 37, -37
    if (F, key) not in TP._oracle_cache:
        arch = TP.ARCHS['vcc']
        P = O.init_params(arch, 5)
        x, y, eps = O.make_inputs(arch, F, 5)
        y = np.full_like(y, 3)
        TP._oracle_cache[(F, key)] = (P, x, y, eps, O.np_forward(arch, P, x, y, eps))
    eng = TP.make_engine('vcc', 'auto', FORCED)
    eng.set_d0w_factor(2)
    fails = TP.compare_everything(eng, F, key, 'd0w-factor one speaker F%d ' % F)
    assert eng.d0w_route == ROUTE_FACTOR
    merge = [f for f in fails if any(k in f for k in ('y_emb', 'fully_connected_1', 'BiasAdd', 'fully_connected/biases'))]
    assert not merge, '\n'.join(merge)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('F,seed,masks', [(1027, 31, (0xffffffff, 0xffffffff)), (37, 5, FORCED)])
def test_switch_off_is_the_frame_sized_route(F, seed, masks):
    """0 = the launches of the plane route as it was: one weight-gradient GEMM over the frames per layer, the planes of h from the forward pass."""
    eng = TP.make_engine('vcc', 'auto', masks)
    eng.set_d0w_factor(0)
    fails = TP.compare_everything(eng, F, seed, 'd0w-factor off F%d ' % F)
    assert eng.d0w_route == ROUTE_PLANES
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('fwd_mode,bwd_mode,route', [(0, 2, ROUTE_FACTOR), (2, 0, ROUTE_PLANES_REDO)])
def test_switch_changed_between_the_passes(fwd_mode, bwd_mode, route):
    """The forward pass decides whether decoder layer 0 leaves the operand planes of h.  A backward-only call under another switch
    must not read planes that were never written: 0 -> 2 needs none (factorised), 2 -> 0 re-makes them.  target = x: the gradient of
    the train step itself."""
    F, seed = 1027, 31
    arch = TP.ARCHS['vcc']
    P, x, y, eps, R = TP.oracle_case(F, seed)
    eng = TP.make_engine('vcc', 'auto')
    eng.set_d0w_factor(fwd_mode)
    xt, yt, et = TP.upload(eng, P, x, y, eps)
    grads = torch.full((eng.n_params,), float('nan'), device=eng.device)
    eng.train_fwd_bwd(xt, yt, et, grads)
    assert eng.d0w_route == (ROUTE_FACTOR if fwd_mode else ROUTE_PLANES)
    eng.set_d0w_factor(bwd_mode)
    grads.fill_(float('nan'))
    eng.train_bwd_target(xt, yt, et, xt, grads)
    torch.cuda.synchronize()
    assert eng.d0w_route == route
    g = grads.cpu().numpy()
    _, G = TP.oracle_grads(eng, arch, P, x, y, eps)
    fails = []
    assert np.isfinite(g).all()
    for name, (off, shape) in eng.layout.items():
        n = int(np.prod(shape))
        TP.check('d0w-factor %d->%d grad %s' % (fwd_mode, bwd_mode, name), g[off:off + n].reshape(shape), G[name], TP.TOL_GRAD, fails)
    assert not fails, '\n'.join(fails)


def test_hipgraph_replay_matches_eager_on_the_factorised_route():
    """The comparison of test_hipgraph_replay_matches_eager at 257 frames with the route forced: nothing in it allocates or synchronises."""
    from hipvae.dp import Stepper
    arch = TP.ARCHS['vcc']
    F = 257
    P = O.init_params(arch, 3)
    x, y, eps = O.make_inputs(arch, F, 3)
    res = []
    for use_graph in (False, True):
        eng = TP.make_engine('vcc', 'auto', FORCED)
        eng.set_d0w_factor(2)
        xt, yt, et = TP.upload(eng, P, x, y, eps)
        st = Stepper(eng, 1e-4, 0.5, 0.999)
        g1 = p1 = None
        if use_graph:
            st.capture(xt, yt, et)
        for t in range(3):
            l3 = st.replay() if use_graph else st.step(xt, yt, et)
            if t == 0:
                g1, p1 = st.grads.clone(), eng.params.clone()
        torch.cuda.synchronize()
        assert st.step_count == 3 and eng.d0w_route == ROUTE_FACTOR
        res.append((eng.params.cpu().numpy().copy(), l3.cpu().numpy().copy(), g1.cpu().numpy().copy(), p1.cpu().numpy().copy()))
    p0 = O.flatten_params(P)
    g_e, g_g = res[0][2], res[1][2]
    assert np.abs(g_e - g_g).max() <= 1e-5 * np.abs(g_e).max()
    strong = np.abs(g_e) > 1e-2 * np.abs(g_e).max()
    assert strong.sum() > 1000
    u_e, u_g = res[0][3] - p0, res[1][3] - p0
    assert np.abs(u_e - u_g)[strong].max() <= 1e-3 * np.abs(u_e).max()
    d_eager, d_graph = res[0][0] - p0, res[1][0] - p0
    assert np.abs(d_eager - d_graph)[strong].max() <= 5e-2 * np.abs(d_eager).max()
    assert np.abs(d_eager - d_graph).mean() <= 5e-3 * np.abs(d_eager).max()
    assert np.allclose(res[0][1], res[1][1], rtol=1e-4)
