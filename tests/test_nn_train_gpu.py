"""The MLP trainer on the device (rvs_nn_train_grad / _adam_step / _epoch through
rvspecfit_amd.nn.train_interpolator) against tests/golden/nn_train_cases.npz -- made
with the reference's NNInterpolator and torch's own Adam, l1_loss and
ReduceLROnPlateau -- and against float64 autograd of tests/refmachines/
nn_train_torch.py.  Every tolerance is a multiple of an error the fixture's own float32
torch run has against float64, recorded by tests/golden/make_golden_nn_train.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmachines import nn_train_torch as rm  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NL = 5


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(GOLD, 'nn_train_cases.npz')))


@pytest.fixture(scope='module')
def F():
    return rm.fixture_rows()


def _trainer(G, F, batch=100):
    from rvspecfit_amd.nn import train_interpolator as ti
    return ti.Trainer(F['dats'], F['x'], [G['W%d' % i] for i in range(NL)],
                      [G['b%d' % i] for i in range(NL)], F['D0'], F['SD0'], F['spread0'],
                      batch=batch)


@pytest.mark.parametrize('nb', [32, 100])
def test_gradients_against_float64_autograd(G, F, nb):
    idx = G['idx%d' % nb]
    pre = 'g%d_' % nb
    tr = _trainer(G, F)
    loss, dW, db, res = tr.grad(idx, resid=True)
    res = res.cpu().double()
    t64 = {k: torch.as_tensor(F[k]).double() for k in ('dats', 'x', 'D0', 'SD0')}
    W64 = [torch.as_tensor(G['W%d' % i]).double() for i in range(NL)]
    b64 = [torch.as_tensor(G['b%d' % i]).double() for i in range(NL)]
    l64, res64, dW64, db64 = rm.loss_and_grads(
        W64, b64, t64['x'][idx], t64['dats'][idx], t64['D0'], t64['SD0'], F['spread0'],
        sign=torch.sign(res))
    res_tol = 4 * float(G[pre + 'res_err'])
    err = float((res - res64).abs().max())
    print('residual error %.3g (tolerance %.3g)' % (err, res_tol))
    assert err <= res_tol
    assert abs(float(loss.item()) - float(l64)) <= res_tol / F['spread0']
    # signs: different from float64 only at near-ties, and at no more of them than exist
    flip = torch.sign(res) != torch.sign(res64)
    tie = res64.abs() < 8 * res_tol
    print('sign flips %d, near-ties %d (fixture %d)' % (int(flip.sum()), int(tie.sum()),
                                                        int(G[pre + 'ntie'])))
    assert not bool((flip & ~tie).any())
    assert int(flip.sum()) <= int(G[pre + 'ntie'])
    gerr = G[pre + 'gerr']
    for l in range(NL):
        for j, (g, g64) in enumerate(((dW[l], dW64[l]), (db[l], db64[l]))):
            e = float((g.cpu().double() - g64).norm() / g64.norm())
            print('layer %d %s: %.3g (tolerance %.3g)' % (l, 'Wb'[j], e,
                                                          4 * gerr[2 * l + j]))
            assert e <= 4 * gerr[2 * l + j]


def test_adam_against_torch(G):
    """rvs_nn_adam_step on the layers 0 and 3 of the fixture's run (a chain 4 -> 64 ->
    40), fed the fixture's float32 gradients for ten updates.

    Moments: equal to torch's, bit for bit, at every recorded state (1, 2, 10 updates).

    Weights after one and two updates: within 2 ulp of |w| + lr, the bound as the issue
    states it.  After each later update k the deviation d_k from the fixture's w_k is
    held to a bound built update by update from the recorded trajectory:

        d_k <= d_{k-1} + 2 ulp(w_k - w_{k-1}) + ulp(max(|w_{k-1}|, |w_k|))

    The update u = (a m) / (sqrt(v) / c + eps) is computed from equal moments; torch's
    float32 sqrt on the CPU is within one ulp of the correctly rounded root but not
    equal to it (0.6 % of this run's values differ), which moves the quotient, itself
    rounded, by at most 2 ulp of u, and |u| = |w_k - w_{k-1}| up to rounding.  The sum
    w + u is rounded once on each side: two results whose inputs differ by d differ by
    at most d plus one ulp of the result.  Nothing else enters.  (Held against |w_10| + lr
    alone the ten updates read 3.7 ulp on ONE weight of layer 3, which falls from
    9.7e-3 to 5.8e-5 and took one rounding of 9.7e-3's size at its second update; that
    figure is printed.)"""
    from rvspecfit_amd.nn import train_interpolator as ti
    lay = (0, 3)
    W = [G['W%d' % l] for l in lay]
    b = [G['b%d' % l] for l in lay]
    tr = ti.Trainer(np.zeros((1, 40), np.float32), np.zeros((1, 4), np.float32), W, b,
                    np.zeros(40), np.ones(40), 1.0, batch=1)
    dev = lambda a: torch.as_tensor(a).to('cuda')  # noqa: E731
    lr, eps = 1e-3, float(np.finfo(np.float32).eps)
    names = [(k, nm, l) for k, l in enumerate(lay) for nm in 'Wb']
    prev = {(nm, l): G['%s%d' % (nm, l)] for _, nm, l in names}
    bound = {key: np.zeros_like(w) for key, w in prev.items()}
    for s in range(10):
        tr.adam_step([dev(G['adam_dW%d_s%d' % (l, s)]) for l in lay],
                     [dev(G['adam_db%d_s%d' % (l, s)]) for l in lay], lr)
        for k, nm, l in names:
            p, m, v = ((tr.W, tr.mW, tr.vW) if nm == 'W' else (tr.b, tr.mb, tr.vb))
            tag = '%s%d_n%d' % (nm, l, s + 1)
            want = G['adam_p_' + tag]
            dp = np.abs(p[k].cpu().numpy() - want)
            bound[nm, l] += 2 * np.spacing(np.abs(want - prev[nm, l])) + \
                np.spacing(np.maximum(np.abs(want), np.abs(prev[nm, l])))
            prev[nm, l] = want
            literal = np.max(dp / (np.abs(want) + lr)) / eps
            print(tag, 'ulp of |w| + lr: %.2f; share of the trajectory bound: %.2f'
                  % (literal, np.max(dp / bound[nm, l])))
            if s + 1 <= 2:
                assert literal <= 2
            assert np.all(dp <= bound[nm, l])
            if 'adam_m_' + tag in G:
                assert np.array_equal(m[k].cpu().numpy(), G['adam_m_' + tag])
                assert np.array_equal(v[k].cpu().numpy(), G['adam_v_' + tag])


def test_steps_against_the_fixture(G, F):
    perms = G['step_perms'].astype(np.int64)
    tr = _trainer(G, F)
    sl = torch.cat([tr.epoch(p, 1e-3, step_loss=True) for p in perms]).cpu().numpy()[:10]
    for s in (0, 1, 9):
        tol = 4 * abs(G['step_loss'][s] - G['step_loss64'][s])
        print('step %d: %.9g, fixture %.9g float64 %.9g (tolerance %.3g)'
              % (s + 1, sl[s], G['step_loss'][s], G['step_loss64'][s], tol))
        assert abs(sl[s] - G['step_loss'][s]) <= tol


def test_two_runs_give_the_same_bits(G, F):
    perms = G['conv_perms'][:5].astype(np.int64)
    runs = []
    for _ in range(2):
        tr = _trainer(G, F)
        acc = []
        for p in perms:      # 254 = 2 x 100 + 54: the short last batch included
            tr.epoch(p, 1e-3)
            acc.append(tr.loss_accum.clone())
        runs.append([t.cpu() for t in tr.W + tr.b + tr.mW + tr.mb + tr.vW + tr.vb + acc])
    assert tr.steps == 15
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_convergence_and_schedule(G, F):
    from rvspecfit_amd.nn import train_interpolator as ti
    tr = _trainer(G, F)
    sched = ti.PlateauScheduler(1e-3, patience=3)
    acc, lrs = [], []
    for p in G['conv_perms'].astype(np.int64):
        lrs.append(sched.lr)
        tr.epoch(p, sched.lr)
        acc.append(float(tr.loss_accum.item()))
        sched.step(acc[-1])
    final = G['conv_accum'][:, -1]
    spread = (final.max() - final.min()) / final.min()
    print('final lossAccum %.6g; fixture %s, relative spread %.3g' % (acc[-1], final,
                                                                     spread))
    assert acc[-1] <= final.max() * (1 + spread)
    # the rates are torch's ReduceLROnPlateau on the run's own losses
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    ts = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=3, eps=1e-9,
                                                    threshold=1e-5)
    for a, lr in zip(acc, lrs):
        assert opt.param_groups[0]['lr'] == lr
        ts.step(a)


def _interpol_specs():
    import test_make_interpol_gpu as mi
    from rvspecfit_amd import make_interpol
    lam_hr, rows, vec = mi._models('gold_b')
    l0, l1, st = mi.SETUPS['gold_b'][3]
    setup = ('gold_b', l0, l1, make_interpol.Resolution(resol=2000.), st, True)
    return lam_hr, rows, vec, setup


def test_end_to_end(G, tmp_path):
    """build_specs -> train -> TemplateLibrary of kind nn -> eval, outside flag,
    vel_fit.process"""
    from rvspecfit_amd import make_ccf, make_interpol, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.library import TemplateLibrary
    from rvspecfit_amd.nn import train_interpolator as ti
    lam_hr, rows, vec, setup = _interpol_specs()
    D = make_interpol.build_specs(lam_hr, rows, vec, setup)
    info = {}
    ck = str(tmp_path / 'state.npz')
    kw = dict(nlayers=2, width=64, npc=40, patience=3, verbose=False,
              generator=torch.Generator().manual_seed(5))
    rec = ti.train(D, num_epochs=40, checkpoint=ck, info=info, **kw)
    assert not os.path.exists(ck)           # removed at the end, as the reference does
    lib = TemplateLibrary('gold_b', rec)
    assert lib.kind == 'nn'
    par = torch.as_tensor(np.ascontiguousarray(vec.T)).to('cuda')
    templ, outside = lib.eval_batch(par)
    # the fold of SD_0, D_0 into pc_layer: the library gives exp of the trainer's own
    # predictions, at the tolerance test_gpu_parity.py asks of rvs_template_nn
    np.testing.assert_allclose(templ.cpu().numpy(), np.exp(info['pred'].astype(np.float64)),
                               rtol=3e-6)
    dats = D['specs'].cpu().numpy()
    mean_abs = np.abs(np.log(templ.cpu().numpy()) - dats).mean()
    assert abs(mean_abs - info['final_loss'] * info['spread0']) <= 3e-6
    assert info['losses'][-1] < 0.5 * info['losses'][0]
    assert np.all(outside.cpu().numpy() == 0)
    far = par.clone()
    far[:, 0] = 12000.
    assert np.all(lib.eval_batch(far)[1].cpu().numpy() > 0)
    # a CCF set attaches as to any library; process on a noiseless training row
    d = np.load(os.path.join(GOLD, 'lib_gold_b.npz'))
    import test_make_interpol_gpu as mi
    lib.add_ccf_set(make_ccf.build_ccf_set(D, ccfconf=mi._conf(d), every=20,
                                           vsinis=[0., 100.]))
    spec_inter.register_library(lib, 'trained-nn://')
    cfg = dict(template_lib='trained-nn://', min_vel=-1000, max_vel=1000,
               min_vel_step=0.2, vel_step0=5, min_vsini=0.1, max_vsini=500,
               second_minimizer=False)
    i = 100
    lam = D['lam']
    sel = slice(50, len(lam) - 50)
    spec = np.exp(dats[i].astype(np.float64))[sel]
    from rvspecfit_amd.engine import SpecBatch
    sd = [spec_fit.SpecData('gold_b', lam[sel], spec, spec * 0 + 0.01)]
    p0 = {k: np.array([v]) for k, v in zip(('teff', 'logg', 'feh', 'alpha'), vec[:, i])}
    p0['vsini'] = np.array([5.])
    r = vel_fit.process(SpecBatch.from_specdata([sd]), p0, config=cfg,
                        options=dict(npoly=5))
    vel = float(r['vel'][0])
    assert np.isfinite(vel) and abs(vel) < 50
    assert int(r['status'][0]) == 0          # no warning bit


def test_resume_from_a_checkpoint(tmp_path):
    """A run that stops after its 32nd epoch leaves the checkpoint of that epoch; the
    checkpoint holds the weights an uninterrupted run of 32 epochs over the same
    permutations ends on (runs repeat bit for bit), and a run resumed from it at rate
    zero ends on exactly those, all layers, pc_layer through the fold of SD_0, D_0.
    Without resume the same call starts from the default initialisation instead."""
    from rvspecfit_amd import make_interpol
    from rvspecfit_amd.nn import train_interpolator as ti
    lam_hr, rows, vec, setup = _interpol_specs()
    D = make_interpol.build_specs(lam_hr, rows, vec, setup)
    T = vec.shape[1]
    g = torch.Generator().manual_seed(9)
    perms = [torch.randperm(T, generator=g).numpy() for _ in range(32)]
    kw = dict(nlayers=2, width=64, npc=40, patience=3, verbose=False)
    ck = str(tmp_path / 'state.npz')
    with pytest.raises(StopIteration):      # the 33rd epoch has no permutation: interrupted
        ti.train(D, num_epochs=40, checkpoint=ck, perms=perms, **kw)
    assert os.path.exists(ck)
    info = {}
    full = ti.train(D, num_epochs=32, perms=perms, info=info, **kw)
    dims = full['nn_dims']
    W, b = ti.load_checkpoint(ck, dims)
    init = ti.init_weights(dims)
    for l in range(4):
        assert np.array_equal(W[l].numpy(), full['nn_W%d' % l])
        assert np.array_equal(b[l].numpy(), full['nn_b%d' % l])
        assert not np.array_equal(W[l].numpy(), init[0][l].numpy())
    D0, SD0 = info['D0'], info['SD0']
    assert np.array_equal(SD0[:, None] * W[4].numpy(), full['nn_W4'])
    assert np.array_equal(D0 + b[4].numpy() * SD0, full['nn_b4'])
    one = dict(num_epochs=1, perms=[np.arange(T)], learning_rate0=0.0, **kw)
    again = ti.train(D, checkpoint=ck, resume=True, **one)
    assert not os.path.exists(ck)           # removed at the end, as the reference does
    for l in range(5):
        assert np.array_equal(again['nn_W%d' % l], full['nn_W%d' % l])
        assert np.array_equal(again['nn_b%d' % l], full['nn_b%d' % l])
    ti.save_checkpoint(ck, ti.Trainer(D['specs'], info['x'].astype(np.float32), W, b, D0,
                                      SD0, info['spread0']))
    fresh = ti.train(D, checkpoint=ck, resume=False, **one)   # the file is not read
    for l in range(4):
        assert np.array_equal(fresh['nn_W%d' % l], init[0][l].numpy())
        assert not np.array_equal(fresh['nn_W%d' % l], full['nn_W%d' % l])


def test_pca_init(capsys):
    from rvspecfit_amd import make_interpol
    from rvspecfit_amd.nn import train_interpolator as ti
    lam_hr, rows, vec, setup = _interpol_specs()
    D = make_interpol.build_specs(lam_hr, rows, vec, setup)
    info = {}
    npc = 20
    rec = ti.train(D, nlayers=2, width=64, npc=npc, num_epochs=1, learning_rate0=0.0,
                   pca_init=True, info=info, perms=[np.arange(vec.shape[1])])
    dats = D['specs'].cpu().numpy().astype(np.float64)
    # at rate zero the record's pc_layer is the initial one times SD_0
    Wpc = rec['nn_W4'].astype(np.float64)
    assert np.allclose(np.sqrt((Wpc**2).sum(axis=0)), 1, atol=1e-5)
    X = dats - dats.mean(axis=0)
    Vt = np.linalg.svd(X, full_matrices=False)[2][:npc]
    cosines = np.linalg.svd(Vt @ np.linalg.qr(Wpc)[0], compute_uv=False)
    assert np.all(cosines > 1 - 1e-5)        # principal angles ~ 0
    loss0 = np.abs(X - X @ Vt.T @ Vt).mean() / info['spread0']
    assert abs(info['loss0'] / loss0 - 1) < 1e-6
    assert 'loss0 %s' % info['loss0'] in capsys.readouterr().out


def test_save_specs_switch(tmp_path):
    """make_interpol --save_specs writes the rows train_interpolator.main reads;
    without the switch the library file is the same, byte for byte.  Both runs are of
    this code (make_interpol needs the device, so this is a GPU test, on FITS files
    written here): it shows that the switch adds a file and changes nothing else, not
    that the output equals an earlier version's."""
    from rvspecfit_amd import fits_min, make_interpol, synth
    from rvspecfit_amd.library import TemplateLibrary
    from rvspecfit_amd.nn import train_interpolator as ti
    pre = str(tmp_path) + '/'
    os.makedirs(pre + 'specs')
    lam_hr = np.linspace(4400., 4700., 15001)
    _, vec = synth.regular_grid(nteff=3, nlogg=2, nfeh=2, nalpha=2)
    for i in range(vec.shape[1]):
        h = fits_min.Header()
        for key, v in zip(('PHXTEFF', 'PHXLOGG', 'PHXM_H', 'PHXALPHA'), vec[:, i]):
            h[key] = float(v)
        row = synth.spectrum(lam_hr, *vec[:, i]).astype(np.float32)
        fits_min.HDUList([fits_min.PrimaryHDU(row, h)]).writeto(
            pre + 'specs/m%03d.fits' % i)
    fits_min.HDUList([fits_min.PrimaryHDU(lam_hr)]).writeto(pre + 'wave.fits')
    args = ['--setup', 'cl', '--lambda0', '4500', '--lambda1', '4600', '--step', '0.4',
            '--resol', '2000', '--templprefix', pre, '--mask', 'specs/*.fits',
            '--wavefile', pre + 'wave.fits']
    a = make_interpol.main(args + ['--oprefix', pre + 'a'])
    b = make_interpol.main(args + ['--oprefix', pre + 'b', '--save_specs'])
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert not os.path.exists(pre + 'a/specs_cl.npz')
    fname = ti.main(['--dir', pre + 'b', '--setup', 'cl', '--nlayers', '1', '--width',
                     '32', '--npc', '8', '--num_epochs', '3', '--batch', '10'])
    lib = TemplateLibrary.from_npz('cl', fname)
    assert lib.kind == 'nn' and list(lib.nn_dims) == [4, 32, 32, 8, lib.ntp]
    p = np.load(pre + 'b/pred_cl.npz')
    assert p['pred'].shape == p['dats'].shape == (vec.shape[1], lib.ntp)
