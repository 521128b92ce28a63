"""GPU: the action classifier (csrc/rgp_action.hip, engine.ActionEngine, models/action_classification.py) against the
float64 helper tests/action_ref.py.

Shapes: B in {1, 10, 16, 23} (a single row; the reference batch with padded tile rows; a full 16-row MFMA tile; a second,
ragged tile) at C in {8, 24} (K = 392: under one 512-row slab; K = 1176: two slabs and a ragged third; both end inside a
64-row update block), plus B = 10 at C = 1024 (98 slabs: every slab and the fixed-order sum over them).

Bounds.  On exact operands (action_ref.exact_operands) every sum is exact in fp32 in any order, so fc1, a, dx and g must
EQUAL the float64 values; the updated W1 / m / v then differ from float64 Adam by Adam's own fp32 arithmetic only (2e-6 of
the largest value, the bound of test_optimizers_match_tf_semantics).  On random data the project's bounds apply: forward
intermediates max|err| / max|ref| <= 2e-5 (f32) / 2e-2 (bf16), gradients relative Frobenius error <= 1e-3 / 3e-2, the loss
relative error <= 1e-5 / 2e-2."""
import numpy as np
import pytest
import torch

import action_ref as ref
from recurrent_gaze_prediction_amd import _lib, synthetic as syn
from recurrent_gaze_prediction_amd.engine import ActionEngine

pytestmark = pytest.mark.gpu

SHAPES = [(B, C) for C in (8, 24) for B in (1, 10, 16, 23)] + [(10, 1024)]
BIG = [(40, 8), (64, 24)]          # three and four 16-row tiles: the MT = 3 / 4 instantiations of the forward and the update pass
FWD_TOL = {'f32': 2e-5, 'bf16': 2e-2}
GRAD_TOL = {'f32': 1e-3, 'bf16': 3e-2}
LOSS_TOL = {'f32': 1e-5, 'bf16': 2e-2}
ADAM_TOL = 2e-6


def max_err(a, r):
    a, r = np.asarray(a, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


def fro_err(a, r):
    a, r = np.asarray(a, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    return np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-30)


def dev(x, gpu):
    return torch.tensor(np.asarray(x, np.float32), device=gpu).contiguous()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def modes_for(C):
    return [('NN', True), ('NN', False), ('SVM', True), ('SVM', False)] if C < 1024 else [('NN', True)]


@pytest.mark.parametrize('B,C', SHAPES + BIG)
def test_fc1_bit_for_bit(gpu, B, C):
    """h1 - b1 and a equal the float64 values exactly: bf16 and f32 plans, fused and unfused, with and without the gaze map."""
    for mode, use_gazemap in modes_for(C) + ([('NN', False)] if C == 1024 else []):
        ops = ref.exact_operands(100 + B + C, B, C, mode, use_gazemap)
        ref.check_exact(ops, mode, use_gazemap)
        p = ref.exact_params(ops, 1, mode, use_gazemap)
        want = ref.forward(p, ops['c3d'], ops['gazemap'], mode, use_gazemap)
        c3d, gm = dev(ops['c3d'], gpu), dev(ops['gazemap'], gpu)
        for dtype in ('bf16', 'f32'):
            for unfused in (False, True):
                e = ActionEngine(B, C, mode, use_gazemap, dtype, device=gpu, unfused=unfused)
                e.set_weights(p)
                e.fc1_fwd(c3d, gm)
                e.tail()
                tag = (mode, use_gazemap, dtype, unfused)
                h1 = host(e.read_buffer('h1')).reshape(B, -1)
                assert np.array_equal(h1 - np.asarray(p['b1'], np.float64), want['h1'] - np.asarray(p['b1'], np.float64)), tag
                if use_gazemap:
                    assert np.array_equal(host(e.read_buffer('a')).reshape(B, 49), want['a']), tag


def _adam32(w, m, v, g, lr_t, c1, c2):
    """The kernels' expression in fp32, for elements whose gradient is exactly zero."""
    f = np.float32
    m = f(0.9) * m + f(c1) * g
    v = f(0.999) * v + f(c2) * g * g
    return w - f(lr_t) * m / (np.sqrt(v) + f(1e-8)), m, v


@pytest.mark.parametrize('B,C', SHAPES + BIG)
def test_update_pass_bit_level(gpu, B, C):
    """rgp_action_fc1_update on exact operands and a caller-supplied exact d_h1, at step 0 (zero slots) and step 2 (non-zero
    m and v): dx exact and from the pre-update W1; W1 / m / v within Adam's own fp32 arithmetic of float64 Adam on the exact
    g (m after step 0 from zero slots is 0.1 g: g itself is pinned); zero-gradient elements get exactly the g = 0 update; the
    SVM update W -= lr (W + 50 g); the refreshed operand copy is what the next forward reads."""
    for mode, use_gazemap in modes_for(C):
        ops = ref.exact_operands(200 + B + C, B, C, mode, use_gazemap)
        if mode == 'NN':
            ops['c3d'][:, :, ::7] = 0                      # rows of W1 whose gradient is exactly zero
        p = ref.exact_params(ops, 2, mode, use_gazemap)
        ig = ref.input_grads(p, ops['c3d'], ops['gazemap'], ops['d_h1'], mode, use_gazemap)
        c3d, gm, d_h1 = dev(ops['c3d'], gpu), dev(ops['gazemap'], gpu), dev(ops['d_h1'], gpu)
        rs = np.random.RandomState(5)
        # (C = 1024: 51 MB per copy of W1 -- the fused pass alone, step 0 in bf16 and step 2 in f32)
        cases = [(d, u, s) for d in ('bf16', 'f32') for u in (False, True) for s in (0, 2)] if C < 1024 else \
            [('bf16', False, 0), ('f32', False, 2)]
        for dtype, unfused, step in cases:
            tag = (mode, use_gazemap, dtype, unfused, step)
            e = ActionEngine(B, C, mode, use_gazemap, dtype, save_for_backward=True, device=gpu, unfused=unfused)
            e.set_weights(p)
            W0 = np.asarray(p['W1'], np.float64)
            if mode == 'NN':
                lr = 2.0 ** -10                    # (exact in fp32: the host's lr_t is the library's)
                m0 = (rs.randn(*W0.shape) * 0.1 * (step > 0)).astype(np.float32)
                v0 = (rs.rand(*W0.shape) * (step > 0)).astype(np.float32)
                mv = e.slots()
                mv[0]['W1'].copy_(torch.tensor(m0))
                mv[1]['W1'].copy_(torch.tensor(v0))
                # the fused pass against float64 Adam; the unfused plan's W1 takes rgp_adam_clip_step, which forms 1 - beta and
                # lr_t from fp32 betas (1.f - 0.999f is 1.3e-5 off 0.001): float64 Adam with ITS constants, the same bound
                k = ref.fp32_adam_constants() if unfused else {}
                Wn, mn, vn = ref.adam(W0, ig['g'], m0.astype(np.float64), v0.astype(np.float64), step, lr, **k)
            else:
                lr = 0.01
                Wn = W0 - lr * (W0 + 50.0 * ig['g'])
            e.fc1_update(c3d, gm, d_h1, step, lr)
            W = host(e.weights['W1'])
            assert max_err(W, Wn) <= ADAM_TOL, tag
            if use_gazemap:
                assert np.array_equal(host(e.read_buffer('dx')).reshape(B, -1), ig['dx']), tag
            if mode == 'NN':
                m, v = host(mv[0]['W1']), host(mv[1]['W1'])
                print('action update %s B=%d C=%d: W %.2e m %.2e v %.2e' % (tag, B, C, max_err(W, Wn), max_err(m, mn), max_err(v, vn)))
                assert max_err(m, mn) <= ADAM_TOL and max_err(v, vn) <= ADAM_TOL, tag
                if step == 0:                              # zero slots: m = c1 g, one rounding from 0.1 g
                    assert max_err(m * 10.0, ig['g']) <= ADAM_TOL, tag
                zero = ig['g'] == 0
                assert zero.any()
                b1, b2 = k.get('b1', 0.9), k.get('b2', 0.999)
                lr_t = lr * np.sqrt(1.0 - b2 ** (step + 1)) / (1.0 - b1 ** (step + 1))
                wz, mz, vz = _adam32(p['W1'][zero], m0[zero], v0[zero], np.float32(0), lr_t, k.get('c1', 0.1), k.get('c2', 0.001))
                assert np.array_equal(m[zero], mz) and np.array_equal(v[zero], vz) and np.array_equal(W[zero], wz), tag
            # the operand copy written by the pass == a fresh pack of the weights read back
            logits = e.forward(c3d, gm)[0]
            h1 = e.read_buffer('h1')
            f = ActionEngine(B, C, mode, use_gazemap, dtype, device=gpu, unfused=unfused)
            f.set_weights({k: t.clone() for k, t in e.get_weights().items()})
            assert torch.equal(f.forward(c3d, gm)[0], logits) and torch.equal(f.read_buffer('h1'), h1), tag


def _random_case(seed, B, C, mode, use_gazemap):
    rs = np.random.RandomState(seed)
    p = syn.action_params(seed, mode, use_gazemap, dim_feat=C)
    if mode == 'SVM':                                      # (the reference's zero start has no margin inside the hinge's kink)
        p['W1'] = (rs.randn(49 * C, 13) * 0.1 / np.sqrt(49 * C)).astype(np.float32)
        p['b1'] = np.where(np.arange(13) % 3 == 0, 3.0, -2.0).astype(np.float32)   # margins far from the kink on both sides
    c3d = np.maximum(rs.randn(B, C, 49), 0).astype(np.float32)          # conv5b features are rectified
    gm = rs.rand(B, 49, 49).astype(np.float32) ** 8
    gm /= gm.sum((1, 2), keepdims=True)
    if use_gazemap:
        p['Wg'] = (p['Wg'] + 1.0).astype(np.float32)                    # attention weights around 1, as after training
    labels = (rs.rand(B, 13) < 0.3).astype(np.float32)
    return p, c3d, gm, labels


@pytest.mark.parametrize('B,C', SHAPES + BIG)
def test_whole_model_against_float64(gpu, B, C):
    """Random data: every forward intermediate, the loss, and every gradient -- the small ones and the intermediates through
    read_buffer, dW1 through Adam's m after one step from zero slots (m = 0.1 g) or, SVM, through the SGD update itself."""
    for mode, use_gazemap in modes_for(C):
        p, c3d_h, gm_h, labels_h = _random_case(300 + B + C, B, C, mode, use_gazemap)
        out, g = ref.grads(p, c3d_h, gm_h, labels_h, mode, use_gazemap)
        want_loss = ref.loss(p, out, labels_h, mode)
        c3d, gm, labels = dev(c3d_h, gpu), dev(gm_h, gpu), dev(labels_h, gpu)
        for dtype in ('f32', 'bf16'):
            tag = (mode, use_gazemap, dtype)
            e = ActionEngine(B, C, mode, use_gazemap, dtype, save_for_backward=True, device=gpu)
            e.set_weights(p)
            logits, y_pred = e.forward(c3d, gm)
            errs = {'logits': max_err(host(logits), out['logits']), 'y_pred': max_err(host(y_pred), out['y_pred']),
                    'h1': max_err(host(e.read_buffer('h1')), out['h1'])}
            if mode == 'NN':
                errs['h2'] = max_err(host(e.read_buffer('h2')), out['h2'])
            if use_gazemap:
                errs['a'] = max_err(host(e.read_buffer('a')), out['a'])
            loss_err = abs(float(e.loss(labels).item()) - want_loss) / abs(want_loss)
            lr = 1e-3
            step_loss = float(e.train_step(c3d, gm, labels, 0, lr).item())
            names = ['d_h1', 'd_b1'] + (['d_h2', 'd_logits', 'd_W2', 'd_b2', 'd_W3', 'd_b3'] if mode == 'NN' else []) \
                + (['dx', 'd_a', 'd_Wg'] if use_gazemap else [])
            gerrs = {k: fro_err(host(e.read_buffer(k)), g[k]) for k in names}
            if mode == 'NN':
                gerrs['d_W1'] = fro_err(host(e.slots()[0]['W1']) * 10.0, g['d_W1'])
            else:
                gerrs['d_W1'] = fro_err((np.asarray(p['W1'], np.float64) - host(e.weights['W1'])) / lr, g['d_W1'])
            print('action %s B=%d C=%d: forward %s loss %.2e gradients %s' % (
                tag, B, C, {k: '%.2e' % v for k, v in errs.items()}, loss_err, {k: '%.2e' % v for k, v in gerrs.items()}))
            assert all(v <= FWD_TOL[dtype] for v in errs.values()), (tag, errs)
            assert loss_err <= LOSS_TOL[dtype] and abs(step_loss - want_loss) <= LOSS_TOL[dtype] * abs(want_loss), (tag, loss_err)
            assert all(v <= GRAD_TOL[dtype] for v in gerrs.values()), (tag, gerrs)


def _three_steps(e, p, c3d, gm, labels):
    e.set_weights(p)
    if e.mode == 'NN':
        for buf in e.slots():
            for t in buf.values():
                t.zero_()
    losses = [e.train_step(c3d, gm, labels, s) for s in range(3)]
    return e.flat_params.clone(), torch.cat(losses)


@pytest.mark.parametrize('B,C', SHAPES)
def test_fused_against_unfused_and_reproducible(gpu, B, C):
    """Three training steps from the same start: the fused and the unfused plan agree to the gradient bounds, and two runs
    of the same plan are bit-identical (no float atomics anywhere)."""
    for mode, use_gazemap in modes_for(C):
        p, c3d_h, gm_h, labels_h = _random_case(400 + B + C, B, C, mode, use_gazemap)
        c3d, gm, labels = dev(c3d_h, gpu), dev(gm_h, gpu), dev(labels_h, gpu)
        for dtype in ('f32', 'bf16'):
            tag = (mode, use_gazemap, dtype)
            fused = ActionEngine(B, C, mode, use_gazemap, dtype, save_for_backward=True, device=gpu)
            unfused = ActionEngine(B, C, mode, use_gazemap, dtype, save_for_backward=True, device=gpu, unfused=True)
            pf, lf = _three_steps(fused, p, c3d, gm, labels)
            pu, lu = _three_steps(unfused, p, c3d, gm, labels)
            for k, off, n in [(k, v.data_ptr(), v.numel()) for k, v in fused.weights.items()]:
                o = (off - fused.flat_params.data_ptr()) // 4
                assert fro_err(host(pf[o:o + n]), host(pu[o:o + n])) <= GRAD_TOL[dtype], (tag, k)
            assert max_err(host(lf), host(lu)) <= LOSS_TOL[dtype], tag
            assert float(lf[0]) != float(lf[2])                      # (the steps did move the model)
            pf2, lf2 = _three_steps(fused, p, c3d, gm, labels)
            pu2, lu2 = _three_steps(unfused, p, c3d, gm, labels)
            assert torch.equal(pf, pf2) and torch.equal(lf, lf2) and torch.equal(pu, pu2) and torch.equal(lu, lu2), tag


def test_classifier_learns_a_separable_task(gpu):
    """Ten single_steps of Classifier (NN with gaze map, f32, C = 24) lower the loss; predict is bit-equal after a
    get_weights -> set_weights round trip."""
    from recurrent_gaze_prediction_amd.models import action_classification as ac
    h = ac.create_standard_hparams()
    h.feat_dimensions, h.use_gazemap = [24, 7, 7], True
    clf = ac.Classifier(h, device=gpu, dtype='f32', seed=3)
    clf.build_model('NN')
    rs = np.random.RandomState(8)
    B = h.batch_size
    labels = np.zeros((B, 13), np.float32)
    labels[np.arange(B), np.arange(B) % 13] = 1.0
    proto = rs.rand(13, 24, 49).astype(np.float32)                 # one feature prototype per class
    c3d = proto[np.arange(B) % 13] + 0.01 * rs.rand(B, 24, 49).astype(np.float32)
    gm = rs.rand(B, 49, 49).astype(np.float32)
    gm /= gm.sum((1, 2), keepdims=True)
    clf.set_weights(dict(clf.get_weights(), Wg=np.full((2401, 49), 1.0, np.float32)))
    losses = [clf.single_step(c3d, gm, labels) for _ in range(10)]
    assert clf.global_step == 10 and losses[-1] < losses[0] and all(np.isfinite(losses))
    y0 = clf.predict(c3d, gm).clone()
    clf.set_weights(clf.get_weights())
    assert torch.equal(clf.predict(c3d, gm), y0)
    s = clf.evaluate(y0.cpu().numpy(), labels)
    assert set(s) == {'Hamming', 'zero-one', 'average-pecision'} and 0.0 <= s['average-pecision'] <= 1.0


def test_create_refuses_bad_arguments_and_call_order(gpu):
    for kwargs in (dict(batch=65), dict(dim_feat=0), dict(batch=0)):
        with pytest.raises(_lib.RgpError) as ei:
            ActionEngine(**dict(dict(batch=4, dim_feat=8, device=gpu), **kwargs))
        assert ei.value.code == -1                                 # RGP_EINVAL
    import ctypes
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_action_create(ctypes.byref(h), 4, 8, _lib.RGP_ACTION_NN, _lib.RGP_BF16, 8) == -1          # unknown flag
    assert lib.rgp_action_create(ctypes.byref(h), 4, 8, 2, _lib.RGP_BF16, 0) == -1                            # unknown mode
    e = ActionEngine(4, 8, 'NN', False, 'bf16', device=gpu)
    c3d = torch.zeros(4, 8, 49, device=gpu)
    with pytest.raises(_lib.RgpError) as ei:
        e.forward(c3d)
    assert ei.value.code == -4                                     # RGP_ESTATE: forward before set_weights
    e.set_weights(syn.action_params(1, 'NN', False, dim_feat=8))
    with pytest.raises(_lib.RgpError) as ei:
        e.train_step(c3d, None, torch.zeros(4, 13, device=gpu), 0)
    assert ei.value.code == -4                                     # not a training plan
    small = torch.empty(256, dtype=torch.uint8, device=gpu)
    assert lib.rgp_action_bind_workspace(e._h, ctypes.c_void_p(small.data_ptr()), 256, None) == -3            # RGP_EWORKSPACE


def test_forward_rows_equals_forward(gpu):
    """conv5b rows (column d*512+c', reference channel 2c'+d) give the logits of the placeholder layout."""
    B = 2
    rs = np.random.RandomState(12)
    p = syn.action_params(4, 'NN', True)
    c3d = np.maximum(rs.randn(B, 1024, 49), 0).astype(np.float32)
    gm = rs.rand(B, 49, 49).astype(np.float32)
    e = ActionEngine(B, 1024, 'NN', True, 'bf16', device=gpu)
    e.set_weights(p)
    t = torch.tensor(c3d, device=gpu).to(torch.bfloat16)                                   # rows carry the operand dtype
    rows = t.reshape(B, 512, 2, 49).permute(0, 3, 2, 1).reshape(B * 49, 1024).contiguous()
    want = e.forward(t.float().contiguous(), dev(gm, gpu))[0].clone()
    assert torch.equal(e.forward_rows(rows, dev(gm, gpu))[0], want)
