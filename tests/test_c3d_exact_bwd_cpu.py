"""CPU: the exact-operand recipe for the conv-stack BACKWARD (tests/c3d_exact_ref.py: light_params, tap_complete_params,
exact_upstream, backward_chain).  Three things are settled here, without a kernel:

* the float64 chain is the gradient: on a light case whose gradient images the bf16 store leaves alone it equals float64
  autograd of conv3d + relu + max_pool3d (the forward's bf16 rounding applied as a straight-through constant) in every
  gradient image, filter gradient and bias gradient;
* the premises of bit-for-bit equality hold at 112 x 112 on the very cases tests/test_c3d_exact_bwd_gpu.py compares with
  (headroom below the fp32 significand, tied pooling windows on every pooled layer and every code used, no filter-gradient
  entry that nothing contributes to -- which takes two cases, W and T --, every (tap, cout) and (tap, cin) of the tap-complete set probed, the 67-window
  combination inside the significand);
* plain equality sees what a relative bound of 1.5e-2 does not: each seeded fault changes the chain, and the test prints in
  how many elements.

Measured (8 threads): the 112 x 112 chains of cases W, T and D 8 s, 5 s and 9 s, the 32 x 32 chains 2 ... 4 s each, 55 s for the
file; the faults change 1 (dropped product) ... 4 317 547 (`>= 0` gate, d conv5a_w) elements."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import c3d_exact_ref as ref

TOL_BITS = 23          # headroom that leaves fp32 accumulation exact in any order (24-bit significand, one bit spare)


def autograd_chain(video, p, g, dtype):
    """float64 autograd -> (gradient images NDHWC, {name: gradient} with filters in DHWIO)."""
    x = torch.as_tensor(video, dtype=torch.float64).permute(0, 4, 1, 2, 3)
    tp, zs = {}, []
    for name, _, _, pool in ref.SPECS:
        w = torch.as_tensor(p[name + '_w'], dtype=torch.float64).permute(4, 3, 0, 1, 2).contiguous().requires_grad_()
        b = torch.as_tensor(p[name + '_b'], dtype=torch.float64).requires_grad_()
        tp[name + '_w'], tp[name + '_b'] = w, b
        z = F.conv3d(x, w, b, padding=1)
        z.retain_grad()
        zs.append(z)
        x = torch.relu(z)
        if pool is not None:
            x = F.max_pool3d(x, (pool[0], pool[1], pool[1]))
        if dtype == 'bf16':
            x = x + (ref.bf16_rne(x.detach()) - x.detach())
    (x * torch.as_tensor(g, dtype=torch.float64)).sum().backward()          # x [n,512,2,h,w] against g [n,1024,h,w]: see caller
    grads = {k: (v.grad.permute(2, 3, 4, 1, 0) if k.endswith('_w') else v.grad) for k, v in tp.items()}
    return [z.grad.permute(0, 2, 3, 4, 1) for z in zs], grads


@pytest.mark.parametrize('dtype,nnz', [('bf16', 8)])
def test_backward_chain_equals_autograd(dtype, nnz):
    """Two 16x32x32 windows, light filters: nothing in the backward rounds (asserted), so the chain must be float64
    autograd exactly -- integers throughout.  bf16 with 8 entries per filter: activations pass 256, so the forward's store
    does round (asserted) and the straight-through constant matters."""
    p = ref.light_params(0, nnz)
    v = ref.exact_video(11, 2, hw=32)
    g = ref.exact_upstream(12, 2, hw=2)
    chain = ref.backward_chain(v, p, g, dtype)
    assert all(c == 0 for c in chain['rounded_elems'].values()), chain['rounded_elems']
    assert all(chain['exact_in_f32'].values())
    assert (sum(chain['fwd_rounded_elems']) > 0) == (dtype == 'bf16'), chain['fwd_rounded_elems']
    n = v.shape[0]
    g5 = torch.as_tensor(g).reshape(n, 512, 2, 2, 2)                          # features channel c*2+d -> [n,c,d,h,w]
    for j in range(n):          # window by window: the chain keeps the windows' gradients apart
        dys, grads = autograd_chain(v[j:j + 1], p, g5[j:j + 1], dtype)
        for i, name in enumerate(ref.NAMES):
            assert ref.first_mismatch(chain['dys'][i][j:j + 1].double(), dys[i], name + ' dY') is None
        for k in grads:
            assert float(grads[k].abs().max()) > 0
            msg = ref.first_mismatch(chain['grads'][j][k], grads[k], k)
            assert msg is None, msg
    mine, _ = ref.combine_windows(chain, [2, 1])
    assert all(torch.equal(mine[k], 2 * chain['grads'][0][k] + chain['grads'][1][k]) for k in mine)


def test_operands():
    for nnz in (4, 8):
        a, b = ref.light_params(0, nnz), ref.light_params(1, nnz)
        for name, cin, cout, _ in ref.SPECS:
            w = a[name + '_w']
            assert w.shape == (3, 3, 3, cin, cout) and w.dtype == np.float32 and set(np.unique(w)) == {-1.0, 0.0, 1.0}
            assert ((w != 0).reshape(-1, cout).sum(0) == nnz).all()
            wk = w.reshape(27, cin, cout)          # pairs: +1 and -1 on the same input channel at two taps
            assert (wk.sum(0) == 0).all() and ((wk != 0).sum(0) % 2 == 0).all()
            assert (w != 0).any(axis=(0, 1, 2, 4)).all(), 'an input channel of %s is multiplied by no filter' % name
            bias = a[name + '_b']
            assert np.array_equal(np.round(bias), bias) and float(np.abs(bias).max()) <= 8 and (bias != 0).mean() > 0.4
            assert not np.array_equal(w, b[name + '_w'])
    t = ref.tap_complete_params(0)
    for name, cin, cout, _ in ref.SPECS:
        w = t[name + '_w'].reshape(27, cin, cout)
        assert set(np.unique(w)) == {-ref.W_MAG, 0.0, ref.W_MAG}
        assert ((w != 0).sum(1) == 1).all(), 'one entry per (tap, cout)'
        assert (w != 0).any(2).all(), 'every (tap, cin)'
    g = ref.exact_upstream(3, 2)
    assert g.shape == (2, 1024, 7, 7) and set(np.unique(g)) == {-1.0, 0.0, 1.0} and 0.6 < (g != 0).mean() < 0.73
    g = ref.exact_upstream(3, 1, density=0.3, gmax=2)
    assert set(np.unique(g)) == {-2.0, -1.0, 0.0, 1.0, 2.0} and 0.27 < (g != 0).mean() < 0.33


def test_premises_of_cases_w_and_t_at_112():
    """The chains the GPU file compares every light-filter run with.

    'Every entry of every filter gradient has a non-zero sum |x dy|' needs both.  Case W delivers it on conv1a ... conv3b
    (asserted: not one entry out of 5 184 ... 1 769 472 without a contribution).  On the 14 x 14 and 7 x 7 layers -- 2 x 784
    and 2 x 98 positions per channel, routed gradient channels with a few dozen non-zero positions -- its gates and routes
    leave 1 / 45 698 / 687 765 / 1 371 903 entries (up to 19 %) of conv4a / conv4b / conv5a / conv5b without any; those must
    still come out as exactly 0 over stale data, but a contribution missing from them could not be noticed.  Case T is case W
    with all-positive filters and biases from conv4a up and an upstream gradient of +-1 everywhere: no activation or
    gradient element of those layers is zero, and every entry of their four filter gradients is reached (asserted)."""
    _, _, _, chain = ref.case_w()
    print('case W:', ref.describe_chain(chain))
    hb = chain['headroom_bits']
    assert len(hb) == 24 and max(hb.values()) <= TOL_BITS, hb
    assert all(chain['exact_in_f32'].values())
    assert all(v == 0 for v in chain['rounded_elems'].values())                  # integers below 256: the store is exact
    assert sum(chain['fwd_rounded_elems']) == 0          # ... in the forward too: this chain is also the f32 plan's
    for i in ref.POOLED:
        name = ref.NAMES[i]
        assert chain['tied_frac'][name] > 0.05, (name, chain['tied_frac'][name])
        assert min(chain['code_hist'][name]) > 0, (name, chain['code_hist'][name])
    assert all(chain['untouched'][nm + '_w'] == 0 for nm in ref.NAMES[:ref.TOP]), chain['untouched']
    assert all(0.01 < float((l == 0).float().mean()) < 0.7 for l in chain['layers'])          # every ReLU gate has both sides
    _, _, _, top = ref.case_t()
    print('case T:', ref.describe_chain(top))
    assert len(top['headroom_bits']) == 3 * (8 - ref.TOP) and max(top['headroom_bits'].values()) <= TOL_BITS, top['headroom_bits']
    assert all(top['exact_in_f32'].values())
    assert all(top['untouched'][nm + '_w'] == 0 for nm in ref.NAMES[ref.TOP:]), top['untouched']
    assert all(torch.equal(a, b) for a, b in zip(top['layers'][:ref.TOP], chain['layers']))   # the same stack below conv4a
    assert all(float((l == 0).float().sum()) == 0 for l in top['layers'][ref.TOP:])
    assert min(top['fwd_rounded_elems'][ref.TOP + 1:]) > 0          # activations pass 256: the forward's bf16 store rounds
    assert top['tied_frac']['conv4b'] > 0.01 and min(top['code_hist']['conv4b']) > 0
    # the partition-edge references: 2 A + B (3 windows), 3 A + 2 B (5 windows), 34 A + 33 B (67 windows)
    for coeffs in ([2, 1], [3, 2], [34, 33]):
        for which in (chain, top):
            grads, bits = ref.combine_windows(which, coeffs)
            print('combination', coeffs, 'headroom bits up to %.1f' % max(bits.values()))
            assert max(bits.values()) <= TOL_BITS, bits
            assert all(torch.equal(t.float().double(), t) for t in grads.values())


def test_premises_of_case_d_at_112():
    """Tap-complete filters: the gradient images are exact and their store rounds; the filter gradients are not exact."""
    p, _, _, chain = ref.case_d()
    print('case D:', ref.describe_chain(chain))
    hb = chain['headroom_bits']
    assert max(hb[nm + '_dy'] for nm in ref.NAMES) <= TOL_BITS, hb
    assert all(chain['exact_in_f32'][nm + '_dy'] for nm in ref.NAMES)
    assert all(chain['rounded_elems'][nm + '_dy'] > 0 for nm in ref.NAMES[:3]), chain['rounded_elems']
    assert max(hb[nm + '_w'] for nm in ref.NAMES) > TOL_BITS           # which is why case W exists
    for i, (name, cin, cout, _) in enumerate(ref.SPECS):
        w = p[name + '_w'].reshape(27, cin, cout) != 0
        assert w.any(1).all() and w.any(2).all() and ref.probed_k(p, i).all()


@pytest.fixture(scope='module')
def small_light():
    p = ref.light_params(0, ref.LIGHT_NNZ)
    v = ref.exact_video(21, 1, hw=32)
    g = ref.exact_upstream(22, 1, hw=2)
    return p, v, g, ref.backward_chain(v, p, g, 'bf16', bounds=False)


def _changed(base, mutated):
    """{tensor name: number of differing elements} over the gradient images and the gradients of window 0."""
    out = {}
    for i, name in enumerate(ref.NAMES):
        c = int((base['dys'][i] != mutated['dys'][i]).sum())
        if c:
            out[name + '_dy'] = c
    for k, t in base['grads'][0].items():
        c = int((t != mutated['grads'][0][k]).sum())
        if c:
            out[k] = c
    return out


def test_f32_chain_is_the_bf16_chain_where_no_store_rounds(small_light):
    """What lets the GPU file compare the f32 plan with case W's chain."""
    p, v, g, base = small_light
    assert sum(base['fwd_rounded_elems']) == 0 and all(c == 0 for c in base['rounded_elems'].values())
    f32 = ref.backward_chain(v, p, g, 'f32', bounds=False)
    assert _changed(base, f32) == {} and all(torch.equal(a, b) for a, b in zip(base['layers'], f32['layers']))


def test_equality_sees_a_dropped_product_and_a_short_bias_sum(small_light):
    """One x * dy product of one window missing from one filter-gradient entry of conv3b; 32 positions (one block's rows)
    missing from conv4a's bias sum.  Neither propagates: exactly that entry, and only channels of that bias, change."""
    p, v, g, base = small_light
    mutated = ref.backward_chain(v, p, g, 'bf16', bounds=False, fault={'drop_product': (3, 0), 'bias_block': (4, 0, 32)})
    diff = _changed(base, mutated)
    print('dropped product / short bias sum:', diff, mutated['fault_info'])
    assert set(diff) == {'conv3b_w', 'conv4a_b'} and diff['conv3b_w'] == 1 and diff['conv4a_b'] >= 1
    tap, ci, co = mutated['fault_info']['drop_product']
    a, b = base['grads'][0]['conv3b_w'].reshape(27, 256, 256), mutated['grads'][0]['conv3b_w'].reshape(27, 256, 256)
    assert a[tap, ci, co] != b[tap, ci, co]
    print('  the entry changes by %g, the largest entry of this 32 x 32 case is %g' % (float(a[tap, ci, co] - b[tap, ci, co]), float(a.abs().max())))


def test_equality_sees_the_last_maximum(small_light):
    p, v, g, base = small_light
    mutated = ref.backward_chain(v, p, g, 'bf16', bounds=False, fault={'route': 'last'})
    diff = _changed(base, mutated)
    print('last instead of first maximum:', diff)
    assert all(torch.equal(a, b) for a, b in zip(base['layers'], mutated['layers']))          # the forward is the same
    assert all(ref.NAMES[i] + '_dy' in diff for i in ref.POOLED), diff
    assert all(nm + '_w' in diff for nm in ref.NAMES[:6]), diff
    for i in ref.POOLED:          # the same gradients on other members: every window sum is unchanged
        pd, ph = ref.SPECS[i][3]
        win = lambda t: ref._to_win(t.permute(4, 0, 1, 2, 3), pd, ph).sum(-1)
        assert torch.equal(win(base['dys'][i]), win(mutated['dys'][i])) or i < 5


def test_equality_sees_a_gate_that_lets_zero_through(small_light):
    p, v, g, base = small_light
    mutated = ref.backward_chain(v, p, g, 'bf16', bounds=False, fault={'gate': 'ge'})
    diff = _changed(base, mutated)
    print('>= 0 gate:', diff)
    assert all(nm + '_dy' in diff for nm in ref.NAMES), diff
    # conv5b's image: exactly the upstream elements whose activation is zero and whose gradient is not
    g5 = torch.as_tensor(g).reshape(1, 512, 2, 2, 2).permute(0, 2, 3, 4, 1)
    assert diff['conv5b_dy'] == int(((base['layers'][7] == 0) & (g5 != 0)).sum())


def test_equality_sees_two_swapped_taps(small_light):
    """Taps 4 and 22 of conv4a's rotated filter (the input gradient that becomes conv3b's image)."""
    p, v, g, base = small_light
    mutated = ref.backward_chain(v, p, g, 'bf16', bounds=False, fault={'swap_taps': (4, 4, 22)})
    diff = _changed(base, mutated)
    print('two taps of the rotated filter swapped:', diff)
    assert 'conv3b_dy' in diff and 'conv3b_w' in diff and not any(k.startswith(('conv4', 'conv5')) for k in diff), diff
    err = (base['dys'][3] - mutated['dys'][3]).abs().max() / base['dys'][3].abs().max()
    print('  max-abs error of the image relative to its maximum: %.3f' % float(err))


def test_equality_sees_a_truncating_gradient_store():
    """Tap-complete filters (the light case's images never round): truncation differs exactly where the chain says."""
    p = ref.tap_complete_params(0)
    v = ref.exact_video(23, 1, hw=32)
    g = ref.exact_upstream(24, 1, density=0.3, gmax=2, hw=2)
    base = ref.backward_chain(v, p, g, 'bf16', bounds=False)
    mutated = ref.backward_chain(v, p, g, 'bf16', bounds=False, fault={'store': 'trunc'})
    diff = _changed(base, mutated)
    print('truncating store:', diff, 'rounded', base['rounded_elems'])
    first = max(i for i, nm in enumerate(ref.NAMES) if mutated['rounded_elems'][nm + '_dy'])      # highest image that differs
    assert first <= 6 and base['rounded_elems'][ref.NAMES[first] + '_dy'] > 0
    assert diff[ref.NAMES[first] + '_dy'] == mutated['rounded_elems'][ref.NAMES[first] + '_dy']
    a, b = base['dys'][first], mutated['dys'][first]
    assert float(((a - b).abs() / a.abs().clamp_min(1e-30)).max()) <= 2.0 ** -7                    # one bf16 ulp
