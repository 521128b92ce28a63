"""CPU: the exact-operand recipe of tests/c3d_exact_ref.py -- the sparse float64 chain against dense conv3d, the properties
the GPU test relies on (headroom below the fp32 significand, every (tap, cin) probed, non-degenerate activations, bf16
rounding really exercised), and the sensitivity of plain equality to the bugs a relative tolerance cannot see.  No kernel
is launched here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import c3d_exact_ref as ref


def dense_chain(video, p, upto):
    """float64 conv3d + bias + ReLU + max-pool, no rounding -> pooled outputs NDHWC."""
    x = torch.as_tensor(video, dtype=torch.float64).permute(0, 4, 1, 2, 3)
    outs = []
    for name, _, _, pool in ref.SPECS[:upto]:
        w = torch.as_tensor(p[name + '_w'], dtype=torch.float64).permute(4, 3, 0, 1, 2)
        x = torch.relu(F.conv3d(x, w, torch.as_tensor(p[name + '_b'], dtype=torch.float64), padding=1))
        if pool is not None:
            x = F.max_pool3d(x, (pool[0], pool[1], pool[1]))
        outs.append(x.permute(0, 2, 3, 4, 1))
    return outs


def test_sparse_reference_equals_dense_conv3d():
    """One 16x16x16 window through conv1a and conv2a: in float64 with these operands both are exact, so equal; the f32
    chain rounds nowhere and the bf16 chain's conv1a output is already bf16 (multiples of 1/4 below 64)."""
    p = ref.exact_params(0)
    v = ref.exact_video(3, 1, hw=16)
    dense = dense_chain(v, p, 2)
    for dtype in ('f32', 'bf16'):
        got = ref.reference_chain(v, p, dtype, upto='conv2a')
        assert len(got['layers']) == 2 and got['rne_trunc_differ'][0] == 0
        assert ref.first_mismatch(got['layers'][0].double(), dense[0], 'conv1a') is None
        want = dense[1] if dtype == 'f32' else ref.bf16_rne(dense[1])
        assert ref.first_mismatch(got['layers'][1].double(), want, 'conv2a') is None
    # dense random filters (not the recipe) through the same routine: within float64 rounding of conv3d
    rs = np.random.RandomState(0)
    w = rs.randn(3, 3, 3, 3, 4)
    x = torch.as_tensor(rs.randn(2, 5, 6, 7, 3))
    z, absmax = ref.sparse_conv(ref.pad_input(x), w)
    want = F.conv3d(x.permute(0, 4, 1, 2, 3), torch.as_tensor(w).permute(4, 3, 0, 1, 2), padding=1).permute(1, 0, 2, 3, 4)
    assert float((z - want).abs().max()) < 1e-12
    want_abs = F.conv3d(x.abs().permute(0, 4, 1, 2, 3), torch.as_tensor(w).abs().permute(4, 3, 0, 1, 2), padding=1)
    assert abs(absmax - float(want_abs.max())) < 1e-12


@pytest.fixture(scope='module')
def reduced():
    """Both filter sets on one 16x32x32 window (the stack pools it down to 2x2x2)."""
    v = ref.exact_video(5, 1, hw=32)
    return v, [(p, ref.reference_chain(v, p, 'bf16')) for p in (ref.exact_params(0), ref.exact_params(1))]


def test_operands_are_exact_in_bf16():
    v = torch.as_tensor(ref.exact_video(5, 2, hw=16))
    assert torch.equal(v.bfloat16().float(), v) and float(v.min()) == -ref.VIDEO_MAX and float(v.max()) == ref.VIDEO_MAX
    assert not torch.equal(v[0], v[1])
    for nnz in (32, 16):
        a, b = ref.exact_params(0, nnz), ref.exact_params(1, nnz)
        for i, (name, cin, cout, _) in enumerate(ref.SPECS):
            w = a[name + '_w']
            assert w.shape == (3, 3, 3, cin, cout) and w.dtype == np.float32
            assert set(np.unique(w)) == {-ref.W_MAG, 0.0, ref.W_MAG}
            assert ((w != 0).reshape(-1, cout).sum(0) == nnz).all()
            bias = a[name + '_b']
            assert np.array_equal(np.round(bias * 4), bias * 4) and (bias != 0).mean() > (0.5 if nnz == 32 else 0.1)
            assert float(np.abs(bias).max()) < 64          # multiples of 1/4 below 64: 8 significant bits, exact in bf16 too
            assert not np.array_equal(w, b[name + '_w'])


def test_recipe_properties(reduced):
    _, sets = reduced
    for p, chain in sets:
        print('headroom bits', ['%.1f' % b for b in chain['headroom_bits']], 'zeros', ['%.2f' % z for z in chain['zero_frac']],
              'rne != trunc', chain['rne_trunc_differ'])
        assert all(chain['exact_in_f32'])
        assert max(chain['headroom_bits']) <= 23
        assert all(0.01 < z < 0.90 for z in chain['zero_frac']), chain['zero_frac']
        for i in range(8):
            assert ref.probed_k(p, i).all(), 'a (tap, cin) of %s is multiplied by no filter' % ref.NAMES[i]
        assert max(chain['rne_trunc_differ']) > 0
        assert chain['rows'].dtype == torch.bfloat16 and chain['rows'].shape == (4, 1024)
        # rows [y*w+x, d*512+c] and features [c*2+d, y, x] are two views of conv5b
        last = chain['layers'][7]
        assert torch.equal(chain['features'][0, 2 * 37 + 1, 1, 0], last[0, 1, 1, 0, 37])
        assert torch.equal(chain['rows'][1 * 2 + 0, 512 + 37].float(), last[0, 1, 1, 0, 37])
    assert ref.first_mismatch(sets[0][1]['features'], sets[1][1]['features'], 'features') is not None


def test_f32_recipe_properties():
    """nnz = 16 without the bf16 step: the lsb shrinks by two bits per layer and everything still fits fp32."""
    v = ref.exact_video(5, 1, hw=32)
    chain = ref.reference_chain(v, ref.exact_params(0, nnz=16), 'f32')
    assert all(chain['exact_in_f32']) and max(chain['headroom_bits']) <= 23
    assert chain['unit_exp'] == [-2 * (i + 1) for i in range(8)]
    assert all(0.01 < z < 0.90 for z in chain['zero_frac']), chain['zero_frac']
    assert chain['rows'].dtype == torch.float32


@pytest.fixture(scope='module')
def tiny():
    """One 16x16x16 window, filter set 0: the unmutated chain of the sensitivity tests."""
    v = ref.exact_video(7, 1, hw=16)
    p = ref.exact_params(0)
    return v, p, ref.reference_chain(v, p, 'bf16')


def _differs(base, mutated, layer):
    """Layers before `layer` equal, `layer` reported with coordinates."""
    for i in range(layer):
        assert ref.first_mismatch(mutated['layers'][i], base['layers'][i], ref.NAMES[i]) is None
    msg = ref.first_mismatch(mutated['layers'][layer], base['layers'][layer], ref.NAMES[layer])
    assert msg is not None and msg.startswith(ref.NAMES[layer] + ': ') and 'got' in msg and 'want' in msg, msg
    return msg


@pytest.mark.parametrize('layer', [0, 2, 5])
def test_equality_sees_one_missing_product(tiny, layer):
    v, p, base = tiny
    name = ref.NAMES[layer]
    q = dict(p)
    w = p[name + '_w'].copy()
    cin = w.shape[3]
    entries = np.argwhere(w.reshape(-1, w.shape[-1]) != 0)
    # a centre-tap entry: it multiplies real data at every output position, however small the image has become
    k, cout = entries[entries[:, 0] // cin == 13][11]
    w.reshape(-1, w.shape[-1])[k, cout] = 0.0
    q[name + '_w'] = w
    got = ref.reference_chain(v, q, 'bf16', upto=name)
    print(_differs(base, got, layer))
    # the report names the output channel of the removed product and nothing else
    got = got['layers'][layer]
    bad = torch.nonzero(got != base['layers'][layer])
    assert set(bad[:, 4].tolist()) == {int(cout)}


def test_equality_sees_a_stale_halo_element(tiny):
    v, p, base = tiny
    # conv3a's padded input [128, 1, 10, 10, 10]: plane z = 0 is halo
    mutated = ref.reference_chain(v, p, 'bf16', halo=(2, (5, 0, 0, 3, 4), 1.0), upto='conv3a')
    _differs(base, mutated, 2)
    bad = torch.nonzero(mutated['layers'][2] != base['layers'][2])
    assert int(bad[:, 1].max()) == 0 and bad.shape[0] < 27 * 256          # only output plane 0, next to the halo


def test_equality_sees_truncation(tiny):
    v, p, base = tiny
    first = next(i for i, c in enumerate(base['rne_trunc_differ']) if c)
    mutated = ref.reference_chain(v, p, 'bf16', rounding='trunc', upto=ref.NAMES[first])
    _differs(base, mutated, first)
    a, b = mutated['layers'][first], base['layers'][first]
    assert int((a != b).sum()) == base['rne_trunc_differ'][first]
    assert float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()) <= 2.0 ** -7      # one bf16 ulp: far below 3e-2


def test_equality_sees_one_dropped_bias(tiny):
    v, p, base = tiny
    q = dict(p)
    b = p['conv4b_b'].copy()
    c = int(np.flatnonzero(b)[3])
    b[c] = 0.0
    q['conv4b_b'] = b
    mutated = ref.reference_chain(v, q, 'bf16', upto='conv4b')
    _differs(base, mutated, 5)
    assert set(torch.nonzero(mutated['layers'][5] != base['layers'][5])[:, 4].tolist()) == {c}


def test_first_mismatch_report():
    want = torch.zeros(2, 3, 4, 5, 6)
    got = want.clone()
    assert ref.first_mismatch(got, want, 'conv2a') is None
    got[1, 2, 0, 4, 3] = 0.5
    got[1, 2, 3, 4, 5] = -1.0
    msg = ref.first_mismatch(got, want, 'conv2a')
    assert msg.splitlines()[0] == 'conv2a: 2 of 720 elements differ; first at (window, z, y, x, c):'
    assert '(1, 2, 0, 4, 3) got 0.5 want 0.0' in msg and '(1, 2, 3, 4, 5) got -1.0 want 0.0' in msg
    assert 'shape' in ref.first_mismatch(got[:1], want, 'conv2a')
    assert ref.first_mismatch(got.bfloat16(), got, 'rows') is None          # compared by value across dtypes
