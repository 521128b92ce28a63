"""Float64 numpy restatement of the action classifier (reference models/action_classification.py:210-292): forward, loss,
every gradient, TF-Adam / SGD, the learning-rate schedule -- and a generator of EXACT operands, on which every product of
the first layer is bf16-representable and every sum is exact in fp32 in any order, so the device must match bit for bit.

Parameter keys: W1, b1 (+ W2, b2, W3, b3 in 'NN' mode; + Wg with use_gazemap), as engine.ACTION_PARAM_TO_FIELD."""
import math

import numpy as np

HIDDEN, CLASSES, SVM_C = 256, 13, 50.0
KEYS = {'NN': ('W1', 'Wg', 'b1', 'W2', 'b2', 'W3', 'b3'), 'SVM': ('W1', 'Wg', 'b1')}


def f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def learning_rate(step, lr0=0.002, decay=0.96, decay_steps=10):
    """tf.train.exponential_decay, staircase=False (:282-283)."""
    return lr0 * decay ** (step / float(decay_steps))


def projection(p, c3d, gazemap, use_gazemap):
    """:210-240 -> (a [B,49] or None, x [B, 49 C])."""
    B = c3d.shape[0]
    c3d = np.asarray(c3d, np.float64).reshape(B, -1, 49)
    if not use_gazemap:
        return None, c3d.reshape(B, -1)
    a = np.asarray(gazemap, np.float64).reshape(B, 2401) @ p['Wg']
    return a, (c3d * a[:, None, :]).reshape(B, -1)


def forward(p, c3d, gazemap, mode, use_gazemap):
    p = f64(p)
    a, x = projection(p, c3d, gazemap, use_gazemap)
    out = {'a': a, 'x': x, 'h1': x @ p['W1'] + p['b1']}
    if mode == 'NN':
        out['h2'] = out['h1'] @ p['W2'] + p['b2']
        out['logits'] = out['h2'] @ p['W3'] + p['b3']
        out['y_pred'] = 1.0 / (1.0 + np.exp(-out['logits']))
    else:
        out['logits'] = out['y_pred'] = out['h1']
    return out


def loss(p, out, labels, mode):
    labels = np.asarray(labels, np.float64)
    z = out['logits']
    if mode == 'NN':                                  # tf.nn.sigmoid_cross_entropy_with_logits, mean over B x 13
        return float(np.mean(np.maximum(z, 0) - z * labels + np.log1p(np.exp(-np.abs(z)))))
    return float(0.5 * np.sum(np.asarray(p['W1'], np.float64) ** 2) + SVM_C * np.sum(np.maximum(0.0, 1.0 - labels * z)))


def input_grads(p, c3d, gazemap, d_h1, mode, use_gazemap):
    """From d_h1 (NN: d loss / d h1; SVM: d hinge sum / d y, the factor 50 applied here): g = x^T d_h1 (the data term of
    dW1), dx, d_a, d_Wg."""
    p = f64(p)
    B = c3d.shape[0]
    a, x = projection(p, c3d, gazemap, use_gazemap)
    scale = SVM_C if mode == 'SVM' else 1.0
    d_h1 = np.asarray(d_h1, np.float64)
    out = {'g': x.T @ d_h1}
    if use_gazemap:
        out['dx'] = scale * (d_h1 @ p['W1'].T)
        out['d_a'] = (np.asarray(c3d, np.float64).reshape(B, -1, 49) * out['dx'].reshape(B, -1, 49)).sum(1)
        out['d_Wg'] = np.asarray(gazemap, np.float64).reshape(B, 2401).T @ out['d_a']
    return out


def grads(p, c3d, gazemap, labels, mode, use_gazemap):
    """Every gradient of the loss, keyed d_<variable>, plus the intermediates d_logits, d_h2, d_h1, dx, d_a."""
    p = f64(p)
    labels = np.asarray(labels, np.float64)
    out = forward(p, c3d, gazemap, mode, use_gazemap)
    B = labels.shape[0]
    g = {}
    if mode == 'NN':
        g['d_logits'] = (out['y_pred'] - labels) / (B * CLASSES)
        g['d_W3'], g['d_b3'] = out['h2'].T @ g['d_logits'], g['d_logits'].sum(0)
        g['d_h2'] = g['d_logits'] @ p['W3'].T
        g['d_W2'], g['d_b2'] = out['h1'].T @ g['d_h2'], g['d_h2'].sum(0)
        g['d_h1'] = g['d_h2'] @ p['W2'].T
        g['d_b1'] = g['d_h1'].sum(0)
        ig = input_grads(p, c3d, gazemap, g['d_h1'], mode, use_gazemap)
        g['d_W1'] = ig.pop('g')
    else:
        g['d_h1'] = np.where(1.0 - labels * out['h1'] > 0, -labels, 0.0)      # the hinge passes gradient strictly inside
        g['d_b1'] = SVM_C * g['d_h1'].sum(0)
        ig = input_grads(p, c3d, gazemap, g['d_h1'], mode, use_gazemap)
        g['d_W1'] = p['W1'] + SVM_C * ig.pop('g')
    g.update(ig)
    return out, g


def adam(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, c1=None, c2=None):
    """tf.train.AdamOptimizer: lr_t = lr sqrt(1-b2^t)/(1-b1^t), t = step+1; theta -= lr_t m / (sqrt(v) + eps).
    c1 / c2: what a kernel uses for 1-b1 / 1-b2 when it forms them in fp32 (fp32_adam_constants)."""
    t = step + 1
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = b1 * m + ((1 - b1) if c1 is None else c1) * g
    v = b2 * v + ((1 - b2) if c2 is None else c2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def fp32_adam_constants():
    """The constants of rgp_adam_clip_step, which takes beta1 / beta2 as fp32 and forms 1 - beta in fp32 (1.f - 0.999f is
    1.3e-5 away from 0.001) and the beta powers of lr_t from the fp32 values: float64 Adam WITH these constants is the
    oracle of a plan whose W1 takes that kernel."""
    f = np.float32
    return dict(b1=float(f(0.9)), b2=float(f(0.999)), c1=float(f(1) - f(0.9)), c2=float(f(1) - f(0.999)))


def train_step(p, slots, c3d, gazemap, labels, step, mode, use_gazemap, lr=None):
    """One optimizer step in float64 -> (new params, new slots {name: (m, v)}, loss before the update)."""
    p = f64(p)
    out, g = grads(p, c3d, gazemap, labels, mode, use_gazemap)
    l = loss(p, out, labels, mode)
    new, new_slots = {}, {}
    for k in p:
        if mode == 'NN':
            m, v = slots.get(k, (np.zeros_like(p[k]), np.zeros_like(p[k])))
            new[k], m, v = adam(p[k], g['d_' + k], m, v, step, learning_rate(step) if lr is None else lr)
            new_slots[k] = (m, v)
        else:
            new[k] = p[k] - (0.01 if lr is None else lr) * g['d_' + k]
    return new, new_slots, l


# ---- exact operands ------------------------------------------------------------------------------------------------------

def exact_operands(seed, B, C, mode, use_gazemap):
    """c3d integer-valued in [-2, 2]; gazemap one-hot; Wg in {0, 1, 2}; W1 integer-valued in [-2, 2]; d_h1 = k/8, |k| <= 8;
    b1 a multiple of 1/4 in [-1, 1].  Then a in {0,1,2}, x = c3d a an integer in [-4, 4], every product x W1 and d_h1 W1 is
    bf16-representable, the sums of fc1 are integers below 8 K (401 408 at C = 1024) and g, dx multiples of 1/8 below 2^11."""
    rs = np.random.RandomState(seed)
    N = HIDDEN if mode == 'NN' else CLASSES
    K = 49 * C
    ops = {'c3d': rs.randint(-2, 3, size=(B, C, 49)).astype(np.float32),
           'W1': rs.randint(-2, 3, size=(K, N)).astype(np.float32),
           'b1': (rs.randint(-4, 5, size=(N,)) / 4.0).astype(np.float32),
           'd_h1': (rs.randint(-8, 9, size=(B, N)) / 8.0).astype(np.float32)}
    gm = np.zeros((B, 2401), np.float32)
    gm[np.arange(B), rs.randint(0, 2401, size=B)] = 1.0
    ops['gazemap'] = gm.reshape(B, 49, 49)
    if use_gazemap:
        ops['Wg'] = rs.randint(0, 3, size=(2401, 49)).astype(np.float32)
    return ops


def exact_params(ops, seed, mode, use_gazemap):
    """The exact W1 / b1 / Wg with ordinary (seeded) values for the layers behind h1."""
    rs = np.random.RandomState(seed)
    p = {'W1': ops['W1'], 'b1': ops['b1']}
    if use_gazemap:
        p['Wg'] = ops['Wg']
    if mode == 'NN':
        p['W2'] = rs.uniform(-0.1, 0.1, size=(HIDDEN, HIDDEN)).astype(np.float32)
        p['b2'] = np.full((HIDDEN,), 0.05, np.float32)
        p['W3'] = rs.uniform(-0.1, 0.1, size=(HIDDEN, CLASSES)).astype(np.float32)
        p['b3'] = np.full((CLASSES,), 0.05, np.float32)
    return p


def is_bf16(x):
    """Every value survives a round trip through bfloat16 (the low 16 bits of its fp32 pattern are zero)."""
    x32 = np.ascontiguousarray(np.asarray(x, np.float32))
    return bool(np.all(x32 == np.asarray(x, np.float64))) and not np.any(x32.view(np.uint32) & 0xffff)


def check_exact(ops, mode, use_gazemap):
    """Asserts what exact_operands promises; returns the largest sums {'fc1', 'g', 'dx'} (sums of absolute products: a
    bound on every partial sum in every order)."""
    p = f64({k: ops[k] for k in ('W1', 'b1') + (('Wg',) if use_gazemap else ())})
    a, x = projection(p, ops['c3d'], ops['gazemap'], use_gazemap)
    W1, d = p['W1'], np.asarray(ops['d_h1'], np.float64)
    assert is_bf16(x) and is_bf16(W1) and is_bf16(d)
    assert np.all(x == np.round(x)) and np.all(W1 == np.round(W1))
    # every distinct product value of the three contractions
    xv, wv, dv = np.unique(x), np.unique(W1), np.unique(d)
    assert is_bf16(np.outer(xv, wv)) and is_bf16(np.outer(dv, wv)) and is_bf16(np.outer(xv, dv))
    if a is not None:
        assert is_bf16(np.outer(np.unique(ops['c3d']), np.unique(a)))
    bound = {'fc1': float((np.abs(x) @ np.abs(W1)).max()), 'g': float((np.abs(x).T @ np.abs(d)).max()),
             'dx': float((np.abs(d) @ np.abs(W1).T).max()) * (SVM_C if mode == 'SVM' else 1.0)}
    assert bound['fc1'] < 2 ** 24 and bound['fc1'] <= 8 * x.shape[1]
    assert bound['g'] * 8 < 2 ** 24 and bound['dx'] * 8 < 2 ** 24          # multiples of 1/8 (SVM dx: of 1/4 after the factor 50)
    return bound
